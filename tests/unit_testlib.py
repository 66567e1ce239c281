"""The unit layer's Python side (a plain module, not a conftest): the ctypes loader of the test-only harness libraries
(tests/unit/tsidb_unit.hip, built by __graft_entry__.build()), ulp helpers, the mpmath truths at 50 digits, and the
same-precision numpy restatements of the device routines exactly as the headers write them.

Gates (one rule, used by every tests/test_gpu_unit_*.py):
  exact answer exists     -> bit equality
  textbook bound exists   -> that bound, computed per case in longdouble / mpmath
  otherwise               -> 8 x the error of the same-precision restatement against the mpmath truth on the same inputs,
                             + 8 ulp of the output's scale (the device may differ from the restatement by contraction,
                             operation order and its own acos / sin / rsq: a handful of differently rounded operations)
The harness indexes only what n and the fixed 64-lane layout imply; Harness.call refuses every buffer whose dtype, device,
contiguity or element count is not exactly what the entry point reads or writes, so no test can fault the device."""
import ctypes as C
import math
import sys
from fractions import Fraction
from pathlib import Path

import mpmath
import numpy as np

ROOT = Path(__file__).resolve().parent.parent
UNIT = ROOT / "tests" / "unit"
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
ROBOTS = {"v1": ("libtsidb_unit.so", "op3_v1.tsidb", "tsidb_topology.hpp", "libtsidb.so"),
          "v0": ("libtsidb_unit_v0.so", "op3_v0.tsidb", "tsidb_topology_v0.hpp", "libtsidb_v0.so")}
WAVE = 64
mpmath.mp.dps = 50
mpf = mpmath.mpf

# entry point -> its arguments in order: "i" = a scalar int, (dtype name, elements per n, fixed elements) = a buffer
_T = {"f32": "float32", "f64": "float64", "i32": "int32"}


def _specs():
    s = {}
    for t in ("f32", "f64"):
        d = _T[t]
        s[f"wave_sum_{t}"] = s[f"wave_min_{t}"] = s[f"lane63_{t}"] = [(d, 64, 0), (d, 64, 0)]
        s[f"rdlane_{t}"] = [(d, 64, 0), (d, 4096, 0)]
        s[f"wave_sum3_{t}"] = [(d, 64, 0)] * 6
        s[f"wave_argmin_{t}"] = [(d, 64, 0), ("int32", 64, 0), (d, 64, 0), ("int32", 64, 0)]
        s[f"subtree_sum32_{t}"] = s[f"bperm_{t}"] = s[f"bcast_{t}"] = [(d, 64, 0), ("int32", 64, 0), (d, 64, 0)]
        s[f"rdlane_dyn_{t}"] = [(d, 64, 0), ("int32", 64, 0), (d, 4096, 0)]
        s[f"rsqrt_{t}"] = s[f"rcp_{t}"] = [(d, 1, 0), (d, 1, 0)]
        s[f"quat_to_R_{t}"] = [(d, 4, 0), (d, 9, 0)]
        s[f"mat_to_quat_{t}"] = [(d, 9, 0), (d, 4, 0)]
        s[f"make_frame_{t}"] = [(d, 3, 0)] * 3
        s[f"tri_closest_{t}"] = [(d, 9, 0), (d, 1, 0), (d, 3, 0)]
        s[f"log6_{t}"] = [(d, 9, 0), (d, 3, 0), (d, 6, 0)]
        s[f"terrain_h_{t}"] = [(d, 0, 20), (d, 2, 0), (d, 1, 0)]
        # (NV-dependent counts are written as callables of the harness)
        s[f"chol26_solve_{t}"] = s[f"chol26_dense_{t}"] = [(d, "NV2", 0), (d, 64, 0), (d, "64NV", 0), (d, 64, 0), ("int32", 64, 0)]
        s[f"chol26_factor_subst_{t}"] = [(d, "NV2", 0), (d, 64, 0), (d, "64NV", 0), (d, 64, 0), (d, 64, 0), ("int32", 64, 0)]
    for name, d in (("tick_chol_f64_dpp", "float64"), ("tick_chol_f64", "float64"), ("tick_chol_f32", "float32")):
        s[name] = [(d, "NV2", 0), (d, "64NV", 0), (d, 64, 0), ("int32", 64, 0)]
    s["sincos_f64"] = [("float64", 1, 0)] * 3     # (the float overload is sinf / cosf: nothing of the project's to test)
    s["wave_sum_int"] = s["wave_min_i32"] = s["lane63_i32"] = [("int32", 64, 0), ("int32", 64, 0)]
    s["env_of_block"] = [("int32", 1, 0)]
    s["row_dup"] = ["i", ("float64", 64, 0), ("float64", 0, 2), ("float64", 64, 0), ("float64", 64, 0)]
    s["bcast_fnma"] = ["i", "i", ("float64", 64, 0), ("float64", 0, 2), ("float64", 64, 0), ("float64", 2048, 0), ("float64", 2048, 0)]
    s["bcast_fnma2"] = ["i", "i", ("float64", 64, 0), ("float64", 0, 2), ("float64", 2048, 0), ("float64", 128, 0), ("float64", 128, 0)]
    return s


SPECS = _specs()
EXPORTS = sorted(["tsidbu_dims", "tsidbu_chol26_rank1_f32", "tsidbu_chol26_rank1_f64"] + ["tsidbu_" + k for k in SPECS])
_loaded = {}


class Harness:
    """One harness library (one robot): dims, mask tables and checked calls."""

    def __init__(self, robot):
        path = UNIT / ROBOTS[robot][0]
        if not path.exists():
            raise RuntimeError(f"{path} is missing: python -c 'import __graft_entry__ as g; g.build()'")
        import torch  # noqa: F401  (its HIP runtime must be the one the process initialises: tsid_control_amd/_lib.py)
        self.robot, self.path = robot, path
        self.L = C.CDLL(str(path))
        d4, anc, m1, m2 = (C.c_int * 4)(), (C.c_uint * 32)(), (C.c_uint * 64)(), (C.c_uint * 64)()
        self.L.tsidbu_dims.restype = C.c_int
        assert self.L.tsidbu_dims(d4, anc, m1, m2) == 0
        self.NV, nf, nf2, self.LDM = (int(x) for x in d4)
        self.dofanc = [int(x) for x in anc][:self.NV]
        self.fnma_masks, self.fnma2_masks = [int(x) for x in m1][:nf], [int(x) for x in m2][:nf2]

    def _count(self, per, fixed, n):
        per = {"NV2": self.NV * self.NV, "64NV": 64 * self.NV}.get(per, per)
        return per * n + fixed

    def _ptr(self, t, dtype, count, what):
        import torch
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{what}: needs a CUDA tensor")
        if str(t.dtype) != "torch." + dtype:
            raise ValueError(f"{what}: dtype {t.dtype}, the entry point takes {dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: not contiguous")
        if t.numel() != count:
            raise ValueError(f"{what}: {t.numel()} elements, the entry point touches exactly {count}")
        return C.c_void_p(t.data_ptr())

    def call(self, name, *args, n):
        """tsidbu_<name>(*args, n, current stream), every buffer checked against SPECS first; raises on a non-zero return"""
        import torch
        spec = SPECS[name]
        if len(args) != len(spec) or not isinstance(n, int) or n <= 0:
            raise ValueError(f"{name}: {len(spec)} arguments and a positive n")
        cargs = []
        for k, (a, sp) in enumerate(zip(args, spec)):
            if sp == "i":
                cargs.append(C.c_int(int(a)))
            else:
                cargs.append(self._ptr(a, sp[0], self._count(sp[1], sp[2], n), f"{name} argument {k}"))
        f = getattr(self.L, "tsidbu_" + name)
        f.restype = C.c_int
        rc = f(*cargs, C.c_int(n), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(f"tsidbu_{name} returned {rc}")

    def rank1(self, t, Uin, rdv_in, xs, sigma, chain, m, U, rdv, done, n):
        import torch
        d = _T[t]
        name = f"chol26_rank1_{t}"
        if not isinstance(n, int) or not isinstance(m, int) or n <= 0 or m <= 0:
            raise ValueError("rank1: positive n and m")
        nv = self.NV
        cargs = [self._ptr(Uin, d, n * nv * nv, name + " Uin"), self._ptr(rdv_in, d, n * 64, name + " rdv_in"),
                 self._ptr(xs, d, n * m * 64, name + " xs"), self._ptr(sigma, d, n * m, name + " sigma"),
                 self._ptr(chain, "int64", n * m, name + " chain"), C.c_int(m), self._ptr(U, d, n * 64 * nv, name + " U"),
                 self._ptr(rdv, d, n * 64, name + " rdv"), self._ptr(done, "int32", n * 64, name + " done")]
        f = getattr(self.L, "tsidbu_" + name)
        f.restype = C.c_int
        rc = f(*cargs, C.c_int(n), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(f"tsidbu_{name} returned {rc}")


def harness(robot):
    if robot not in _loaded:
        _loaded[robot] = Harness(robot)
    return _loaded[robot]


def header_dofanc(robot):
    import re
    txt = (ROOT / "tsid_control_amd" / "csrc" / ROBOTS[robot][2]).read_text()
    m = re.search(r"constexpr unsigned MJ_DOFANC\[\] = \{([^}]*)\};", txt)
    return [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]


def report(name, **kv):
    """the measured worst error per bucket, as every GPU test prints it (profiles/unit_primitives.txt is this output)"""
    print("UNIT " + name + " " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


# ---------------------------------------------------------------------------------------------- ulp helpers, exact FMA
def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def ulp(x, dtype=np.float64):
    """spacing of the floats at |x| (array)"""
    return np.spacing(np.abs(np.asarray(x, dtype=dtype))).astype(np.float64)


def to_mp(x):
    """exact mpf of a numpy float (float32 / float64 are binary fractions)"""
    return mpf(float(x))


def mp_err(dev, truth):
    """|dev - truth| as floats, truth a list of mpf"""
    return np.array([float(abs(to_mp(d) - t)) for d, t in zip(np.asarray(dev).reshape(-1), truth)])


def fma_exact(a, b, c):
    """fma(a, b, c) rounded once (Python 3.10 has no math.fma): exact rational, int / int true division rounds correctly"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c  # the sign of an exact zero follows IEEE addition of the exact product's sign and c's
    return r.numerator / r.denominator


def gamma(k, dtype=np.float64):
    """Higham's gamma_k = k u / (1 - k u), u = the unit round-off of dtype, in longdouble"""
    u = np.longdouble(np.finfo(dtype).eps) / 2
    return k * u / (1 - k * u)


# ---------------------------------------------------------------------------------------------- trees
def subtree_last(parent):
    """last index of every node's subtree in a pre-order numbered tree (parent[0] = -1)"""
    n = len(parent)
    last = list(range(n))
    for j in range(n - 1, 0, -1):
        p = int(parent[j])
        last[p] = max(last[p], last[j])
    return last


def random_preorder_tree(rng, n):
    """parent array of a random tree numbered depth-first pre-order: node j hangs off a node on the path of j - 1"""
    parent = [-1]
    for j in range(1, n):
        path, a = [], j - 1
        while a >= 0:
            path.append(a)
            a = parent[a]
        parent.append(int(path[rng.integers(len(path))]))
    return parent


# ---------------------------------------------------------------------------------------------- sincos, rsqrt, rcp truths
def sincos_restated(x):
    """sincos_t(double) as tsidb_common.hpp writes it, float64 numpy scalars and exact FMAs"""
    S = [1.58969099521155010221e-10, -2.50507602534068634195e-08, 2.75573137070700676789e-06, -1.98412698298579493134e-04,
         8.33333333332248946124e-03, -1.66666666666666324348e-01]
    Cc = [-1.13596475577881948265e-11, 2.08757232129817482790e-09, -2.75573143513906633035e-07, 2.48015872894767294178e-05,
          -1.38888888888741095749e-03, 4.16666666666666019037e-02]
    x = float(x)
    k = float(np.rint(x * 0.63661977236758134308))
    r = fma_exact(-k, 1.57079632679489655800e+00, x)
    r = fma_exact(-k, 6.12323399573676603587e-17, r)
    z = r * r
    ps = S[0]
    for c in S[1:]:
        ps = fma_exact(ps, z, c)
    sr = fma_exact(r * z, ps, r)
    pc = Cc[0]
    for c in Cc[1:]:
        pc = fma_exact(pc, z, c)
    hz = 0.5 * z
    w = 1.0 - hz
    cr = w + (((1.0 - w) - hz) + fma_exact(z * z, pc, 0.0))
    q = int(k) & 3
    s0, c0 = (cr, sr) if q & 1 else (sr, cr)
    sv = -s0 if q & 2 else s0
    return (x if x == 0 else sv), (-c0 if (q + 1) & 2 else c0)


# ---------------------------------------------------------------------------------------------- log6
def log6_thresholds(dtype):
    """(small, beta series threshold, near-pi margin) of tsidb_common.hpp's log6 in that type"""
    return (1e-8, 1e-4, 1e-6) if np.dtype(dtype) == np.float64 else (1e-4, 1e-2, 1e-3)


def log6_restated(R, p, dtype):
    """log6 of tsidb_common.hpp, statement for statement, in numpy scalars of dtype (no contraction)"""
    T = np.dtype(dtype).type
    R = [T(v) for v in np.asarray(R).reshape(9)]
    p = [T(v) for v in np.asarray(p).reshape(3)]
    f64 = np.dtype(dtype) == np.float64
    PI = T(3.14159265358979323846)
    tr = R[0] + R[4] + R[8]
    ct = T(0.5) * (tr - T(1))
    ct = T(1) if ct > 1 else (T(-1) if ct < -1 else ct)
    th = np.arccos(ct)
    sth, cth = np.sin(th), np.cos(th)
    w = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    small = T(1e-8) if f64 else T(1e-4)
    if th < small:
        k = T(0.5) * (T(1) + th * th / T(6))
    elif th > PI - T(1e-6) * T(1 if f64 else 1000):
        for i in range(3):
            d = (R[4 * i] - ct) / (T(1) - ct)
            ax = np.sqrt(d if d > 0 else T(0))
            if w[i] < 0:
                ax = -ax
            w[i] = ax * th
        k = T(0)
    else:
        k = T(0.5) * th / sth
    if k != 0:
        w = [w[0] * k, w[1] * k, w[2] * k]
    th2 = th * th
    if th < T(1e-4) * T(1 if f64 else 100):
        beta = T(1.0 / 12) + th2 / T(720)
    else:
        beta = (T(1) - th * sth / (T(2) * (T(1) - cth))) / th2
    cr = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    wxp = cr(w, p)
    wxwxp = cr(w, wxp)
    return np.array([p[i] - T(0.5) * wxp[i] + beta * wxwxp[i] for i in range(3)] + w, dtype=dtype), float(beta)


def log6_mp(R, p, dtype):
    """the header's formulas and branches in mpmath on the exact input bits (thresholds as the type rounds them)"""
    T = np.dtype(dtype).type
    f64 = np.dtype(dtype) == np.float64
    R = [to_mp(v) for v in np.asarray(R, dtype=dtype).reshape(9)]
    p = [to_mp(v) for v in np.asarray(p, dtype=dtype).reshape(3)]
    PI = to_mp(T(3.14159265358979323846))
    ct = (R[0] + R[4] + R[8] - 1) / 2
    ct = mpf(1) if ct > 1 else (mpf(-1) if ct < -1 else ct)
    th = mpmath.acos(ct)
    sth, cth = mpmath.sin(th), mpmath.cos(th)
    w = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    small = to_mp(T(1e-8) if f64 else T(1e-4))
    margin = to_mp(T(1e-6) * T(1 if f64 else 1000))
    if th < small:
        k = (1 + th * th / 6) / 2
    elif th > PI - margin:
        for i in range(3):
            d = (R[4 * i] - ct) / (1 - ct)
            ax = mpmath.sqrt(d if d > 0 else 0)
            if w[i] < 0:
                ax = -ax
            w[i] = ax * th
        k = mpf(0)
    else:
        k = th / sth / 2
    if k != 0:
        w = [x * k for x in w]
    if th < to_mp(T(1e-4) * T(1 if f64 else 100)):
        beta = mpf(1) / 12 + th * th / 720
    else:
        beta = (1 - th * sth / (2 * (1 - cth))) / (th * th)
    cr = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    wxp = cr(w, p)
    wxwxp = cr(w, wxp)
    return [p[i] - wxp[i] / 2 + beta * wxwxp[i] for i in range(3)] + w, th


def log6_error_bound(th, dtype):
    """Ceiling, from the conditioning of the header's formulas, on the error of a same-precision evaluation of log6 at the
    rotation angle th (mpf, as log6_mp returns it), relative to the output's scale max(|p|, |out|); computed in mpmath.
      cosine       ct = (tr - 1) / 2 carries 3 roundings of numbers <= 3: |d ct| <= 2 eps
      angle        th = acos(ct): |d th| <= 2 eps / sin th
      w            k = th / (2 sin th) moves by |1 / th - cot th| |d th| relatively (2/3 eps as th -> 0, 2 eps / (pi - th)^2 next
                   to pi); R[7] - R[5] etc. are differences of entries whose symmetric part is (1 - cos th) a_i a_j against
                   a difference of 2 sin th a_k: eps tan(th / 2) relatively
      linear part  -w x p / 2 + beta w x (w x p): w's error times at most (1/2 + 2 beta |w|) |p| < 2 |p|; beta's own error is
                   3 eps / th^2 on a term of size th^2 |p| (1 - cos th is exact for th = acos(ct): Sterbenz), plain roundings
    -> 2 eps (8 + 2 |1 / th - cot th| / sin th + tan(th / 2)) below the near-pi branch.
    In the near-pi branch (th > pi - margin) the axis is ax_i = sqrt((R_ii - ct) / (1 - ct)): an argument off by 2 eps moves a
    component that should be 0 to sqrt(2 eps), and th = acos(ct) is itself off by at most sqrt(4 eps) at ct = -1 + O(eps):
    -> 2 (2 sqrt(2 eps) + 8 eps)."""
    T = np.dtype(dtype).type
    eps = mpf(eps_of(dtype))
    margin = to_mp(T(1e-6) * T(1 if np.dtype(dtype) == np.float64 else 1000))
    if th > to_mp(T(3.14159265358979323846)) - margin:
        return float(2 * (2 * mpmath.sqrt(2 * eps) + 8 * eps))
    if th == 0:
        return float(2 * eps * (8 + mpf(2) / 3))
    return float(2 * eps * (8 + 2 * abs(1 / th - mpmath.cot(th)) / mpmath.sin(th) + mpmath.tan(th / 2)))


def rot_mp(axis, angle):
    """Rodrigues rotation in mpmath (axis normalised there), as a 3x3 list of mpf"""
    a = [mpf(float(v)) for v in axis]
    nrm = mpmath.sqrt(sum(v * v for v in a))
    a = [v / nrm for v in a]
    th = mpf(angle) if not isinstance(angle, mpmath.mpf) else angle
    c, s = mpmath.cos(th), mpmath.sin(th)
    K = [[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]
    return [[(c if i == j else 0) + s * K[i][j] + (1 - c) * a[i] * a[j] for j in range(3)] for i in range(3)]


LOG6_AXES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1), (0, 3, 4), (5, 0, -12), (2, 1, 0)]


def log6_cases(dtype, seed=0):
    """(bucket name, R (9,), p (3,)) over the issue's angle list x axes x translations, rounded to dtype; the exact-pi cases last"""
    rng = np.random.default_rng(seed)
    small, bth, margin = log6_thresholds(dtype)
    pi = mpmath.pi
    angles = [("0", mpf(0)), ("1e-12", mpf("1e-12")), ("1e-9", mpf("1e-9"))]
    for nm, t in (("small", mpf(small)), ("beta", mpf(bth))):
        angles += [(f"0.99*{nm}", t * mpf("0.99")), (f"1.01*{nm}", t * mpf("1.01"))]
    angles += [("pi-1.01*margin", pi - mpf(margin) * mpf("1.01")), ("pi-0.99*margin", pi - mpf(margin) * mpf("0.99"))]
    angles += [(s, mpf(s)) for s in ("1e-6", "1e-3", "0.1", "1", "2", "3")]
    angles += [("pi-1e-2", pi - mpf("1e-2")), ("pi-1e-5", pi - mpf("1e-5")), ("pi-1e-9", pi - mpf("1e-9"))]
    axes = LOG6_AXES + [tuple(rng.normal(size=3)) for _ in range(4)]
    ps = [np.zeros(3), np.array([0.0, 1.0, 0.0])] + [rng.normal(size=3) / np.sqrt(3) * s for s in (1e-3, 1.0, 10.0)]
    out = []
    for nm, th in angles:
        for ax in axes:
            Rm = rot_mp(ax, th)
            R = np.array([[float(Rm[i][j]) for j in range(3)] for i in range(3)]).astype(dtype).reshape(9)
            for p in ps:
                out.append((nm, R, p.astype(dtype)))
    for d in ((1, -1, -1), (-1, 1, -1), (-1, -1, 1)):
        for p in ps:
            out.append(("pi", np.diag(np.array(d, dtype=dtype)).reshape(9), p.astype(dtype)))
    return out


# ---------------------------------------------------------------------------------------------- factorisations, restated
def tick_chol_restated(A, dtype):
    """tick_chol: right-looking, rk = 1 / sqrt(akk), column scaled by rk, trailing update a[j] -= lik * L[j][k] (one FMA each
    in the device code; numpy rounds product and difference apart - inside the gate's factor).  Returns L (lower), rdv."""
    a = np.array(A, dtype=dtype)
    n = a.shape[0]
    one = a.dtype.type(1)
    rdv = np.zeros(n, dtype=dtype)
    for k in range(n):
        akk = a[k, k]
        rk = one / np.sqrt(akk)
        rdv[k] = rk
        a[k:, k] = a[k:, k] * rk
        for j in range(k + 1, n):
            a[:, j] = a[:, j] - a[:, k] * a[j, k]
    return np.tril(a), rdv


def chol26_restated(A, anc, dtype, dense=False):
    """chol26_solve / chol26_factor: leaves first (k = NV-1 .. 0), A = U U^T, U upper; only ancestor pairs are updated"""
    a = np.array(A, dtype=dtype)
    n = a.shape[0]
    one = a.dtype.type(1)
    rd = np.zeros(n, dtype=dtype)
    for k in range(n - 1, -1, -1):
        akk = a[k, k]
        rk = one / np.sqrt(akk)
        rd[k] = rk
        col = a[:, k] * rk
        col[k] = akk * rk
        col[k + 1:] = 0
        a[:, k] = col
        for j in range(k):
            if dense or (anc[k] >> j) & 1:
                a[:, j] = a[:, j] - col * col[j]
    return a, rd


def chol26_subst_restated(U, rd, rhs):
    """U y = rhs (descendants first), U^T x = y (ancestors first), as chol26_subst orders them"""
    n = U.shape[0]
    acc = np.array(rhs, dtype=U.dtype)
    y = np.zeros(n, dtype=U.dtype)
    for k in range(n - 1, -1, -1):
        y[k] = acc[k] * rd[k]
        acc = acc - U[:, k] * y[k]
    acc = y.copy()
    x = np.zeros(n, dtype=U.dtype)
    for i in range(n):
        x[i] = acc[i] * rd[i]
        acc = acc - U[i, :] * x[i]
    return x


def chol26_rank1_restated(U, rd, x, sigma, chain):
    """chol26_rank1's recurrences (tsidb_sim.hpp); returns (U', rd', ok)"""
    U, rd, xv = U.copy(), rd.copy(), np.array(x, dtype=U.dtype)
    T = U.dtype.type
    thr = T(1e-10) if U.dtype == np.float64 else T(1e-5)
    n = U.shape[0]
    sg = T(sigma)
    for k in range(n - 1, -1, -1):
        if not (chain >> k) & 1:
            continue
        s = xv[k] * rd[k]
        q = T(1) + sg * s * s
        if not q > thr:
            return U, rd, False
        ic = T(1) / np.sqrt(q)
        c = q * ic
        un = (U[:, k] + sg * s * xv) * ic
        xv = c * xv - s * un
        xv[k] = 0
        U[:, k] = un
        rd[k] = rd[k] * ic
    return U, rd, True


def pattern_mask(anc, n):
    """boolean (n, n): True where U[i][k] may be non-zero (i == k or i an ancestor of k)"""
    P = np.eye(n, dtype=bool)
    for k in range(n):
        for i in range(k):
            if (anc[k] >> i) & 1:
                P[i, k] = True
    return P


def tree_sparse_spd(rng, anc, n, count):
    """random SPD matrices with the tree's sparsity: a diagonal plus sum of x x^T, x supported on root paths"""
    out = np.zeros((count, n, n))
    for c in range(count):
        A = np.diag(rng.uniform(0.5, 2.0, n))
        for _ in range(2 * n):
            k = int(rng.integers(n))
            x = np.zeros(n)
            for i in range(n):
                if i == k or (anc[k] >> i) & 1:
                    x[i] = rng.normal()
            A += rng.uniform(0.1, 1.0) * np.outer(x, x)
        out[c] = A
    return out


def robot_mass_matrices(robot, count, seed=3):
    """the joint-space inertia M of oracle.terms at random poses of the robot (TSID dof order), as (count, NV, NV)"""
    from oracle.oracle import Oracle, build
    from tsid_control_amd.model import ModelBlob
    build()
    blob = ModelBlob(ROOT / "tsid_control_amd" / "assets" / ROBOTS[robot][1])
    orc = Oracle(blob.raw)
    nq, nv = int(blob["model_dims"][1]), int(blob["model_dims"][2])
    rng = np.random.default_rng(seed)
    Ms = []
    for _ in range(count):
        q = blob.q0
        quat = rng.normal(size=4)
        q[3:7] = quat / np.linalg.norm(quat)
        q[7:] += rng.uniform(-0.8, 0.8, nq - 7)
        Ms.append(np.asarray(orc.terms(q, np.zeros(nv))["M"]).reshape(nv, nv).copy())
    return np.stack(Ms), blob


def sim_order(M, blob):
    """M of the TSID order permuted into the sim's dof order (mj_sim2tsid), whose tree MJ_DOFANC describes"""
    s2t = np.asarray(blob["mj_sim2tsid"]).astype(int)
    perm = np.concatenate([np.arange(6), 6 + s2t])
    return M[..., perm[:, None], perm[None, :]]
