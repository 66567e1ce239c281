"""Unit layer, device scalar maths and small geometry alone (through tests/unit/tsidb_unit.hip): rsqrt_t / rcp_t, the
hand-written double sincos_t, log6 with its three branches and four thresholds, quat_to_R, mat_to_quat, make_frame,
origin_tri_closest, terrain_h.  Truths are mpmath at 50 digits or longdouble; gates follow unit_testlib's rule.

Measured on the MI355X: profiles/unit_primitives.txt.  log6's beta just above its series threshold: test_log6 and DESIGN.md
section 7; origin_tri_closest on thin triangles: test_origin_tri_closest."""
import mpmath
import numpy as np
import pytest
import torch

import unit_testlib as U
from unit_testlib import mpf

pytestmark = pytest.mark.gpu
DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def h():
    return U.harness("v1")


def call_map(h, name, x, outs, n):
    """element-wise entry point: x host array, outs = per-output elements per n"""
    xd = dev(x)
    o = [torch.empty(n * k, dtype=xd.dtype, device="cuda") for k in outs]
    h.call(name, xd, *o, n=n)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in o]


# ------------------------------------------------------------------------------------------------ rsqrt_t, rcp_t
def positive_inputs(rng):
    x = [10.0 ** rng.uniform(-290, 290, 4000), 2.0 ** np.arange(-960, 961, 7.0), 4.0 ** np.arange(-480, 481, 3.0)]
    one = [1.0]
    for _ in range(64):
        one.append(np.nextafter(one[-1], 2.0))
    lo = [1.0]
    for _ in range(64):
        lo.append(np.nextafter(lo[-1], 0.0))
    return np.concatenate(x + [np.array(one), np.array(lo)])


def test_rsqrt_rcp_f64(h):
    """4 ulp against mpmath on the domain the header names (positive normal x).  rcp_t(double) has no call site in the
    kernels today, so there is no negative argument to test: its domain here is the header's."""
    x = positive_inputs(np.random.default_rng(20))
    n = len(x)
    for name, f in (("rsqrt_f64", lambda v: 1 / mpmath.sqrt(v)), ("rcp_f64", lambda v: 1 / v)):
        y, = call_map(h, name, x, [1], n)
        truth = [f(U.to_mp(v)) for v in x]
        err = U.mp_err(y, truth) / U.ulp([float(t) for t in truth])
        assert np.isfinite(y).all()
        U.report(name, n=n, worst_ulp=float(err.max()), gate_ulp=4)
        assert err.max() <= 4, (name, x[err.argmax()])


def test_rsqrt_rcp_f32_match_torch(h):
    """the float overloads are plain IEEE expressions: bit-compared with torch's on the device"""
    rng = np.random.default_rng(21)
    x = np.concatenate([10.0 ** rng.uniform(-37, 38, 4000), 2.0 ** np.arange(-120.0, 121.0), [1.0, 3.0, 0.1]]).astype(np.float32)
    xd = dev(x)
    for name, ref in (("rsqrt_f32", 1 / torch.sqrt(xd)), ("rcp_f32", 1 / xd)):
        y = torch.empty_like(xd)
        h.call(name, xd, y, n=len(x))
        torch.cuda.synchronize()
        bad = int((bits(y.cpu().numpy()) != bits(ref.cpu().numpy())).sum())
        U.report(name, n=len(x), bit_mismatches=bad)
        assert bad == 0


# ------------------------------------------------------------------------------------------------ sincos_t(double)
def sincos_inputs(rng):
    pts = []
    half_pi = mpmath.pi / 2
    for k in range(-640, 641):
        for c in (mpf(k), mpf(k) + mpf("0.5")):   # multiples of pi/2, and the points where rint flips
            x0 = float(c * half_pi)
            lo = hi = x0
            pts.append(x0)
            for _ in range(2):
                lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
                pts += [lo, hi]
    pts += [0.0, -0.0, 1e-300, -1e-300, 5e-324, 2.5e-310, 1e3, -1e3]
    return np.concatenate([np.array(pts), rng.uniform(-1e3, 1e3, 100000)])


def sincos_gate(x, s_true, c_true):
    """per output: 4 ulp of the true value where |r| >= 2^-26 (r = x - k pi/2 in mpmath); below that the component that is
    ~ r gets the absolute 2^-76 the two-constant reduction implies (640 |pi/2 - hi - lo| + 2^-53 |r| < 2^-77; the first FMA
    is exact), the component that is ~ 1 keeps 4 ulp"""
    m = U.to_mp(x)
    k = mpmath.nint(m * 2 / mpmath.pi)
    r = abs(m - k * mpmath.pi / 2)
    out = []
    for t in (s_true, c_true):
        if r < mpf(2) ** -26 and abs(t) < 0.5:
            out.append(2.0 ** -76)
        else:
            out.append(4 * float(U.ulp(float(t))))
    return out


def test_sincos_f64(h):
    x = sincos_inputs(np.random.default_rng(22))
    n = len(x)
    s, c = call_map(h, "sincos_f64", x, [1, 1], n)
    worst = {"ulp": 0.0, "abs_small_r": 0.0}
    xl = x.astype(np.longdouble)
    r_approx = np.abs(xl - np.rint(xl * (2 / np.pi)) * (np.longdouble(np.pi) / 2))   # only to pick the gate's branch early
    for i in range(n):
        ctv, st = mpmath.cos_sin(U.to_mp(x[i]))
        if r_approx[i] > 2.0 ** -20:
            gs, gc = 4 * float(U.ulp(float(st))), 4 * float(U.ulp(float(ctv)))
        else:
            gs, gc = sincos_gate(x[i], st, ctv)
        for got, t, g in ((s[i], st, gs), (c[i], ctv, gc)):
            e = float(abs(U.to_mp(got) - t))
            if g == 2.0 ** -76:
                worst["abs_small_r"] = max(worst["abs_small_r"], e)
            else:
                worst["ulp"] = max(worst["ulp"], e / (g / 4))
            assert e <= g, (x[i], got, float(t), e, g)
    U.report("sincos_f64", n=n, worst_ulp=worst["ulp"], gate_ulp=4, worst_abs_small_r=worst["abs_small_r"], gate_abs=2.0 ** -76)
    # odd / even symmetry, bit for bit, and the signed zeros
    sm, cm = call_map(h, "sincos_f64", -x, [1, 1], n)
    assert np.array_equal(bits(sm), bits(-s)) and np.array_equal(bits(cm), bits(c))
    z = np.array([0.0, -0.0])
    sz, cz = call_map(h, "sincos_f64", z, [1, 1], 2)
    assert np.array_equal(bits(sz), bits(z)) and np.array_equal(cz, [1.0, 1.0])


# ------------------------------------------------------------------------------------------------ log6
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_log6(h, t):
    """Per angle bucket: device error against the header's formulas in mpmath on the exact input bits, normalised by the
    output's scale max(|p|, |truth|), gated at 8 x the same-precision numpy restatement's own error in that bucket + 8 ulp.

    The bucket just above the beta threshold (1.01 x threshold) is where (1 - th sin th / (2 (1 - cos th))) / th^2 cancels
    when it is evaluated on an angle (numpy: beta = 0.596 in float64 at 1.01e-4, 3.35 in float32 at 1.01e-2, instead of
    0.0833: tests/test_unit_reference.py prints both).  Inside log6 th = acos(ct), cos(th) rounds back to ct and 1 - cos th is
    exact: measured on the MI355X the bucket's error is 1.6e-16 (float64) and 1.3e-7 (float32) of the output's scale, the
    same as the restatement's (profiles/unit_primitives.txt; test_log6_beta_cancellation_measured prints beta itself)."""
    _, npdt = DT[t]
    cases = U.log6_cases(npdt)
    n = len(cases)
    R = np.stack([c[1] for c in cases])
    p = np.stack([c[2] for c in cases])
    Rd, pd = dev(R), dev(p)
    out = torch.empty(n * 6, dtype=Rd.dtype, device="cuda")
    h.call(f"log6_{t}", Rd, pd, out, n=n)
    torch.cuda.synchronize()
    o = out.cpu().numpy().reshape(n, 6)
    assert np.isfinite(o).all()
    eps = U.eps_of(npdt)
    buckets = {}
    for i, (name, Ri, pi_) in enumerate(cases):
        truth, _th = U.log6_mp(Ri, pi_, npdt)
        ref, _ = U.log6_restated(Ri, pi_, npdt)
        scale = max(float(np.abs(pi_).max()), max(float(abs(v)) for v in truth), 1e-300)
        b = buckets.setdefault(name, dict(dev=0.0, ref=0.0, n=0))
        b["dev"] = max(b["dev"], float(U.mp_err(o[i], truth).max()) / scale)
        ref_err = float(U.mp_err(ref, truth).max()) / scale
        # (the gate's ceiling: the restatement is inside the formulas' conditioning here too, as tests/test_unit_reference.py
        #  asserts it where no GPU is needed - a broken restatement cannot widen a bucket's gate)
        assert ref_err <= U.log6_error_bound(_th, npdt), (name, ref_err)
        b["ref"] = max(b["ref"], ref_err)
        b["n"] += 1
    failed = []
    for name, b in buckets.items():
        gate = 8 * b["ref"] + 8 * eps
        U.report(f"log6_{t}[{name}]", n=b["n"], dev_rel_err=b["dev"], restated_rel_err=b["ref"], gate=gate)
        if not b["dev"] <= gate:
            failed.append((name, b["dev"], gate))
    assert not failed, failed


def test_log6_beta_cancellation_measured(h):
    """the device's own beta just above the series threshold, recovered from out = p + beta w x (w x p) with w _|_ p"""
    for t, th in (("f64", 1.01e-4), ("f32", 1.01e-2)):
        _, npdt = DT[t]
        Rm = U.rot_mp((0, 0, 1), mpf(th))
        R = np.array([[float(Rm[i][j]) for j in range(3)] for i in range(3)]).astype(npdt).reshape(1, 9)
        p = np.array([[1.0, 0.0, 0.0]], dtype=npdt)
        out = torch.empty(6, dtype=DT[t][0], device="cuda")
        h.call(f"log6_{t}", dev(R), dev(p), out, n=1)
        torch.cuda.synchronize()
        o = out.cpu().numpy().astype(np.float64)
        w = o[5]
        beta_dev = (1.0 - o[0]) / (w * w)        # w x (w x p) = -w^2 p for p = e_x, w along z
        _, beta_ref = U.log6_restated(R[0], p[0], npdt)
        truth, _ = U.log6_mp(R[0], p[0], npdt)
        _, thm = U.log6_mp(R[0], p[0], npdt)
        beta_true = float((1 - thm * mpmath.sin(thm) / (2 * (1 - mpmath.cos(thm)))) / (thm * thm))
        # 8 x the restated beta's own error, + 8 eps / w^2: what recovering beta from 1 - beta w^2 costs
        gate = 8 * abs(beta_ref - beta_true) + 8 * U.eps_of(npdt) / (w * w)
        U.report(f"log6_beta_{t}", theta=th, beta_device=float(beta_dev), beta_restated=beta_ref, beta_true=beta_true,
                 err=float(abs(beta_dev - beta_true)), gate=float(gate), linear_err_per_unit_p=float(abs(U.to_mp(o[0]) - truth[0])))
        assert abs(beta_dev - beta_true) <= gate     # (the bare formula's 0.596 / 3.35 would be far outside)


# ------------------------------------------------------------------------------------------------ quat_to_R, mat_to_quat
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_quat_to_R(h, t):
    _, npdt = DT[t]
    rng = np.random.default_rng(23)
    n = 512
    q = rng.normal(size=(n, 4))
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    q[:4] = np.eye(4) * 7.0
    q = q.astype(npdt)
    R, = call_map(h, f"quat_to_R_{t}", q, [9], n)
    R = R.reshape(n, 3, 3).astype(np.longdouble)
    ql = q.astype(np.longdouble)
    ql = ql / np.sqrt((ql * ql).sum(axis=1, keepdims=True))
    x, y, z, w = ql.T
    ref = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                    2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)
    # normalisation (sum of 4 squares, sqrt, divide, 4 products: <= 6 roundings on every component), then <= 5 roundings on an
    # entry whose terms are bounded by 2: 16 eps absolute covers it; orthonormality inherits twice that
    gate = 16 * U.eps_of(npdt)
    err = float(np.abs(R - ref).max())
    orth = float(np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max())
    U.report(f"quat_to_R_{t}", n=n, worst_abs_err=err, gate=gate, worst_orthonormality=orth, gate_orth=2 * gate)
    assert err <= gate and orth <= 2 * gate


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_mat_to_quat(h, t):
    """all four branches, pi about each axis, trace within 1e-12 of 0; agreement with the longdouble quaternion up to sign"""
    _, npdt = DT[t]
    rng = np.random.default_rng(24)
    qs = [rng.normal(size=4) for _ in range(256)]
    qs += [np.array(v, dtype=float) for v in ((0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 0, 0))]   # wxyz: pi about x, y, z; identity
    for ax in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3)):
        for d in (-1e-12, 0.0, 1e-12):        # trace = 1 + 2 cos(th) = d
            th = np.arccos((d - 1) / 2)
            a = np.array(ax, dtype=float) / np.linalg.norm(ax)
            qs.append(np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * a]))
    for i in range(3):                        # a dominant diagonal entry with a negative trace: branches 2, 3, 4
        v = np.array([0.05, 0.1, 0.1, 0.1]); v[1 + i] = 1.0
        qs.append(v)
    q = np.array(qs, dtype=np.longdouble)
    q /= np.sqrt((q * q).sum(axis=1, keepdims=True))
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).astype(npdt)
    n = len(R)
    tr = R[:, 0] + R[:, 4] + R[:, 8]
    br = np.where(tr > 0, 0, np.where((R[:, 0] > R[:, 4]) & (R[:, 0] > R[:, 8]), 1, np.where(R[:, 4] > R[:, 8], 2, 3)))
    assert set(br.tolist()) == {0, 1, 2, 3}
    got, = call_map(h, f"mat_to_quat_{t}", R, [4], n)
    got = got.reshape(n, 4).astype(np.longdouble)
    # R is the rounded image of q (entries off by eps/2): the branch's square root argument is >= 1, so the quaternion moves by
    # a few eps; the routine adds 3 sums, sqrt, divide, normalisation.  32 eps on a unit quaternion.
    gate = 32 * U.eps_of(npdt)
    sign = np.sign((got * q).sum(axis=1, keepdims=True))
    err = float(np.abs(got - sign * q).max())
    nrm = float(np.abs(np.sqrt((got * got).sum(axis=1)) - 1).max())
    U.report(f"mat_to_quat_{t}", n=n, worst_abs_err=err, gate=gate, worst_norm_err=nrm, gate_norm=4 * U.eps_of(npdt))
    assert err <= gate and nrm <= 4 * U.eps_of(npdt)


# ------------------------------------------------------------------------------------------------ make_frame
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_make_frame(h, t):
    _, npdt = DT[t]
    rng = np.random.default_rng(25)
    ns = [v for e in np.eye(3) for v in (e, -e)]
    half = npdt(0.5)
    for ny in (np.nextafter(half, npdt(0)), half, np.nextafter(half, npdt(1))):
        for sg in (1, -1):
            ny64 = float(ny)
            rest = np.sqrt(1 - ny64 * ny64)
            ns.append(np.array([rest * 0.6, sg * ny64, rest * 0.8]))
    r = rng.normal(size=(256, 3))
    ns += list(r / np.linalg.norm(r, axis=1, keepdims=True))
    nrm = np.array(ns).astype(npdt)          # (|n_y| is kept exactly as built; the other two carry the rounding)
    n = len(nrm)
    t1, t2 = call_map(h, f"make_frame_{t}", nrm, [3, 3], n)
    N, T1, T2 = nrm.astype(np.longdouble), t1.reshape(n, 3).astype(np.longdouble), t2.reshape(n, 3).astype(np.longdouble)
    assert np.isfinite(t1).all() and np.isfinite(t2).all()
    # which axis t1 is built from: y unless |n_y| >= 0.5 - checked through the sign pattern of the exact construction
    seed = np.where(np.abs(nrm[:, 1:2]) < half, np.array([[0, 1, 0]]), np.array([[0, 0, 1]])).astype(np.longdouble)
    ref = seed - (N * seed).sum(axis=1, keepdims=True) * N
    ref /= np.sqrt((ref * ref).sum(axis=1, keepdims=True))
    e = 8 * U.eps_of(npdt)
    worst = dict(t1=float(np.abs(T1 - ref).max()), unit=float(np.abs((T1 * T1).sum(axis=1) - 1).max()),
                 n_dot_t1=float(np.abs((N * T1).sum(axis=1)).max()), t2=float(np.abs(T2 - np.cross(N, T1)).max()))
    U.report(f"make_frame_{t}", n=n, gate=e, **worst)
    # n itself is a rounded unit vector (|n| = 1 +- eps): n . t1 and the lengths inherit that, all within the 8 ulp
    assert all(v <= e for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------ origin_tri_closest
def tri_truth(tri):
    """min over the vertices, the edge projections and the face projection, in longdouble"""
    a, b, c = (tri[i].astype(np.longdouble) for i in range(3))
    best = min(float(v @ v) for v in (a, b, c))
    for p, q in ((a, b), (a, c), (b, c)):
        d = q - p
        dd = d @ d
        if dd > 0:
            s = -(p @ d) / dd
            if 0 <= s <= 1:
                v = p + s * d
                best = min(best, float(v @ v))
    nrm = np.cross(b - a, c - a)
    nn = nrm @ nrm
    if nn > 0:
        v = nrm * ((a @ nrm) / nn)           # projection of the origin onto the plane
        # inside test by barycentric signs
        s = [np.cross(q - p, v - p) @ nrm for p, q in ((a, b), (b, c), (c, a))]
        if all(x >= 0 for x in s):
            best = min(best, float(v @ v))
    return best


def tri_cases(rng, eps):
    out = []
    base = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    # the seven Voronoi regions and their borders: the origin placed relative to a fixed triangle (shift = -point)
    pts = [(-1, -1), (2, -1), (-1, 2), (0.5, -1), (-1, 0.5), (1, 1), (0.25, 0.25),           # A, B, C, AB, AC, BC, face
           (0, -1), (-1, 0), (1, -1), (2, 0), (0, 2), (-1, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (0, 0), (1, 0), (0, 1)]
    for (u, v) in pts:
        for hgt in (0.0, 0.3):
            out.append(base - np.array([u, v, hgt]))
    for _ in range(200):
        out.append(rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-2, 1))
    for _ in range(64):                                                                    # nearly degenerate: slivers
        a, d = rng.normal(size=3), rng.normal(size=3)
        out.append(np.stack([a, a + d, a + 2 * d + rng.normal(size=3) * 10.0 ** rng.uniform(-14, -6)]))
    for _ in range(96):                                                                    # slivers at the type's own resolution
        a, d = rng.normal(size=3), rng.normal(size=3)                                      # (0.1 .. 1e4 ulp off the line) and up to
        if rng.uniform() < 0.5:                                                            # thin but sound triangles; half of them
            a = 0.2 * a - d                                                                # with the origin over the middle
        out.append(np.stack([a, a + d, a + 2 * d + rng.normal(size=3) * (eps * 10.0 ** rng.uniform(-1, 4) if rng.uniform() < 0.5 else 10.0 ** rng.uniform(-7, 0))]))
    # exactly collinear, the origin's projection inside / on / outside the segment, and ON the line (va + vb + vc = 0)
    for s0 in (-1.0, -0.25, 0.0, 0.5, 1.0, 2.5):
        for off in (0.0, 0.5):
            a = np.array([-1.0 - s0, off, 0.0])
            out.append(np.stack([a, a + [1, 0, 0], a + [2, 0, 0]]))
            out.append(np.stack([a, a + [2, 0, 0], a + [1, 0, 0]]))
            out.append(np.stack([a + [1, 0, 0], a, a + [2, 0, 0]]))
    out.append(np.zeros((3, 3)))                                                            # a point at the origin
    out.append(np.ones((3, 3)))                                                             # a point elsewhere
    return np.array(out)


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_origin_tri_closest(h, t):
    """Distance^2 within 64 eps x the largest squared vertex norm of the longdouble truth, and finite, in every case.
    The slivers are what found the routine's thin-triangle fault: a, a + d, a + 2 d + delta with delta at the type's resolution
    rounds to a collinear or one-ulp-off triangle, va / vb / vc = d1 d4 - d3 d2 etc. are then rounding noise of either sign
    (-ffp-contract=on fuses each into an FMA, so not even an exactly collinear triangle gives exact zeros), no region test
    fired and the face formula divided by that noise: distance^2 off by 0.04 .. 15 in float32 on the MI355X, 5.9e5 x this
    gate, everything finite.  origin_tri_closest now answers thin triangles with the least of its edge points and the face
    point; numbers after the fix: profiles/unit_primitives.txt."""
    _, npdt = DT[t]
    tri = tri_cases(np.random.default_rng(26), U.eps_of(npdt)).astype(npdt)
    n = len(tri)
    d2, q = call_map(h, f"tri_closest_{t}", tri.reshape(n, 9), [1, 3], n)
    q = q.reshape(n, 3)
    finite = np.isfinite(d2) & np.isfinite(q).all(axis=1)
    truth = np.array([tri_truth(x) for x in tri])
    scale = (tri.astype(np.float64) ** 2).sum(axis=2).max(axis=1)
    gate = 64 * U.eps_of(npdt) * scale
    err = np.abs(d2.astype(np.float64) - truth)
    ok = finite & (err <= gate)
    U.report(f"origin_tri_closest_{t}", n=n, non_finite=int((~finite).sum()), worst_err_over_gate=float(np.nanmax(np.where(finite, err, 0) / np.maximum(gate, 1e-300))))
    assert finite.all(), tri[~finite][:4]
    assert ok.all(), (tri[~ok][:4], err[~ok][:4], gate[~ok][:4])
    assert np.allclose((q.astype(np.float64) ** 2).sum(axis=1), d2, rtol=8 * U.eps_of(npdt), atol=0)


# ------------------------------------------------------------------------------------------------ terrain_h
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_terrain_h(h, t):
    """negative u, u exactly on cell borders, |(u - phase) inv_len| up to 2^30; against numpy's floor mod 16 in the same type"""
    _, npdt = DT[t]
    rng = np.random.default_rng(27)
    terr = np.concatenate([[1.0, 0.0, 0.25, 4.0], np.arange(16) * 0.01 + 0.5]).astype(npdt)   # dir = x, phase 0.25, cells of 0.25
    cells = np.concatenate([np.arange(-40, 41), rng.integers(-2 ** 30, 2 ** 30, 200), [2 ** 30 - 1, -2 ** 30]])
    X = np.concatenate([0.25 + cells * 0.25,                                   # exactly on the borders
                        0.25 + rng.uniform(-40, 40, 500) * 0.25,               # inside cells, both signs
                        0.25 + rng.integers(-2 ** 30, 2 ** 30, 200) * 0.25 + 0.125])
    xy = np.stack([X, rng.normal(size=len(X))], axis=1).astype(npdt)
    n = len(xy)
    td, xd = dev(terr), dev(xy)
    out = torch.empty(n, dtype=DT[t][0], device="cuda")
    h.call(f"terrain_h_{t}", td, xd, out, n=n)
    torch.cuda.synchronize()
    u = terr[0] * xy[:, 0] + terr[1] * xy[:, 1]
    cell = np.floor((u - terr[2]) * terr[3]).astype(np.int64) % 16
    bad = int((bits(out.cpu().numpy()) != bits(terr[4 + cell])).sum())
    U.report(f"terrain_h_{t}", n=n, mismatches=bad)
    assert bad == 0
