"""The unit layer's references, checked where no GPU is needed: the same-precision numpy restatements of unit_testlib against
the mpmath truths on the GPU tests' own case lists (their errors printed: these are what the device gates are 8 x of), the
harness libraries' exports, and tsidbu_dims against tsidb_dims and the topology headers."""
import ctypes as C
import subprocess

import mpmath
import numpy as np
import pytest

import unit_testlib as U
from unit_testlib import mpf


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if " T " in line)


@pytest.mark.parametrize("robot", ["v1", "v0"])
def test_harness_exports_and_dims(robot):
    lib, _, _, product = U.ROBOTS[robot]
    assert exported(U.UNIT / lib) == U.EXPORTS          # exactly the tsidbu_* entry points, nothing of the product's
    L = U.harness(robot).L                              # (torch's HIP runtime first: see tsid_control_amd/_lib.py)
    d4, anc, m1, m2 = (C.c_int * 4)(), (C.c_uint * 32)(), (C.c_uint * 64)(), (C.c_uint * 64)()
    assert L.tsidbu_dims(d4, anc, m1, m2) == 0
    assert L.tsidbu_dims(None, anc, m1, m2) != 0
    from tsid_control_amd import _lib
    P = _lib.load(U.ROOT / "tsid_control_amd" / product)       # both libraries in one process
    nv = _lib.dims9(P)[2]
    want = U.header_dofanc(robot)
    assert d4[0] == nv == len(want) and d4[3] == 27
    assert [int(x) for x in anc][:nv] == want and not any(int(x) for x in anc[nv:])
    masks = [int(x) for x in m1][:d4[1]]
    assert all(m >> 32 == 0 for m in masks) and masks[-nv:] == [want[k] & ((1 << k) - 1) for k in range(nv)]
    for k in (0, 7, 8, nv - 2):                                 # tick_chol's masks are among the compiled ones
        assert ((1 << nv) - 1) & ~((2 << k) - 1) in masks
    # launch nothing and return non-zero for n <= 0 or a null pointer (no device is touched: the checks come first)
    L.tsidbu_wave_sum_f64.restype = C.c_int
    assert L.tsidbu_wave_sum_f64(None, None, C.c_int(4), None) != 0
    assert L.tsidbu_wave_sum_f64(C.c_void_p(8), C.c_void_p(8), C.c_int(0), None) != 0


def test_loader_refuses_mismatched_buffers():
    import torch
    h = U.Harness.__new__(U.Harness)
    h.NV = 26
    with pytest.raises(ValueError):
        h._ptr(torch.zeros(64), "float32", 64, "cpu tensor")
    with pytest.raises(ValueError, match="CUDA tensor"):
        h.call("wave_sum_f64", None, None, n=1)               # the right number of arguments: refused for the buffer itself
    with pytest.raises(ValueError, match="arguments"):
        h.call("wave_sum_f64", None, n=1)
    assert h._count("NV2", 0, 3) == 3 * 676 and h._count(64, 0, 2) == 128 and h._count(0, 20, 5) == 20


def test_fma_exact_and_ulp_helpers():
    assert U.fma_exact(3.0, 5.0, 7.0) == 22.0
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30
    assert U.fma_exact(a, b, -1.0) == -2.0 ** -60 and a * b - 1.0 == 0.0      # the product alone rounds to 1
    assert U.ulp(1.0) == 2.0 ** -52 and U.ulp(np.float32(1.0), np.float32) == 2.0 ** -23
    assert abs(float(U.gamma(31)) - 31 * 2.0 ** -53) < 1e-28


def test_sincos_restated_against_mpmath():
    from test_gpu_unit_math import sincos_gate, sincos_inputs
    x = sincos_inputs(np.random.default_rng(22))
    pick = np.concatenate([x[:12818:11], x[12810:12818], x[12818::400]])
    worst = 0.0
    for v in pick:
        s, c = U.sincos_restated(v)
        ct, st = mpmath.cos_sin(U.to_mp(v))
        gs, gc = sincos_gate(v, st, ct)
        worst = max(worst, float(abs(U.to_mp(s) - st)) / gs, float(abs(U.to_mp(c) - ct)) / gc)
        sm, cm = U.sincos_restated(-v)
        assert sm == -s and cm == c and np.signbit(sm) != np.signbit(s)
    print(f"UNIT sincos_restated n={len(pick)} worst_err_over_gate={worst:.3e}")
    assert worst <= 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_log6_restated_against_mpmath_and_logm(dtype):
    cases = U.log6_cases(dtype)
    buckets = {}
    for name, R, p in cases:
        truth, th = U.log6_mp(R, p, dtype)
        ref, _ = U.log6_restated(R, p, dtype)
        scale = max(float(np.abs(p).max()), max(float(abs(v)) for v in truth), 1e-300)
        err, bound = float(U.mp_err(ref, truth).max()) / scale, U.log6_error_bound(th, dtype)
        # every case of every bucket, the one above the beta threshold and the ones next to pi included: the restatement's
        # error is inside what the formulas' conditioning allows at that angle (unit_testlib.log6_error_bound).  The GPU
        # gates are 8 x these errors, so 8 x this bound is their ceiling
        assert err <= bound, (name, err, bound)
        b = buckets.setdefault(name, [0.0, 0.0])
        b[0], b[1] = max(b[0], err), max(b[1], bound)
    small, bth, margin = U.log6_thresholds(dtype)
    for name, (e, bd) in buckets.items():
        print(f"UNIT log6_restated_{np.dtype(dtype).name}[{name}] rel_err={e:.3e} conditioning_bound={bd:.3e}")
    # the cancellation itself, on the angle alone (through a rotation matrix acos returns an angle whose cosine is the rounded
    # input again, and 1 - cos loses nothing): beta = (1 - th sin th / (2 (1 - cos th))) / th^2 just above its threshold
    T = np.dtype(dtype).type
    th = T(1.01) * T(bth)
    beta = (T(1) - th * np.sin(th) / (T(2) * (T(1) - np.cos(th)))) / (th * th)
    print(f"UNIT log6_beta_formula_{np.dtype(dtype).name} theta={float(th):.3e} beta={float(beta):.4f} exact={1 / 12:.4f} "
          f"linear_err_per_unit_p={abs(float(beta) - 1 / 12) * float(th) ** 2:.3e}")
    assert np.isfinite(beta)
    # the header's formulas against the matrix logarithm of the 4x4 placement, away from pi and from the cancellation
    rng = np.random.default_rng(40)
    for _ in range(12):
        ax, th = rng.normal(size=3), rng.uniform(0.05, 2.8)
        Rm = U.rot_mp(ax, mpf(th))
        R = np.array([[float(Rm[i][j]) for j in range(3)] for i in range(3)])
        p = rng.normal(size=3)
        truth, _ = U.log6_mp(R.reshape(9), p, np.float64)
        Tm = mpmath.matrix(4, 4)
        for i in range(3):
            for j in range(3):
                Tm[i, j] = mpf(R[i, j])
            Tm[i, 3] = mpf(p[i])
        Tm[3, 3] = 1
        Lg = mpmath.logm(Tm)
        want = [Lg[0, 3], Lg[1, 3], Lg[2, 3], Lg[2, 1], Lg[0, 2], Lg[1, 0]]
        # (R is a rounded rotation: logm's skew part and the header's axis-angle agree to the rounding of R)
        assert max(float(abs(mpmath.re(a) - b)) for a, b in zip(want, truth)) < 1e-14


@pytest.mark.parametrize("robot", ["v1", "v0"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_factor_restatements(robot, dtype):
    """the restated factorisations meet the same gamma bounds the device is held to, keep the tree's zeros, and the rank-1
    recurrences reproduce U U^T + sigma x x^T; the sim-ordered M has the sparsity MJ_DOFANC describes"""
    anc = U.header_dofanc(robot)
    nv = len(anc)
    M, blob = U.robot_mass_matrices(robot, 4)
    Ms = U.sim_order(M, blob)
    P = U.pattern_mask(anc, nv)
    assert (Ms[:, ~(P | P.T)] == 0).all() and np.abs(Ms - Ms.transpose(0, 2, 1)).max() < 1e-15
    rng = np.random.default_rng(41)
    LD = np.longdouble
    for A in list(Ms) + list(U.tree_sparse_spd(rng, anc, nv, 4)):
        A = A.astype(dtype)
        A = np.triu(A) + np.triu(A, 1).T
        Uf, rd = U.chol26_restated(A, anc, dtype)
        assert (Uf[~P] == 0).all()
        Ul = Uf.astype(LD)
        res = np.abs(A.astype(LD) - Ul @ Ul.T)
        assert (res <= U.gamma(nv + 5, dtype) * (np.abs(Ul) @ np.abs(Ul).T)).all()
        Ud, _ = U.chol26_restated(A, anc, dtype, dense=True)
        assert np.array_equal(Ud, Uf)                           # on tree-sparse input the dense order updates with zeros only
        b = rng.normal(size=nv).astype(dtype)
        x = U.chol26_subst_restated(Uf, rd, b)
        r = np.abs(b.astype(LD) - A.astype(LD) @ x.astype(LD))
        assert (r <= U.gamma(3 * nv + 5, dtype) * (np.abs(Ul) @ np.abs(Ul).T @ np.abs(x.astype(LD)))).all()
        L, rdv = U.tick_chol_restated(A, dtype)
        Ll = L.astype(LD)
        assert (np.abs(A.astype(LD) - Ll @ Ll.T) <= U.gamma(nv + 5, dtype) * (np.abs(Ll) @ np.abs(Ll).T)).all()
        k = int(rng.integers(nv))
        c = anc[k] | (1 << k)
        xv = np.array([rng.normal() if (c >> i) & 1 else 0.0 for i in range(nv)]).astype(dtype)
        U1, rd1, ok = U.chol26_rank1_restated(Uf, rd, xv, 1.0, c)
        assert ok and (U1[~P] == 0).all()
        want = Ul @ Ul.T + np.outer(xv.astype(LD), xv.astype(LD))
        e = float(np.abs(U1.astype(LD) @ U1.astype(LD).T - want).max() / np.abs(want).max())
        U0, rd0, ok = U.chol26_rank1_restated(U1, rd1, xv, -1.0, c)
        back = float(np.abs(U0.astype(LD) - Ul).max() / np.abs(Ul).max())
        print(f"UNIT rank1_restated_{robot}_{np.dtype(dtype).name} update_rel_err={e:.3e} round_trip_rel_err={back:.3e}")
        cond = np.linalg.cond(A.astype(np.float64))
        assert ok and e <= 64 * U.eps_of(dtype) and back <= 64 * U.eps_of(dtype) * cond
        _, _, ok = U.chol26_rank1_restated(Uf, rd, np.eye(nv, dtype=dtype)[0] * Uf[0, 0], -1.0, 1)
        assert not ok                                           # q = 1 - s^2 <= the header's threshold


def test_trees_and_subtree_last():
    rng = np.random.default_rng(42)
    for n in (1, 16, 17, 32):
        parent = U.random_preorder_tree(rng, n)
        last = U.subtree_last(parent)
        for j in range(n):
            desc = [k for k in range(n) if k == j or j in _path(parent, k)]
            assert desc == list(range(j, last[j] + 1))          # pre-order: a subtree is a contiguous range


def _path(parent, k):
    out = []
    while parent[k] >= 0:
        k = parent[k]
        out.append(k)
    return out
