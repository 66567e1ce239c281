"""Unit layer, wavefront primitives alone (tsidb_common.hpp / tsidb_tick.hpp through tests/unit/tsidb_unit.hip): the DPP
reductions, subtree_sum32 / bperm, row_dup / bcast_fnma / bcast_fnma2 with their hand-placed wait states, the lane reads and
env_of_block.  Gates: unit_testlib's rule - bit equality wherever an exact answer exists, textbook bounds otherwise."""
import math

import numpy as np
import pytest
import torch

import unit_testlib as U

pytestmark = pytest.mark.gpu
NB = 64  # blocks (wavefronts) per call
DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
EDGE_LANES = (0, 15, 16, 31, 32, 47, 48, 63)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def run1(h, name, x, out_elems=None):
    """unary wave entry point on a (NB, 64) host array; returns the (NB, 64[, ...]) host result"""
    xd = dev(x)
    out = torch.empty(out_elems or xd.numel(), dtype=xd.dtype, device="cuda")
    h.call(name, xd, out, n=x.shape[0])
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def h():
    return U.harness("v1")


def sum_inputs(npdt, rng):
    """(NB, 64): integer-valued rows, single non-zero lanes, then mixed signs and magnitudes 1e-8 .. 1e8"""
    x = np.zeros((NB, 64))
    x[:16] = rng.integers(-1000, 1000, (16, 64))
    for r, lane in enumerate(EDGE_LANES):
        x[16 + r, lane] = 3.0 + r
    x[24:] = rng.choice([-1.0, 1.0], (NB - 24, 64)) * 10.0 ** rng.uniform(-8, 8, (NB - 24, 64))
    return x.astype(npdt)


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_wave_sum_and_sum3(h, t):
    _, npdt = DT[t]
    rng = np.random.default_rng(1)
    xs = [sum_inputs(npdt, rng) for _ in range(3)]
    outs = [run1(h, f"wave_sum_{t}", x).reshape(NB, 64) for x in xs]
    worst = 0.0
    for x, o in zip(xs, outs):
        assert (bits(o) == bits(o[:, :1])).all(), "every lane gets the same sum"
        exact = np.array([math.fsum(float(v) for v in row) for row in x])
        assert np.array_equal(o[:24, 0].astype(np.float64), exact[:24]), "integer-valued and single-lane rows are exact"
        bound = 6 * U.eps_of(npdt) * np.abs(x.astype(np.float64)).sum(axis=1)
        err = np.abs(o[:, 0].astype(np.float64) - exact)
        worst = max(worst, float((err[24:] / bound[24:]).max()))
        assert (err <= bound).all()
    d = [dev(x) for x in xs]
    o3 = [torch.empty_like(d[0]) for _ in range(3)]
    h.call(f"wave_sum3_{t}", *d, *o3, n=NB)
    torch.cuda.synchronize()
    for o, ref in zip(o3, outs):
        assert np.array_equal(bits(o.cpu().numpy().reshape(NB, 64)), bits(ref)), "wave_sum3 = three wave_sums, bit for bit"
    U.report(f"wave_sum_{t}", worst_err_over_gate=worst, gate="6*eps*sum|v|")


def test_wave_sum_int(h):
    rng = np.random.default_rng(2)
    x = rng.integers(-2 ** 20, 2 ** 20, (NB, 64)).astype(np.int32)
    x[:8] = 0
    for r, lane in enumerate(EDGE_LANES):
        x[r, lane] = 7 + r
    o = run1(h, "wave_sum_int", x).reshape(NB, 64)
    assert np.array_equal(o, np.repeat(x.sum(axis=1, dtype=np.int64).astype(np.int32)[:, None], 64, axis=1))
    U.report("wave_sum_int", mismatches=0)


def min_inputs(npdt, rng, integer):
    """rows 0..63: the unique minimum at lane r; then ties across row boundaries, all equal, negatives, +inf, +-0"""
    rows = []
    for r in range(64):
        v = rng.integers(10, 1000, 64).astype(np.float64)
        v[r] = 3
        rows.append(v)
    for pair in ((15, 16), (31, 32), (47, 48), (0, 63), (16, 17, 48), (5, 21, 37, 53)):
        v = rng.integers(10, 1000, 64).astype(np.float64)
        v[list(pair)] = -5
        rows.append(v)
    rows.append(np.full(64, 42.0))
    rows.append(-rng.integers(1, 1000, 64).astype(np.float64))
    if not integer:
        v = np.full(64, np.inf); v[40] = 1e30; v[41] = 2e30
        rows.append(v)
        rows.append(np.full(64, np.inf))
        v = np.zeros(64); v[33] = -0.0; v[20] = 5.0
        rows.append(v)
        rows.append(rng.normal(size=64) * 10.0 ** rng.uniform(-30, 30, 64))
    return np.array(rows).astype(npdt)


@pytest.mark.parametrize("t", ["f32", "f64", "i32"])
def test_wave_min(h, t):
    npdt = np.int32 if t == "i32" else DT[t][1]
    x = min_inputs(npdt, np.random.default_rng(3), t == "i32")
    o = run1(h, f"wave_min_{t}", x).reshape(x.shape)
    assert np.array_equal(o, np.repeat(x.min(axis=1)[:, None], 64, axis=1))  # (-0 == +0: either zero is a minimum)
    U.report(f"wave_min_{t}", rows=len(x), mismatches=0)


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_wave_argmin(h, t):
    _, npdt = DT[t]
    rng = np.random.default_rng(4)
    x = min_inputs(npdt, rng, False)
    n = len(x)
    for idx in (np.tile(np.arange(64, dtype=np.int32), (n, 1)),                       # the lane id
                np.tile((1000 - 7 * np.arange(64)).astype(np.int32), (n, 1)),         # descending: not the lane order
                rng.permuted(np.tile(np.arange(100, 164, dtype=np.int32), (n, 1)), axis=1)):
        xd, idd = dev(x), dev(idx)
        ov, oi = torch.empty_like(xd), torch.empty_like(idd)
        h.call(f"wave_argmin_{t}", xd, idd, ov, oi, n=n)
        torch.cuda.synchronize()
        ov, oi = ov.cpu().numpy().reshape(n, 64), oi.cpu().numpy().reshape(n, 64)
        vmin = x.min(axis=1)
        want = np.array([idx[r][x[r] == vmin[r]].min() for r in range(n)])   # lowest caller index among equals
        assert np.array_equal(ov, np.repeat(vmin[:, None], 64, axis=1))
        assert np.array_equal(oi, np.repeat(want[:, None], 64, axis=1))
    U.report(f"wave_argmin_{t}", rows=n, mismatches=0)


def trees():
    from tsid_control_amd.model import ModelBlob
    rng = np.random.default_rng(5)
    out = []
    for r in ("v1", "v0"):
        blob = ModelBlob(U.ROOT / "tsid_control_amd" / "assets" / U.ROBOTS[r][1])
        out += [(f"{r} pin", list(blob["pin_parent"])), (f"{r} mj", list(blob["mj_parent"]))]
    out += [("chain32", [-1] + list(range(31))), ("star32", [-1] + [0] * 31)]
    for n in (1, 16, 17, 32):
        out += [(f"random{n}", U.random_preorder_tree(rng, n)) for _ in range(3)]
    return out


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_subtree_sum32(h, t):
    _, npdt = DT[t]
    rng = np.random.default_rng(6)
    tr = trees()
    n = 2 * len(tr)
    v, last = np.zeros((n, 64), dtype=npdt), np.tile(np.arange(64, dtype=np.int32), (n, 1))
    for k, (_, parent) in enumerate(tr):
        m = len(parent)
        la = U.subtree_last(parent)
        last[2 * k, :m] = last[2 * k + 1, :m] = la
        v[2 * k, :m] = rng.integers(-1000, 1000, m)
        v[2 * k + 1, :m] = rng.normal(size=m) * 10.0 ** rng.uniform(-3, 3, m)
    vd, ld = dev(v), dev(last)
    out = torch.empty_like(vd)
    h.call(f"subtree_sum32_{t}", vd, ld, out, n=n)
    torch.cuda.synchronize()
    o = out.cpu().numpy().reshape(n, 64)
    worst = 0.0
    for k, (name, parent) in enumerate(tr):
        m = len(parent)
        la = U.subtree_last(parent)
        for row in (2 * k, 2 * k + 1):
            x = v[row].astype(np.float64)
            for j in range(m):
                exact = math.fsum(x[j:la[j] + 1])
                got = float(o[row, j])
                if la[j] == j:
                    assert bits(o[row, j:j + 1])[0] == bits(v[row, j:j + 1])[0], (name, j, "a leaf returns its own value")
                elif row % 2 == 0:
                    assert got == exact, (name, j)
                else:
                    # S_j = (P[last] - P[j]) + v_j: each prefix carries at most 5 scan additions, each off by eps/2 of a partial
                    # sum bounded by sum |v[0..last]|, and the two final operations add eps/2 each: 12 * eps/2 of that sum
                    bound = 6 * U.eps_of(npdt) * np.abs(x[:la[j] + 1]).sum()
                    worst = max(worst, abs(got - exact) / bound)
                    assert abs(got - exact) <= bound, (name, j, got, exact)
    U.report(f"subtree_sum32_{t}", trees=len(tr), worst_err_over_gate=worst, gate="6*eps*sum|v[0..last]|")


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_bperm_bcast_lane_reads(h, t):
    """every source lane; payloads whose two dwords differ (random bit patterns of finite floats)"""
    tdt, npdt = DT[t]
    rng = np.random.default_rng(7)
    x = (rng.normal(size=(NB, 64)) * 10.0 ** rng.uniform(-20, 20, (NB, 64))).astype(npdt)
    if t == "f64":
        assert ((bits(x) >> np.uint64(32)) != (bits(x) & np.uint64(0xffffffff))).all()
    src = rng.integers(0, 64, (NB, 64)).astype(np.int32)
    src[0] = np.arange(64); src[1] = 63 - np.arange(64); src[2] = (np.arange(64) + 16) % 64
    for name in ("bperm", "bcast"):
        xd, sd = dev(x), dev(src)
        out = torch.empty_like(xd)
        h.call(f"{name}_{t}", xd, sd, out, n=NB)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy().reshape(NB, 64)), bits(np.take_along_axis(x, src.astype(np.int64), axis=1))), name
    o = run1(h, f"lane63_{t}", x).reshape(NB, 64)
    assert np.array_equal(bits(o), bits(np.repeat(x[:, 63:], 64, axis=1)))
    o = run1(h, f"rdlane_{t}", x[:8], out_elems=8 * 4096).reshape(8, 64, 64)
    assert np.array_equal(bits(o), bits(np.repeat(x[:8, :, None], 64, axis=2))), "rdlane: lane l reads source lane s"
    order = np.stack([rng.permutation(64) for _ in range(8)]).astype(np.int32)
    xd, od = dev(x[:8]), dev(order)
    out = torch.empty(8 * 4096, dtype=tdt, device="cuda")
    h.call(f"rdlane_dyn_{t}", xd, od, out, n=8)
    torch.cuda.synchronize()
    want = np.repeat(np.take_along_axis(x[:8], order.astype(np.int64), axis=1)[:, :, None], 64, axis=2)
    assert np.array_equal(bits(out.cpu().numpy().reshape(8, 64, 64)), bits(want))
    U.report(f"lane_reads_{t}", mismatches=0)


def test_lane63_int(h):
    x = np.random.default_rng(8).integers(-2 ** 31, 2 ** 31 - 1, (NB, 64)).astype(np.int32)
    assert np.array_equal(run1(h, "lane63_i32", x).reshape(NB, 64), np.repeat(x[:, 63:], 64, axis=1))


def test_env_of_block(h):
    for n in list(range(1, 71)) + [257, 4096]:
        out = torch.empty(n, dtype=torch.int32, device="cuda")
        h.call("env_of_block", out, n=n)
        torch.cuda.synchronize()
        e = out.cpu().numpy()
        assert sorted(e.tolist()) == list(range(n)), n                      # a bijection onto 0 .. n-1
        for x in range(min(8, n)):                                           # a contiguous range per XCD residue, in block order
            r = e[x::8]
            assert np.array_equal(r, np.arange(r[0], r[0] + len(r))), (n, x)
    U.report("env_of_block", sizes=72, mismatches=0)


# ------------------------------------------------------------------------------------------------ row_dup / bcast_fnma*
SCALES = {0: (1.0, 1.0), 1: (0.5, 4.0)}   # variant 1 multiplies by these powers of two in front of the broadcast: exact


def fnma_data(rng):
    x = rng.normal(size=(NB, 64)) * 10.0 ** rng.uniform(-2, 2, (NB, 64))
    m = rng.normal(size=(NB, 64))
    a = rng.normal(size=(NB, 64, 32)) * 10.0 ** rng.uniform(-2, 2, (NB, 64, 32))
    return x, m, a


@pytest.mark.parametrize("var", [0, 1])
def test_row_dup(h, var):
    rng = np.random.default_rng(9)
    x, _, _ = fnma_data(rng)
    xd, sc = dev(x), dev(np.array(SCALES[var]))
    lo, hi = torch.empty_like(xd), torch.empty_like(xd)
    h.call("row_dup", var, xd, sc, lo, hi, n=NB)
    torch.cuda.synchronize()
    lo, hi = lo.cpu().numpy().reshape(NB, 64), hi.cpu().numpy().reshape(NB, 64)
    xe = x * SCALES[var][0] * SCALES[var][1]
    # rows 0 and 1 (lanes 0..31) of lo hold x's lanes 0..15, of hi its lanes 16..31; nothing is asserted about lanes >= 32
    assert np.array_equal(bits(lo[:, :32]), bits(np.tile(xe[:, :16], (1, 2))))
    assert np.array_equal(bits(hi[:, :32]), bits(np.tile(xe[:, 16:32], (1, 2))))
    U.report(f"row_dup_var{var}", mismatches=0)


@pytest.mark.parametrize("robot", ["v1", "v0"])
@pytest.mark.parametrize("var", [0, 1])
def test_bcast_fnma(robot, var):
    """lanes 0..31 of a[j], j in MASK, equal fma(-x[j], m, a[j]) with an exactly rounded host FMA, bit for bit; a[j] outside
    the mask is untouched.  Checked exhaustively on 2 blocks per mask (the host FMA is rational arithmetic)."""
    hh = U.harness(robot)
    rng = np.random.default_rng(10)
    x, m, a = fnma_data(rng)
    nb = 2
    xd, md, ad, sc = dev(x[:nb]), dev(m[:nb]), dev(a[:nb]), dev(np.array(SCALES[var]))
    xe = x * SCALES[var][0] * SCALES[var][1]
    for mi, mask in enumerate(hh.fnma_masks):
        out = torch.empty_like(ad)
        hh.call("bcast_fnma", mi, var, xd, sc, md, ad, out, n=nb)
        torch.cuda.synchronize()
        o = out.cpu().numpy().reshape(nb, 64, 32)
        for b in range(nb):
            for j in range(32):
                if (mask >> j) & 1:
                    want = np.array([U.fma_exact(-xe[b, j], m[b, l], a[b, l, j]) for l in range(32)])
                else:
                    want = a[b, :32, j]
                assert np.array_equal(bits(o[b, :32, j]), bits(want)), (hex(mask), b, j)
    U.report(f"bcast_fnma_{robot}_var{var}", masks=len(hh.fnma_masks), mismatches=0)


@pytest.mark.parametrize("robot", ["v1", "v0"])
@pytest.mark.parametrize("var", [0, 1])
def test_bcast_fnma2(robot, var):
    """s_(j & 1) = fma(-x[j], m[j], s_(j & 1)) over the mask's j in ascending order, two interleaved chains"""
    hh = U.harness(robot)
    rng = np.random.default_rng(11)
    x, _, mm = fnma_data(rng)
    s = rng.normal(size=(NB, 64, 2))
    nb = 2
    xd, md, sd, sc = dev(x[:nb]), dev(mm[:nb]), dev(s[:nb]), dev(np.array(SCALES[var]))
    xe = x * SCALES[var][0] * SCALES[var][1]
    for mi, mask in enumerate(hh.fnma2_masks):
        out = torch.empty_like(sd)
        hh.call("bcast_fnma2", mi, var, xd, sc, md, sd, out, n=nb)
        torch.cuda.synchronize()
        o = out.cpu().numpy().reshape(nb, 64, 2)
        for b in range(nb):
            for l in range(32):
                acc = [s[b, l, 0], s[b, l, 1]]
                for j in range(32):
                    if (mask >> j) & 1:
                        acc[j & 1] = U.fma_exact(-xe[b, j], mm[b, l, j], acc[j & 1])
                assert np.array_equal(bits(o[b, l]), bits(np.array(acc))), (hex(mask), b, l)
    U.report(f"bcast_fnma2_{robot}_var{var}", masks=len(hh.fnma2_masks), mismatches=0)
