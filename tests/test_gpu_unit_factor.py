"""Unit layer, the register factorisations alone (through tests/unit/tsidb_unit.hip): tick_chol in its three forms,
chol26_solve sparse and dense, chol26_factor + chol26_subst, chol26_rank1.  256 matrices per call, both robots.
Gates (unit_testlib's rule): Higham's componentwise gamma bounds in longdouble for the factorisations and solves, exact
zeros outside the tree's pattern, bit equality where the header claims it, 8 x the restatement's own error for the rank-1
recurrences."""
import numpy as np
import pytest
import torch

import unit_testlib as U

pytestmark = pytest.mark.gpu
NM = 256
DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
LD = np.longdouble


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module", params=["v1", "v0"])
def rob(request):
    h = U.harness(request.param)
    M, blob = U.robot_mass_matrices(request.param, 32)
    return dict(h=h, name=request.param, M=M, Msim=U.sim_order(M, blob), nv=h.NV, anc=h.dofanc)


def dense_spd(rob, npdt):
    """NM SPD matrices: conditions 1 .. 1e12 (float32: 1e5), the robot's M, M + J^T D J, the identity, a wide diagonal"""
    nv, rng = rob["nv"], np.random.default_rng(30)
    f64 = npdt == np.float64
    out = []
    for c in np.linspace(0, 12 if f64 else 5, 150):
        Q, _ = np.linalg.qr(rng.normal(size=(nv, nv)))
        lam = 10.0 ** -np.concatenate([[0, c], rng.uniform(0, c, nv - 2)])
        A = (Q * lam) @ Q.T
        out.append((A + A.T) / 2)
    out += list(rob["M"])
    # D = 1e6 in float64; float32 takes the D that keeps the condition at the 1e5 its random matrices reach (with D = 1e6
    # the condition passes 1 / eps of float32: not a positive definite matrix in that type)
    for M in rob["M"]:
        J = rng.normal(size=(int(rng.integers(1, 8)), nv))
        D = 1e6 if f64 else min(1e6, 1e5 * np.linalg.eigvalsh(M)[0] / np.linalg.eigvalsh(J.T @ J)[-1])
        out.append(M + D * J.T @ J)
    out.append(np.eye(nv))
    out.append(np.diag(10.0 ** np.linspace(-6, 6, nv)))
    while len(out) < NM:
        out.append(out[len(out) % 150])
    A = np.array(out[:NM]).astype(npdt)
    return np.tril(A) + np.tril(A, -1).transpose(0, 2, 1)      # exactly symmetric after rounding


def run_tick_chol(h, name, A):
    tdt = torch.float64 if A.dtype == np.float64 else torch.float32
    n, nv = A.shape[0], h.NV
    L = torch.empty(n * 64 * nv, dtype=tdt, device="cuda")
    rdv = torch.empty(n * 64, dtype=tdt, device="cuda")
    ns = torch.empty(n * 64, dtype=torch.int32, device="cuda")
    h.call(name, dev(A), L, rdv, ns, n=n)
    torch.cuda.synchronize()
    return L.cpu().numpy().reshape(n, 64, nv), rdv.cpu().numpy().reshape(n, 64), ns.cpu().numpy().reshape(n, 64)


def factor_excess(A, F, k, npdt):
    """max over entries of |A - F F^T| / (gamma_k |F| |F|^T) (entries with a zero bound must be exact)"""
    Fl, Al = F.astype(LD), A.astype(LD)
    res = np.abs(Al - Fl @ Fl.transpose(0, 2, 1))
    bound = U.gamma(k, npdt) * (np.abs(Fl) @ np.abs(Fl).transpose(0, 2, 1))
    assert (res[bound == 0] == 0).all()
    return float((res / np.where(bound == 0, 1, bound)).max())


@pytest.mark.parametrize("form", ["tick_chol_f64_dpp", "tick_chol_f64", "tick_chol_f32"])
def test_tick_chol(rob, form):
    h, nv = rob["h"], rob["nv"]
    npdt = np.float32 if form.endswith("f32") else np.float64
    A = dense_spd(rob, npdt)
    L, rdv, ns = run_tick_chol(h, form, A)
    assert (ns == 0).all(), "notspd on an SPD matrix"
    Lt = np.tril(L[:, :nv, :])
    ex = factor_excess(A, Lt, nv + 5, npdt)
    d = np.diagonal(Lt, axis1=1, axis2=2).astype(LD)
    r = rdv[:, :nv].astype(LD)
    rd_ulp = float((np.abs(r - 1 / d) / U.ulp((1 / d).astype(np.float64), npdt)).max())
    U.report(f"{form}_{rob['name']}", n=NM, residual_over_gamma_bound=ex, rdv_worst_ulp=rd_ulp, gate_ulp=4)
    assert ex <= 1 and rd_ulp <= 4
    if form == "tick_chol_f64":
        L2, rdv2, _ = run_tick_chol(h, "tick_chol_f64_dpp", A)
        same = np.array_equal(bits(L[:, :nv]), bits(L2[:, :nv])) and np.array_equal(bits(rdv[:, :nv]), bits(rdv2[:, :nv]))
        U.report(f"tick_chol_f64_forms_{rob['name']}", bit_identical=same)
        assert same, "the DPP and the v_readlane forms are the same operations on lanes < NV"


@pytest.mark.parametrize("form", ["tick_chol_f64_dpp", "tick_chol_f64", "tick_chol_f32"])
def test_tick_chol_not_spd(rob, form):
    h, nv = rob["h"], rob["nv"]
    npdt = np.float32 if form.endswith("f32") else np.float64
    rng = np.random.default_rng(31)
    B = rng.normal(size=(nv, nv))
    base = B @ B.T + nv * np.eye(nv)
    cases = []
    for k in (0, 12, nv - 1):
        # a non-positive pivot exactly at step k: shrink A[k][k] below what the first k columns take from it
        Lk = np.linalg.cholesky(base)
        A = base.copy()
        A[k, k] = (Lk[k, :k] ** 2).sum() - 1.0
        cases.append(A)
        A = base.copy()
        A[k, k] = (Lk[k, :k] ** 2).sum() if k else 0.0   # a zero pivot (up to rounding) at k
        cases.append(A)
    d = np.ones(nv); d[5] = 0.0
    cases.append(np.diag(d))                  # exactly singular: the pivot at k = 5 is an exact zero
    cases.append(np.zeros((nv, nv)))
    A = np.array(cases).astype(npdt)
    L, rdv, ns = run_tick_chol(h, form, A)
    flagged = (ns != 0).all(axis=1)
    # required to be flagged: the strictly negative pivots (0, 2, 4), the exact zero at k = 0 (1: nothing is subtracted from it) and
    # the two exactly singular matrices.  Cases 3 and 5 put A[k][k] at what the first k columns take from it, a pivot of 0 up to
    # the rounding of k products: either sign is a right answer there, they are in for the finiteness of what comes out
    must = [0, 1, 2, 4, len(cases) - 2, len(cases) - 1]
    U.report(f"{form}_notspd_{rob['name']}", flagged=int(flagged.sum()), of=len(cases))
    assert flagged[must].all(), flagged
    assert np.isfinite(L[:, :nv]).all() and np.isfinite(rdv[:, :nv]).all()


# ------------------------------------------------------------------------------------------------ chol26_*
def sparse_spd(rob, npdt):
    """NM tree-sparse SPD matrices of the robot's MJ_DOFANC: M in the sim's dof order, M + sum sigma x x^T with x on root
    paths, and random ones"""
    nv, anc, rng = rob["nv"], rob["anc"], np.random.default_rng(32)
    out = list(rob["Msim"])
    for M in rob["Msim"]:
        A = M.copy()
        lmin = np.linalg.eigvalsh(M)[0]
        for _ in range(6):   # (sigma up to 1e4; float32: up to 1e3 x M's smallest eigenvalue, the condition that type can factor)
            k = int(rng.integers(nv))
            x = np.array([rng.normal() if (i == k or (anc[k] >> i) & 1) else 0.0 for i in range(nv)])
            A += (1e4 if npdt == np.float64 else 1e3 * lmin) * rng.uniform() * np.outer(x, x)
        out.append(A)
    out += list(U.tree_sparse_spd(rng, anc, nv, NM - len(out)))
    A = np.array(out).astype(npdt)
    A = np.triu(A) + np.triu(A, 1).transpose(0, 2, 1)
    P = U.pattern_mask(anc, nv)
    assert (A[:, ~(P | P.T)] == 0).all()
    return A


def run_solve(h, name, A, rhs, with_rdv=False):
    tdt = torch.float64 if A.dtype == np.float64 else torch.float32
    n, nv = A.shape[0], h.NV
    Uo = torch.empty(n * 64 * nv, dtype=tdt, device="cuda")
    x = torch.empty(n * 64, dtype=tdt, device="cuda")
    rdv = torch.empty(n * 64, dtype=tdt, device="cuda")
    spd = torch.empty(n * 64, dtype=torch.int32, device="cuda")
    r = np.zeros((n, 64), dtype=A.dtype)
    r[:, :nv] = rhs
    if with_rdv:
        h.call(name, dev(A), dev(r), Uo, rdv, x, spd, n=n)
    else:
        h.call(name, dev(A), dev(r), Uo, x, spd, n=n)
    torch.cuda.synchronize()
    return (Uo.cpu().numpy().reshape(n, 64, nv), x.cpu().numpy().reshape(n, 64), spd.cpu().numpy().reshape(n, 64),
            rdv.cpu().numpy().reshape(n, 64))


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_chol26_solves(rob, t):
    h, nv, anc = rob["h"], rob["nv"], rob["anc"]
    _, npdt = DT[t]
    A = sparse_spd(rob, npdt)
    rhs = np.random.default_rng(33).normal(size=(NM, nv)).astype(npdt)
    P = U.pattern_mask(anc, nv)
    res = {}
    for form in ("chol26_solve", "chol26_dense", "chol26_factor_subst"):
        Uo, x, spd, rdv = run_solve(h, f"{form}_{t}", A, rhs, with_rdv=form == "chol26_factor_subst")
        assert (spd == 1).all(), form
        Um = Uo[:, :nv, :]
        assert (Um[:, ~P] == 0).all(), f"{form}: exact zeros outside the ancestor pattern (and below the diagonal)"
        assert (Uo[:, nv:, :] == 0).all(), f"{form}: lanes >= NV stay exact zeros"
        ex = factor_excess(A, Um, nv + 5, npdt)
        Ul, xl = np.abs(Um.astype(LD)), x[:, :nv].astype(LD)
        r = np.abs(rhs.astype(LD) - np.einsum("nij,nj->ni", A.astype(LD), xl))
        bound = U.gamma(3 * nv + 5, npdt) * np.einsum("nij,nj->ni", Ul @ Ul.transpose(0, 2, 1), np.abs(xl))
        sx = float((r / bound).max())
        U.report(f"{form}_{t}_{rob['name']}", n=NM, factor_residual_over_gamma_bound=ex, solve_residual_over_gamma_bound=sx)
        assert ex <= 1 and sx <= 1, form
        if form == "chol26_factor_subst":
            d = np.diagonal(Um, axis1=1, axis2=2).astype(LD)
            rd_ulp = float((np.abs(rdv[:, :nv].astype(LD) - 1 / d) / U.ulp((1 / d).astype(np.float64), npdt)).max())
            U.report(f"chol26_factor_rdv_{t}_{rob['name']}", worst_ulp=rd_ulp, gate_ulp=4)
            assert rd_ulp <= 4
        res[form] = (Um, x[:, :nv])
    # recorded, not required: is the dense variant bit-identical to the sparse one on tree-sparse input?
    U.report(f"chol26_dense_vs_sparse_{t}_{rob['name']}", factor_bit_identical=np.array_equal(bits(res["chol26_solve"][0]), bits(res["chol26_dense"][0])),
             x_bit_identical=np.array_equal(bits(res["chol26_solve"][1]), bits(res["chol26_dense"][1])))
    assert np.array_equal(bits(res["chol26_solve"][0]), bits(res["chol26_factor_subst"][0])), "chol26_factor is chol26_solve's factorisation"


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_chol26_not_spd(rob, t):
    h, nv = rob["h"], rob["nv"]
    _, npdt = DT[t]
    A = sparse_spd(rob, npdt)[:8].copy()
    A[0, nv - 1, nv - 1] = -1.0          # the first pivot
    A[1, 0, 0] = -1.0                    # the last pivot
    A[2, 7, 7] = 0.0
    A[3] = 0
    rhs = np.ones((8, nv), dtype=npdt)
    for form in ("chol26_solve", "chol26_dense", "chol26_factor_subst"):
        _, _, spd, _ = run_solve(h, f"{form}_{t}", A, rhs, with_rdv=form == "chol26_factor_subst")
        assert (spd[:4] == 0).all() and (spd[4:] == 1).all(), (form, spd[:, 0])


def chains_of(rob):
    anc, nv = rob["anc"], rob["nv"]
    ch = [anc[k] | (1 << k) for k in range(nv)] + [1]
    return ch          # (the full leg chains are the root paths of the legs' last dofs: among these)


def run_rank1(h, t, Uin, rdv, xs, sigma, chain):
    tdt, npdt = DT[t]
    n, m, nv = xs.shape[0], xs.shape[1], h.NV
    x64 = np.zeros((n, m, 64), dtype=npdt); x64[:, :, :nv] = xs
    r64 = np.zeros((n, 64), dtype=npdt); r64[:, :nv] = rdv
    Uo = torch.empty(n * 64 * nv, dtype=tdt, device="cuda")
    ro = torch.empty(n * 64, dtype=tdt, device="cuda")
    done = torch.empty(n * 64, dtype=torch.int32, device="cuda")
    h.rank1(t, dev(Uin.astype(npdt)), dev(r64), dev(x64), dev(sigma.astype(npdt)), dev(chain.astype(np.int64)), m, Uo, ro, done, n)
    torch.cuda.synchronize()
    return Uo.cpu().numpy().reshape(n, 64, nv)[:, :nv], ro.cpu().numpy().reshape(n, 64)[:, :nv], done.cpu().numpy().reshape(n, 64)


def host_factors(rob, npdt, n):
    A = sparse_spd(rob, npdt)[:n]
    F = [U.chol26_restated(a, rob["anc"], npdt) for a in A]
    return A, np.array([f[0] for f in F]), np.array([f[1] for f in F])


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_chol26_rank1_single(rob, t):
    """one update (sigma = +1) and one downdate (sigma = -1, of a vector the matrix contains) per chain: U' U'^T against
    U U^T + sigma x x^T and rdv against the new diagonal, both at 8 x the restatement's own error + 8 ulp"""
    h, nv, anc = rob["h"], rob["nv"], rob["anc"]
    _, npdt = DT[t]
    rng = np.random.default_rng(34)
    ch = chains_of(rob)
    n = 2 * len(ch)
    A, Uh, rd = host_factors(rob, npdt, n)
    xs, sg, chain = np.zeros((n, 1, nv)), np.zeros((n, 1)), np.zeros((n, 1), dtype=np.int64)
    for i in range(n):
        c = ch[i // 2]
        x = np.array([rng.normal() if (c >> k) & 1 else 0.0 for k in range(nv)])
        # scaled to x^T A^-1 x = 1: the update grows the pivots by q = 1 + s^2 <= 2, the downdate of the same vector from
        # A + x x^T shrinks them by 1 / 2 overall - a well-conditioned change, so the restatement's error is rounding, not
        # rounding amplified by 1 / q (an unscaled x against M's 1e-3 entries makes q ~ 1e-4 .. 1e-5, the refusal threshold)
        x = (x / np.sqrt(x @ np.linalg.solve(A[i].astype(np.float64), x))).astype(npdt)
        xs[i, 0], chain[i, 0] = x, c
        if i % 2 == 0:
            sg[i, 0] = 1.0
        else:   # a downdate that stays positive definite: the factor is that of A + x x^T
            sg[i, 0] = -1.0
            Uh[i], rd[i], ok = U.chol26_rank1_restated(Uh[i], rd[i], x, 1.0, c)
            assert ok
    Ud, rdd, done = run_rank1(h, t, Uh, rd, xs, sg, chain)
    assert (done == 1).all()
    eps = U.eps_of(npdt)
    worst = dict(dev=0.0, ref=0.0, rd_dev=0.0, rd_ref=0.0)
    for i in range(n):
        Ur, rr, ok = U.chol26_rank1_restated(Uh[i], rd[i], xs[i, 0].astype(npdt), sg[i, 0], int(chain[i, 0]))
        assert ok
        want = Uh[i].astype(LD) @ Uh[i].astype(LD).T + LD(sg[i, 0]) * np.outer(xs[i, 0].astype(LD), xs[i, 0].astype(LD))
        scale = float(np.abs(want).max())
        e = lambda F: float(np.abs(F.astype(LD) @ F.astype(LD).T - want).max()) / scale
        er = lambda F, r: float(np.abs(r.astype(LD) * np.diagonal(F).astype(LD) - 1).max())
        ed, ef, rdev, rref = e(Ud[i]), e(Ur), er(Ud[i], rdd[i]), er(Ur, rr)
        worst = dict(dev=max(worst["dev"], ed), ref=max(worst["ref"], ef), rd_dev=max(worst["rd_dev"], rdev), rd_ref=max(worst["rd_ref"], rref))
        assert ed <= 8 * ef + 8 * eps, (i, ed, ef)
        assert rdev <= 8 * rref + 8 * eps, (i, rdev, rref)
        off = [k for k in range(nv) if not (int(chain[i, 0]) >> k) & 1]
        assert np.array_equal(bits(Ud[i][:, off]), bits(Uh[i][:, off].astype(npdt))), "pivots off the chain are untouched"
    U.report(f"chol26_rank1_{t}_{rob['name']}", n=n, dev_rel_err=worst["dev"], restated_rel_err=worst["ref"], rdv_dev=worst["rd_dev"], rdv_restated=worst["rd_ref"])


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_chol26_rank1_round_trip_refusal_and_support(rob, t):
    h, nv, anc = rob["h"], rob["nv"], rob["anc"]
    _, npdt = DT[t]
    rng = np.random.default_rng(35)
    ch = chains_of(rob)
    n, m = 16, 64
    A, Uh, rd = host_factors(rob, npdt, n)
    xs, chain = np.zeros((n, m, nv)), np.zeros((n, m), dtype=np.int64)
    for i in range(n):
        for r in range(32):
            c = ch[int(rng.integers(len(ch)))]
            x = np.array([rng.normal() if (c >> k) & 1 else 0.0 for k in range(nv)])
            # x^T A^-1 x = 1/4: every downdate removes a vector from a matrix that is at least A + x x^T, so its pivots keep
            # q >= 4/5 - far from the header's refusal threshold, which an unscaled x against M's 1e-3 entries reaches
            xs[i, r] = xs[i, 32 + r] = 0.5 * x / np.sqrt(x @ np.linalg.solve(A[i].astype(np.float64), x))
            chain[i, r] = chain[i, 32 + r] = c
    xs = xs.astype(npdt)
    sg = np.concatenate([np.ones((n, 32)), -np.ones((n, 32))], axis=1)
    Ud, rdd, done = run_rank1(h, t, Uh, rd, xs, sg, chain)
    assert (done == m).all()
    worst = dict(dev=0.0, ref=0.0)
    for i in range(n):
        Ur, rr = Uh[i], rd[i]
        for r in range(m):
            Ur, rr, ok = U.chol26_rank1_restated(Ur, rr, xs[i, r], sg[i, r], int(chain[i, r]))
            assert ok
        scale = float(np.abs(Uh[i]).max())
        ed, ef = float(np.abs(Ud[i].astype(LD) - Uh[i].astype(LD)).max()) / scale, float(np.abs(Ur.astype(LD) - Uh[i].astype(LD)).max()) / scale
        worst = dict(dev=max(worst["dev"], ed), ref=max(worst["ref"], ef))
        assert ed <= 8 * ef + 8 * U.eps_of(npdt), (i, ed, ef)
    U.report(f"chol26_rank1_round_trip_{t}_{rob['name']}", n=n, dev_rel_err=worst["dev"], restated_rel_err=worst["ref"])
    # a downdate that takes the whole pivot: q = 1 - s^2 = 0 <= the header's threshold -> refused, nothing applied
    x1 = np.zeros((n, 1, nv)); x1[:, 0, 0] = Uh[:, 0, 0]
    _, _, done = run_rank1(h, t, Uh, rd, x1, -np.ones((n, 1)), np.ones((n, 1), dtype=np.int64))
    assert (done == 0).all()
    # chain bits outside the support of x: those pivots come back bit-identical
    full = (1 << nv) - 1
    x2 = np.zeros((n, 1, nv)); x2[:, 0, :6] = rng.normal(size=(n, 6))
    U2, r2, done = run_rank1(h, t, Uh, rd, x2, np.ones((n, 1)), np.full((n, 1), full, dtype=np.int64))
    assert (done == 1).all()
    assert np.array_equal(bits(U2[:, :, 6:]), bits(Uh[:, :, 6:].astype(npdt))) and np.array_equal(bits(r2[:, 6:]), bits(rd[:, 6:].astype(npdt)))
