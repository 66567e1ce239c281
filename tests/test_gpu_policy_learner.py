"""The policy learner on the device (tsidb_policy_learn, PolicyLearner) against the float64 restatement
tests/policy_learner_reference.py.  The yardstick of every gradient is torch's CPU float32 autograd of the same case, E = e32(case),
computed here: the device passes when max|g_dev - g64| <= 8 max(E, 2^-22) max|g64| per parameter tensor, stats 0 .. 5 likewise
relative to max(1, |ref|).  The 8: the device sums the batch as one k-ordered fmaf chain per segment where torch's CPU kernels
sum in blocks, and expf / logf differ by an ulp or two."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_actor_reference as RA  # noqa: E402
import policy_learner_reference as R  # noqa: E402
from policy_testlib import capture, host, make_env  # noqa: E402
from test_policy_learner_reference import e32  # noqa: E402

pytestmark = pytest.mark.gpu

ACT = {"elu": torch.nn.ELU, "tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}
N = 33                                     # envs of every synthetic storage: rows = T * 33
_envs = {}


def env_of(v0, n=N):
    if (v0, n) not in _envs:
        _envs[v0, n] = make_env(n, "f32", v0=v0, decimation=2)
    return _envs[v0, n]


def torch_net(layers, act, device):
    mods = []
    for i, (w, b) in enumerate(layers):
        lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=b is not None)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w))
            if b is not None:
                lin.bias.copy_(torch.from_numpy(b))
        mods.append(lin)
        if i + 1 < len(layers):
            mods.append(ACT[act]())
    return torch.nn.Sequential(*mods).to(device)


def padded(shape, dtype, device, before=1, after=1):
    """a NaN-filled (for ints: -1-filled) allocation with `before` / `after` more leading rows than shape, and the view of shape
    inside it: a read past either end of the view lands in memory the test owns"""
    fill = float("nan") if dtype.is_floating_point else -1
    big = torch.full((shape[0] + before + after,) + tuple(shape[1:]), fill, dtype=dtype, device=device)
    return big, big[before:before + shape[0]]


def build(case, **kw):
    """(PolicyActor, RolloutStorage, PolicyLearner, index) of a case on the device; every stored tensor is a view into a larger
    NaN-filled allocation, value's row T is NaN as well: nothing beyond the T * N stored rows may be read"""
    from tsid_control_amd import PolicyActor, PolicyLearner, RolloutStorage
    env = env_of(case["v0"])
    dev = env.device
    assert env.NA == case["na"] and case["rows"] % N == 0
    T = case["rows"] // N
    blocks = {k: torch.zeros(N, case[k + "_input"].shape[1], dtype=env.dtype, device=dev) for k in ("actor", "critic") if case[k] is not None}
    nets = {k: torch_net(*case[k], dev) for k in blocks}
    pa = PolicyActor(env, nets["actor"], nets.get("critic"), actor_inputs=(blocks["actor"],),
                     critic_inputs=(blocks["critic"],) if "critic" in blocks else None, log_std=torch.from_numpy(case["log_std"]).to(dev))
    st = RolloutStorage(env, pa, T)
    st.gae()
    st._keep = []
    for k in ("actor_input", "critic_input", "action", "logp", "advantage", "returns", "value"):
        if case[k] is None:
            continue
        old = getattr(st, k)
        shape = old.shape if k != "value" else (T,) + tuple(old.shape[1:])
        big, view = padded(shape, torch.float32, dev, after=2 if k == "value" else 1)
        view.copy_(torch.from_numpy(case[k]).reshape(shape))
        if k == "value":
            view = big[1:T + 2]                       # [T + 1, N]: the last row NaN
        assert view.is_contiguous() and view.shape == old.shape
        setattr(st, k, view)
        st._keep.append(big)
    pl = PolicyLearner(pa, clip=case["clip"], value_coef=case["value_coef"], entropy_coef=case["entropy_coef"], value_clip=case["value_clip"],
                       normalize_advantage=case["adv_stats"] is not None, **kw)
    pl.adv_stats.copy_(torch.from_numpy(case["adv_stats"]))
    return pa, st, pl, torch.from_numpy(case["index"]).to(dev)


def run(pl, st, index):
    """one backward with the case's own adv_stats (not refilled from the storage); ({name: gradient}, stats) on the host"""
    stats = pl.backward(st, index, adv_stats=pl.adv_stats)
    torch.cuda.synchronize()
    return grads_of(pl), host(stats)


def grads_of(pl):
    a = pl.actor
    out = {}
    for name, net in (("actor", a.actor_net), ("critic", a.critic_net)):
        for l, (w, b) in enumerate(net.layers if net is not None else []):
            out[f"{name}.{l}.weight"] = host(w.grad)
            if b is not None:
                out[f"{name}.{l}.bias"] = host(b.grad)
    out["log_std"] = host(a.log_std.grad)
    return out


def gate_ratio(case, got, stats, ev=None, E=None):
    """the largest error / gate over the parameter tensors and over stats 0 .. 5, each printed"""
    ev = R.evaluate(case) if ev is None else ev
    E = max(e32(case) if E is None else E, 2.0 ** -22)
    worst = 0.0
    want = dict(R.grad_list(ev))
    assert sorted(want) == sorted(got)
    for k, g64 in want.items():
        assert got[k].shape == g64.shape and np.isfinite(got[k]).all(), k
        if not np.abs(g64).max():                  # (a gradient that is 0 throughout - behind the all-ties critic's zero weights: 0 here too)
            assert not np.abs(got[k]).max(), k
            continue
        ratio = float(np.abs(got[k] - g64).max() / (8 * E * np.abs(g64).max()))
        print(f"{case['name']} {k}: error / gate {ratio:.3f}")
        worst = max(worst, ratio)
    for i in range(6):
        ratio = float(abs(stats[i] - ev["stats"][i]) / (8 * E * max(1.0, abs(ev["stats"][i]))))
        print(f"{case['name']} stats[{i}] {R.STATS[i]}: error / gate {ratio:.3f}")
        worst = max(worst, ratio)
    print(f"{case['name']}: E = {E:.2e}, largest error / gate {worst:.3f}")
    return worst, ev


# ---------------------------------------------------------------------------- (1) the gradients against the float64 reference
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_gradients_match_the_float64_reference(name):
    """every case of policy_learner_reference.CASES: both robots; 1, 17, 33 and TSIDB_POL_LEARN_SEG_ROWS + 17 rows out of a larger
    storage by a shuffled index with repeats; tanh, ELU (K = 75, no multiple of 4; a layer without bias; value_clip off) and ReLU
    networks, the 512-wide one whose LDS images exceed 64 KB, without a critic; the all-ties case.  stats 6, 7 exact.
    Measured (MI355X), E and the largest error / gate: tanh_relu_17 1.28e-6, 0.159; elu3_nobias_33 1.11e-6, 0.125; segments 1.91e-6,
    0.099; wide_no_critic 1.09e-6, 0.127; v0_single_row 1.14e-6, 0.127; v0_elu3_17 5.84e-7, 0.106; all_ties 7.02e-7, 0.255."""
    case = R.make_case(name)
    pa, st, pl, index = build(case)
    got, stats = run(pl, st, index)
    worst, ev = gate_ratio(case, got, stats)
    assert worst <= 1.0
    assert list(stats[6:]) == [case["M"], 0]
    mu, v = pl.outputs(case["M"])
    assert np.abs(host(mu) - ev["mu"]).max() <= 1e-4 * max(1.0, np.abs(ev["mu"]).max())
    assert (v is None) == (case["critic"] is None)


# ---------------------------------------------------------------------------- (2) the forward pass is the actor's
def test_forward_pass_is_the_actors_bit_for_bit_on_a_real_rollout():
    """4 steps of 17 envs, weights untouched: the learner's mu and v of stored row j are storage.mean[j] and storage.value[j] bit
    for bit, and r = exp(logp - logp_old) stays within the float32 rounding of the two logp formulas - the actor's from eps, the
    learner's from z = (action - mu) / sigma.  The bound per row, u = 2^-24: each formula's own error is
    policy_actor_reference.sample's b_logp; z differs from eps by dz_a = (4 u (|mu_a| + |sigma_a eps_a|) / sigma_a + 2 u |eps_a|)
    (the action's rounding over sigma, the subtraction and the division), which moves logp by sum_a (|eps_a| dz_a + dz_a^2 / 2).
    With clip = expm1 of the largest such bound (+ 2^-23 for 1 +- clip itself) no row may count as clipped.
    Measured (MI355X): clip 1.65e-4, clip_fraction 0, approx_kl -2.8e-8."""
    from tsid_control_amd import PolicyLearner
    from test_gpu_policy_actor import small_actor
    n, T = 17, 4
    env = env_of(False, n)
    pa = small_actor(env, seed=5)[0]
    st = env.rollout(pa, T)
    st.gae()
    torch.cuda.synchronize()
    NA = env.NA
    mean, action, ls = host(st.mean).reshape(-1, NA).astype(np.float64), host(st.action).reshape(-1, NA).astype(np.float64), host(pa.log_std)
    sigma = np.exp(ls.astype(np.float64))
    eps = (action - mean) / sigma
    s = RA.sample(mean, np.zeros_like(mean), ls, eps)
    dz = 4 * RA.U32 * (np.abs(mean) + np.abs(sigma * eps)) / sigma + 2 * RA.U32 * np.abs(eps)
    bound = 2 * s["b_logp"] + (np.abs(eps) * dz + 0.5 * dz * dz).sum(1)
    clip = float(np.expm1(bound.max()) + 2.0 ** -23)
    assert 0 < clip < 1e-3
    pl = PolicyLearner(pa, clip=clip)
    index = torch.randperm(n * T, generator=torch.Generator().manual_seed(1)).to(torch.int32).to(env.device)
    stats = host(pl.backward(st, index))
    mu, v = pl.outputs(n * T)
    j = index.long()
    assert torch.equal(mu, st.mean.reshape(-1, NA)[j]) and torch.equal(v, st.value[:T].reshape(-1)[j])
    assert float(st.mean.abs().max()) > 1e-3 and float(st.value.abs().max()) > 1e-3
    print(f"clip {clip:.2e}, clip_fraction {stats[4]}, approx_kl {stats[3]:.2e}, bound {bound.max():.2e}")
    assert stats[4] == 0 and abs(stats[3]) <= bound.max() and list(stats[6:]) == [n * T, 0]


# ---------------------------------------------------------------------------- (3) - (6) bits
def test_two_calls_rows_outside_the_index_a_permutation_and_bad_indices():
    """on the two-segment case.  Two calls: the same bits.  Every stored row not in index overwritten with NaN: the same bits.
    A permuted index: inside the gate, rows used the same.  index + [-1, T * N] with every tensor inside a NaN-filled allocation:
    inside the gate of its own reference, and the result of the call without the two times M / (M + 2) - the means stay over the
    length of index - to twice the gate (each side is within one gate of references that are exactly so related), stats[7] = 2."""
    case = R.make_case("segments")
    pa, st, pl, index = build(case)
    E = max(e32(case), 2.0 ** -22)
    g1, s1 = run(pl, st, index)
    for p in pl.parameters():
        p.grad.fill_(7.0)
    g2, s2 = run(pl, st, index)
    assert all(np.array_equal(g1[k], g2[k]) for k in g1) and np.array_equal(s1, s2)
    # the rows outside index
    unused = torch.ones(case["rows"], dtype=torch.bool, device=index.device)
    unused[index.long()] = False
    assert int(unused.sum()) > 50
    for k in ("actor_input", "critic_input", "action", "logp", "advantage", "returns"):
        t = getattr(st, k)
        t.view(case["rows"], -1)[unused] = float("nan")
    st.value[:-1].view(-1)[unused] = float("nan")
    g3, s3 = run(pl, st, index)
    assert all(np.array_equal(g1[k], g3[k]) for k in g1) and np.array_equal(s1, s3)
    # permuted
    perm = index[torch.randperm(len(index), generator=torch.Generator().manual_seed(2)).to(index.device)].contiguous()
    g4, s4 = run(pl, st, perm)
    worst, ev = gate_ratio(case, g4, s4, E=E)
    assert worst <= 1.0 and s4[6] == s1[6] == case["M"]
    assert any(not np.array_equal(g1[k], g4[k]) for k in g1)
    # bad indices, at the end: the rows before them keep their tiles
    M = case["M"]
    bad = torch.cat([index, torch.tensor([-1, case["rows"]], dtype=torch.int32, device=index.device)])
    g5, s5 = run(pl, st, bad)
    assert list(s5[6:]) == [M, 2] and list(s1[6:]) == [M, 0]
    worst5, _ = gate_ratio(dict(case, index=host(bad)), g5, s5, E=E)
    assert worst5 <= 1.0
    f = M / (M + 2.0)
    for k in g1:
        ec = case["entropy_coef"] if k == "log_std" else 0.0
        want, have = g1[k].astype(np.float64) + ec, g5[k].astype(np.float64) + ec
        assert np.abs(have - want * f).max() <= 2 * 8 * E * np.abs(want).max(), k
    for i in (0, 1, 3, 4):
        assert abs(s5[i] - s1[i] * f) <= 2 * 8 * E * max(1.0, abs(s1[i])), i
    assert s5[2] == s1[2]


# ---------------------------------------------------------------------------- (7) in place
def test_an_optimizer_step_is_seen_by_the_next_backward_and_the_next_act_and_update_is_the_hand_driven_loop():
    case = R.make_case("tanh_relu_17")
    pa, st, pl, index = build(case)
    opt = torch.optim.SGD(pl.parameters(), lr=0.05)
    g0, _ = run(pl, st, index)
    before = pl.outputs(case["M"])[0].clone()
    opt.step()
    torch.cuda.synchronize()
    moved = dict(case, log_std=host(pa.log_std))
    for which, net in (("actor", pa.actor_net), ("critic", pa.critic_net)):
        moved[which] = ([(host(w), host(b) if b is not None else None) for w, b in net.layers], case[which][1])
    assert np.abs(moved["actor"][0][0][0] - case["actor"][0][0][0]).max() > 1e-4 and np.abs(moved["log_std"] - case["log_std"]).max() > 1e-5
    g1, s1 = run(pl, st, index)
    worst, ev = gate_ratio(moved, g1, s1)
    assert worst <= 1.0
    mu = pl.outputs(case["M"])[0]
    assert float((mu - before).abs().max()) > 1e-4
    # act() on the rows of the storage the index names: the same new weights, the same bits as the learner's forward pass
    rows = min(N, case["M"])
    j = index.long()[:rows]
    pa.actor_net.blocks[0][:rows].copy_(st.actor_input.reshape(case["rows"], -1)[j])
    pa.critic_net.blocks[0][:rows].copy_(st.critic_input.reshape(case["rows"], -1)[j])
    out = pa.act(deterministic=True)
    torch.cuda.synchronize()
    assert torch.equal(out["mean"][:rows], mu[:rows]) and torch.equal(out["value"][:rows], pl.outputs(case["M"])[1][:rows])
    # update() against the loop by hand, from the same weights with the same generator seed
    start = [p.detach().clone() for p in pl.parameters()]
    st2 = st
    gen = torch.Generator(device=index.device).manual_seed(11)
    stats = pl.update(st2, opt, epochs=2, minibatches=3, generator=gen).clone()
    torch.cuda.synchronize()
    ended = [p.detach().clone() for p in pl.parameters()]
    with torch.no_grad():
        for p, s in zip(pl.parameters(), start):
            p.copy_(s)
    gen = torch.Generator(device=index.device).manual_seed(11)
    pl.fill_adv_stats(st2)
    mine, rows = [], case["rows"]
    for ep in range(2):
        perm = torch.randperm(rows, generator=gen, dtype=torch.int32, device=index.device)
        for k in range(3):
            mine.append(pl.backward(st2, perm[k * rows // 3:(k + 1) * rows // 3].contiguous(), adv_stats=pl.adv_stats).clone())
            opt.step()
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(mine), stats) and stats.shape == (6, 8) and bool(torch.isfinite(stats).all())
    assert all(torch.equal(p, e) for p, e in zip(pl.parameters(), ended))
    assert any(not torch.equal(s, e) for s, e in zip(start, ended)) and list(host(stats[:, 6])) == [22.0] * 6


# ---------------------------------------------------------------------------- (8) a captured backward
def test_captured_backward_replays_bit_identically():
    case = R.make_case("elu3_nobias_33")
    pa, st, pl, index = build(case)
    buf = torch.zeros_like(index)
    pl.backward(st, buf, adv_stats=pl.adv_stats)                     # (the workspace and every .grad exist before the capture)
    g, rewind = capture(lambda: pl.backward(st, buf, adv_stats=pl.adv_stats), pl.written())
    buf.copy_(index)
    g.replay()
    torch.cuda.synchronize()
    replayed, rstats = grads_of(pl), host(pl.stats)
    for p in pl.parameters():
        p.grad.zero_()
    eager, estats = run(pl, st, index)
    assert all(np.array_equal(replayed[k], eager[k]) for k in eager) and np.array_equal(rstats, estats)
    assert np.abs(eager["actor.0.weight"]).max() > 0 and estats[6] == case["M"]


# ---------------------------------------------------------------------------- (9) the library's own checks
def test_calls_are_rejected_with_a_message_and_launch_nothing():
    from tsid_control_amd import _lib
    case = R.make_case("tanh_relu_17")
    pa, st, pl, index = build(case)
    env = pa.env
    wc = env.wc
    pl.backward(st, index, adv_stats=pl.adv_stats)
    torch.cuda.synchronize()
    batch, ag, cg = pl._last
    a, c = pa.actor_net.struct, pa.critic_net.struct
    for p in pl.parameters():
        p.grad.fill_(-77.0)
    pl.stats.fill_(-77.0)
    pl.workspace.fill_(-77.0)
    cfg = pl._cfg

    def copy(s, **kw):
        o = type(s).from_buffer_copy(s)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(o, k)[v[0]] = v[1]
            else:
                setattr(o, k, v)
        return o
    vp = lambda t: C.c_void_p(t.data_ptr())
    base = dict(actor=a, critic=c, batch=batch, ag=ag, cg=cg, log_std=vp(pa.log_std), log_std_grad=vp(pa.log_std.grad), cfg=cfg,
                ws=vp(pl.workspace), ws_bytes=pl.workspace.numel() * 4, stats=vp(pl.stats))

    def call(**kw):
        k = dict(base, **kw)
        ref = lambda s: C.byref(s) if s is not None else None
        wc._call("tsidb_policy_learn", ref(k["actor"]), ref(k["critic"]), ref(k["batch"]), ref(k["ag"]), ref(k["cg"]), k["log_std"],
                 k["log_std_grad"], ref(k["cfg"]), k["ws"], C.c_size_t(k["ws_bytes"]), k["stats"], wc._stream())
    NA = env.NA
    bad = [
        (dict(actor=None), "null actor"), (dict(batch=None), "null batch"), (dict(ag=None), "null actor_grads"), (dict(cg=None), "null critic_grads"),
        (dict(cfg=None), "null cfg"), (dict(log_std=None), "null log_std"), (dict(log_std_grad=None), "null log_std"), (dict(stats=None), "null stats"),
        (dict(ws=None), "null workspace"), (dict(batch=copy(batch, index=None)), "null index"),
        (dict(batch=copy(batch, M=0)), "M must be >= 1"), (dict(batch=copy(batch, rows=0)), "rows must be >= 1"),
        (dict(cfg=copy(cfg, clip=0.0)), "clip must be > 0"), (dict(cfg=copy(cfg, clip=-0.2)), "clip must be > 0"),
        (dict(batch=copy(batch, action=None)), "null stored array"), (dict(batch=copy(batch, advantage=None)), "null stored array"),
        (dict(batch=copy(batch, critic_input=None)), "a critic needs critic_input, value and returns"),
        (dict(batch=copy(batch, value=None)), "a critic needs"), (dict(batch=copy(batch, returns=None)), "a critic needs"),
        (dict(ws_bytes=pl._ws_bytes - 4), "workspace of"),
        (dict(actor=copy(a, n_layers=5)), "actor: n_layers"), (dict(critic=copy(c, n_layers=0)), "critic: n_layers"),
        (dict(actor=copy(a, n_blocks=0)), "actor: n_blocks"), (dict(actor=copy(a, width=(0, 513))), "actor: width"),
        (dict(actor=copy(a, block_cols=(0, 513))), "actor: block_cols"), (dict(actor=copy(a, weight=(1, None))), "actor: null weight"),
        (dict(actor=copy(a, activation=3)), "actor: unknown activation"), (dict(actor=copy(a, width=(1, NA + 1))), "actor: the last width must be NA"),
        (dict(critic=copy(c, width=(1, 2))), "critic: the last width must be 1"),
        (dict(ag=copy(ag, weight=(0, None))), "actor: null weight gradient"), (dict(cg=copy(cg, bias=(1, None))), "critic: null bias gradient"),
    ]
    for kw, msg in bad:
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_learn: .*" + msg):
            call(**kw)
        assert wc._L.tsidb_last_error(wc._h).decode().startswith("tsidb_policy_learn: ")
    n = C.c_size_t(0)
    for args, msg in (((None, None, 4, C.byref(n)), "null actor"), ((C.byref(a), None, 0, C.byref(n)), "M must be >= 1"),
                      ((C.byref(a), None, 4, None), "null bytes"), ((C.byref(copy(a, n_layers=9)), None, 4, C.byref(n)), "actor: n_layers")):
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_learn_workspace: " + msg):
            wc._call("tsidb_policy_learn_workspace", *args)
    torch.cuda.synchronize()
    assert all(bool((p.grad == -77.0).all()) for p in pl.parameters()) and bool((pl.stats == -77.0).all()) and bool((pl.workspace == -77.0).all())
    # the block pointers and strides are not the learner's business; the policy gradient alone is a call; the workspace grows with M
    call(actor=copy(a, block=(0, None), block_ld=(0, 0)))
    torch.cuda.synchronize()
    want = grads_of(pl)
    assert np.isfinite(want["actor.0.weight"]).all() and float(pl.stats[6]) == case["M"]
    critic_grad = pa.critic_net.layers[0][0].grad
    critic_grad.fill_(-77.0)
    call(critic=None, cg=None)
    torch.cuda.synchronize()
    assert bool((critic_grad == -77.0).all()) and float(pl.stats[1]) == 0 and np.array_equal(host(pa.actor_net.layers[0][0].grad), want["actor.0.weight"])
    sizes = []
    for M in (1, 16, 17, R.SEG_ROWS, R.SEG_ROWS + 1):
        wc._call("tsidb_policy_learn_workspace", C.byref(a), C.byref(c), M, C.byref(n))
        sizes.append(n.value)
    assert sizes[0] == sizes[1] < sizes[2] < sizes[3] < sizes[4] and sizes[0] % 4 == 0
