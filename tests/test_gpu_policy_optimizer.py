"""The policy optimiser on the device (tsidb_policy_opt_step, PolicyOptimizer) against the float64 restatement
tests/policy_optimizer_reference.py.  The yardstick of parameters and moments is torch's CPU float32 clip_grad_norm_ + Adam on
the same case, E = e32(case) after as many steps, computed here: the device passes when max|x_dev - x64| <= 8 max(E, 2^-22)
max|x64| per tensor.  The 8 is the learner's, for the same reason: a different but fixed operation order and an ulp or two in
sqrt and the division.  With lr = 1e-2 a wrong-signed or missing update is three orders of magnitude outside that gate.
The norm and the clip factor: 2^-22 relative (float32 squares are exact in float64, the float64 sum of under a million terms
errs below 1e-9, one cast follows).  The KL, formed in float64: 1e-12 relative to max(1, |kl|), on the float64 value the call
leaves in its workspace; stats[2] is its float32 cast.  lr, its direction and the step count: exact."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_optimizer_reference as R  # noqa: E402
from policy_testlib import capture, host  # noqa: E402
from test_gpu_policy_learner import N, build, env_of, padded  # noqa: E402
from test_policy_optimizer_reference import case_of, e32, torch_run  # noqa: E402

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -22


def setup(name, **kw):
    """(case, the restatement's steps, PolicyActor, RolloutStorage, PolicyLearner, index, PolicyOptimizer) of a case on the
    device, behind one backward(): the workspace and every .grad exist.  The stored means sit in a NaN-filled allocation and
    are NaN in every row the index does not name."""
    from tsid_control_amd import PolicyOptimizer
    case, ref = case_of(name)
    pa, st, pl, index = build(case)
    o, T = case["opt"], case["rows"] // N
    big, view = padded((T, N, case["na"]), torch.float32, index.device)
    view.copy_(torch.from_numpy(o["mean"]).reshape(T, N, -1))
    st.mean = view
    st._keep.append(big)
    pl.backward(st, index, adv_stats=pl.adv_stats)
    cfg = o["cfg"]
    args = dict(lr=o["lr"], betas=(cfg["b1"], cfg["b2"]), eps=cfg["eps"], max_grad_norm=cfg["max_norm"], desired_kl=cfg["desired_kl"],
                lr_min=cfg["lr_min"], lr_max=cfg["lr_max"], skip_nonfinite=cfg["skip_nonfinite"])
    args.update(kw)
    opt = PolicyOptimizer(pl, **args)
    opt.log_std_old.copy_(torch.from_numpy(o["log_std_old"]))
    return case, ref, pa, st, pl, index, opt


def load(pl, case, k):
    """the gradients of step k into .grad and its mu into the learner's workspace"""
    o = case["opt"]
    for p, g in zip(pl.parameters(), o["grads"][k]):
        p.grad.copy_(torch.from_numpy(g).reshape(p.shape))
    if o["mu"][k] is not None:
        pl.workspace[:case["M"] * case["na"]].copy_(torch.from_numpy(o["mu"][k]).reshape(-1))


def snap(opt):
    return [t.detach().clone() for t in opt.parameters() + [opt.moments, opt.lr, opt.step_count]]


def rewind(opt, saved):
    with torch.no_grad():
        for t, s in zip(opt.parameters() + [opt.moments, opt.lr, opt.step_count], saved):
            t.copy_(s)


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def gate_ratio(case, state, opt, E, what):
    """the largest error / gate over parameters, exp_avg and exp_avg_sq against the restatement's state, each tensor printed"""
    worst = 0.0
    for key, get in (("params", lambda p: p), ("exp_avg", opt.exp_avg), ("exp_avg_sq", opt.exp_avg_sq)):
        for (pname, _), p, want in zip(R.param_list(case), opt.parameters(), state[key]):
            got = host(get(p)).astype(np.float64)
            assert got.shape == want.shape and np.isfinite(got).all(), (key, pname)
            ratio = float(np.abs(got - want).max() / (8 * max(E, FLOOR) * np.abs(want).max()))
            print(f"{case['name']} {what} {key} {pname}: error / gate {ratio:.3f}")
            worst = max(worst, ratio)
    print(f"{case['name']} {what}: E = {E:.2e}, largest error / gate {worst:.3f}")
    return worst


# ---------------------------------------------------------------------------- (1) five steps against the float64 reference
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_five_steps_match_the_float64_reference(name):
    """every case of policy_optimizer_reference.CASES: tanh_relu_17 (every piece smaller than a chunk, ragged tails, one KL
    segment), wide_no_critic (a 262144-element piece of 256 chunks, chunk boundaries inside and between pieces, no critic),
    segments (two KL segments, the second ragged) and segments_bad (two bad indices), v0_single_row (NA = 18: pieces whose
    moments are not 16-byte aligned; M = 1), elu3_nobias_33 (a layer without bias: a missing piece), no_schedule_no_clip
    (max_grad_norm = 0, desired_kl = None: no KL inputs in the call, coef = 1, kl = 0).  Clipping is active in steps 2, 4, 5;
    lr goes up, is held by lr_max, stays, goes down, is held by lr_min.  .grad keeps its bits.
    Measured (MI355X), E after 5 steps and the largest error / gate after 1 / 5 steps: tanh_relu_17 1.43e-7, 0.050 / 0.080;
    wide_no_critic 2.50e-6, 0.063 / 0.009; segments 1.50e-7, 0.055 / 0.093; segments_bad 3.47e-7, 0.061 / 0.205; v0_single_row
    1.48e-7, 0.039 / 0.089; elu3_nobias_33 1.55e-7, 0.057 / 0.081; no_schedule_no_clip 1.50e-7, 0.057 / 0.078; the float64 KL
    within 2.7e-16 of the restatement throughout ("Policy optimiser")."""
    case, ref, pa, st, pl, index, opt = setup(name)
    o = case["opt"]
    cfg = o["cfg"]
    E = e32(name)
    worst = {}
    for k in range(R.STEPS):
        load(pl, case, k)
        before = [p.grad.clone() for p in pl.parameters()]
        log_std = host(pa.log_std)
        s = host(opt.step())
        n64 = host(opt.norm_kl64())
        state, want = ref[k]
        assert all(torch.equal(p.grad.view(torch.int32), b.view(torch.int32)) for p, b in zip(pl.parameters(), before)), k
        print(f"{name} step {k + 1}: stats {s.tolist()}, float64 norm {n64[0]!r} kl {n64[1]!r}, reference {want.tolist()}")
        assert abs(s[0] - want[0]) <= FLOOR * want[0] and abs(s[1] - want[1]) <= FLOOR * want[1], k
        assert abs(n64[0] - want[0]) <= 1e-12 * want[0]
        if cfg["desired_kl"]:
            kl = R.kl_of(o["mu"][k], o["mean"], case["index"], case["rows"], log_std, o["log_std_old"])[0]
            assert abs(kl - want[2]) <= 1e-4 * want[2]                   # (the device's log_std is the restatement's to float32)
            print(f"{name} step {k + 1}: kl error {abs(n64[1] - kl) / max(1.0, abs(kl)):.2e}")
            assert abs(n64[1] - kl) <= 1e-12 * max(1.0, abs(kl)), k
            assert s[2] == np.float32(n64[1])
        else:
            assert s[2] == 0 and n64[1] == 0 and s[1] == 1.0
        assert s[3] == want[3] == float(host(opt.lr)[0]) and s[3] == np.float32(state["lr"]), (k, s[3], want[3])
        assert list(s[4:]) == [k + 1, 0, want[6], want[7]] and int(opt.step_count) == k + 1, k
        if k + 1 in (1, R.STEPS):
            worst[k + 1] = gate_ratio(case, state, opt, E[k + 1], f"after {k + 1}")
    assert worst[1] <= 1.0 and worst[R.STEPS] <= 1.0


# ---------------------------------------------------------------------------- (2) bits: two calls, a captured step
def test_two_calls_from_the_same_state_and_a_captured_step_write_the_same_bits():
    case, ref, pa, st, pl, index, opt = setup("segments")
    load(pl, case, 1)
    start = snap(opt)
    s1 = opt.step().clone()
    first = snap(opt)
    assert not same_bits(start[:-1], first[:-1]) and float(s1[1]) < 1.0 and float(s1[7]) == 1.0
    rewind(opt, start)
    opt.stats.fill_(-1.0)
    opt.workspace.fill_(-1.0)
    s2 = opt.step().clone()
    assert same_bits(first, snap(opt)) and torch.equal(s1, s2)
    # captured: the warm-up's writes are rewound by capture(), the replay is the step
    rewind(opt, start)
    g, _ = capture(lambda: opt.step(), opt.written())
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(first, snap(opt)) and torch.equal(opt.stats, s1)
    g.replay()
    torch.cuda.synchronize()
    assert int(opt.step_count) == 2 and not same_bits(first[:-1], snap(opt)[:-1])


# ---------------------------------------------------------------------------- (3) in place
def test_the_step_is_what_the_next_backward_and_the_next_act_compute_with():
    case, ref, pa, st, pl, index, opt = setup("tanh_relu_17")
    M = case["M"]
    before = pl.outputs(M)[0].clone()
    load(pl, case, 0)
    w0 = pa.actor_net.layers[0][0].detach().clone()
    opt.step()
    assert float((pa.actor_net.layers[0][0].detach() - w0).abs().max()) > 1e-3
    pl.backward(st, index, adv_stats=pl.adv_stats)
    mu, v = pl.outputs(M)
    assert float((mu - before).abs().max()) > 1e-4
    rows = min(N, M)
    j = index.long()[:rows]
    pa.actor_net.blocks[0][:rows].copy_(st.actor_input.reshape(case["rows"], -1)[j])
    pa.critic_net.blocks[0][:rows].copy_(st.critic_input.reshape(case["rows"], -1)[j])
    out = pa.act(deterministic=True)
    torch.cuda.synchronize()
    assert torch.equal(out["mean"][:rows], mu[:rows]) and torch.equal(out["value"][:rows], v[:rows])


# ---------------------------------------------------------------------------- (4) the skip
def test_a_nonfinite_gradient_skips_the_step_or_poisons_it_as_torchs_does():
    case, ref, pa, st, pl, index, opt = setup("tanh_relu_17")
    load(pl, case, 0)
    opt.step()
    load(pl, case, 1)
    start = snap(opt)
    want_stats = opt.step().clone()
    want = snap(opt)
    rewind(opt, start)
    spot = pl.parameters()[2].grad.view(-1)
    keep = float(spot[5])
    spot[5] = float("inf")
    s = host(opt.step())
    assert same_bits(start, snap(opt)) and s[5] == 1 and np.isinf(s[0]) and s[4] == 1 and s[7] == 0 and s[3] == float(start[-2])
    spot[5] = keep
    s = opt.step()
    assert same_bits(want, snap(opt)) and torch.equal(s, want_stats) and float(s[5]) == 0
    # a NaN in the KL's inputs skips as well
    load(pl, case, 2)
    start = snap(opt)
    pl.workspace[3] = float("nan")
    s = host(opt.step())
    assert same_bits(start, snap(opt)) and s[5] == 1 and np.isnan(s[2]) and np.isfinite(s[0])
    # skip_nonfinite = False: torch's arithmetic - the clip factor is 0, 0 * inf = NaN in that element alone
    case, ref, pa, st, pl, index, opt = setup("tanh_relu_17", skip_nonfinite=False, desired_kl=None)
    load(pl, case, 0)
    pl.parameters()[2].grad.view(-1)[5] = float("inf")
    start = snap(opt)
    s = host(opt.step())
    assert s[5] == 0 and s[4] == 1 and np.isinf(s[0]) and s[1] == 0
    grads = [g.copy() for g in case["opt"]["grads"][0]]
    grads[2].reshape(-1)[5] = np.inf
    t32 = torch_run(dict(case, opt=dict(case["opt"], grads=[grads])), torch.float32, [case["opt"]["lr"]], steps=1)[0]
    for i, (p, p0, tp) in enumerate(zip(opt.parameters(), start, t32["params"])):
        got = host(p)
        assert np.array_equal(np.isnan(got), np.isnan(tp)) and np.isnan(got).sum() == (i == 2), i
        assert np.array_equal(np.nan_to_num(got), np.nan_to_num(tp.astype(np.float32))) and np.array_equal(np.nan_to_num(got), np.nan_to_num(host(p0)) * ~np.isnan(got))


# ---------------------------------------------------------------------------- (5) update() on a real rollout
def test_update_with_a_policy_optimizer_is_the_hand_driven_loop_on_a_real_rollout():
    """17 envs x 4 steps.  update(storage, PolicyOptimizer) against snapshot() / backward() / step() by hand from the same
    weights and the same generator seed: bit for bit.  With untouched weights the first minibatch has mu == mean bit for bit
    (the learner's forward pass is the actor's) and log_std == log_std_old, so every term of kl_m is s - s + (e + 0) / (2 e')
    - 1/2 with e' = e: exactly 0 - the bound is 0, and lr does not move (0 < kl fails)."""
    from tsid_control_amd import PolicyLearner, PolicyOptimizer
    from test_gpu_policy_actor import small_actor
    n, T = 17, 4
    env = env_of(False, n)
    pa = small_actor(env, seed=5)[0]
    st = env.rollout(pa, T)
    st.gae()
    pl = PolicyLearner(pa)
    start = [p.detach().clone() for p in pl.parameters()]
    runs = []
    for by_hand in (False, True):
        with torch.no_grad():
            for p, s in zip(pl.parameters(), start):
                p.copy_(s)
        opt = PolicyOptimizer(pl, lr=1e-3, desired_kl=0.01)
        opt.log_std_old.fill_(7.0)                                   # (snapshot() must overwrite it)
        opt.log = torch.zeros(6, 8, dtype=torch.float32, device=env.device)
        gen = torch.Generator(device=env.device).manual_seed(11)
        if not by_hand:
            stats = pl.update(st, opt, epochs=2, minibatches=3, generator=gen).clone()
        else:
            pl.fill_adv_stats(st)
            opt.snapshot()
            mine, rows = [], n * T
            for ep in range(2):
                perm = torch.randperm(rows, generator=gen, dtype=torch.int32, device=env.device)
                for k in range(3):
                    mine.append(pl.backward(st, perm[k * rows // 3:(k + 1) * rows // 3].contiguous(), adv_stats=pl.adv_stats).clone())
                    opt.step()
            stats = torch.stack(mine)
        torch.cuda.synchronize()
        runs.append((stats, snap(opt), opt.log.clone(), opt.log_std_old.clone()))
    (s0, a, log0, old0), (s1, b, log1, old1) = runs
    assert torch.equal(s0, s1) and same_bits(a, b) and torch.equal(log0, log1) and bool(torch.isfinite(s0).all())
    assert torch.equal(old0, start[-1]) and torch.equal(old1, start[-1])
    log = host(log0)
    print("kl", log[:, 2].tolist(), "lr", log[:, 3].tolist(), "norm", log[:, 0].tolist())
    assert log[0, 2] == 0.0 and log[0, 7] == 0 and log[0, 3] == np.float32(1e-3)
    assert list(log[:, 4]) == [1, 2, 3, 4, 5, 6] and not log[:, 5].any() and (log[1:, 2] > 0).all() and list(log[:, 6]) == [22, 23, 23] * 2
    assert any(not torch.equal(p, s) for p, s in zip(pl.parameters(), start)) and int(a[-1]) == 6


# ---------------------------------------------------------------------------- (6) checkpoints
def test_a_checkpoint_moves_to_torch_adam_and_back():
    """after two steps: state_dict() into torch.optim.Adam(learner.parameters()) on the device, one more step of each on the
    same .grad (no clipping: torch's step has none) - torch's lands inside the gate of this class's own; then torch's
    state_dict() into a fresh PolicyOptimizer, one more step of each likewise"""
    from tsid_control_amd import PolicyOptimizer
    name = "no_schedule_no_clip"
    case, ref, pa, st, pl, index, opt = setup(name)
    E = e32(name)
    for k in range(2):
        load(pl, case, k)
        opt.step()
    params = pl.parameters()
    twin = torch.optim.Adam(params, lr=123.0)
    twin.load_state_dict(opt.state_dict())
    assert twin.param_groups[0]["lr"] == float(np.float32(R.LR))
    for k, (mine, theirs) in ((2, (opt, twin)), (3, (None, twin))):
        if mine is None:
            mine = PolicyOptimizer(pl, max_grad_norm=None)
            mine.load_state_dict(twin.state_dict())
            assert int(mine.step_count) == k and float(mine.lr) == float(np.float32(R.LR))
        load(pl, case, k)
        start = [p.detach().clone() for p in params]
        mine.step()
        ours = [p.detach().clone() for p in params]
        with torch.no_grad():
            for p, s in zip(params, start):
                p.copy_(s)
        theirs.step()
        torch.cuda.synchronize()
        state, _ = ref[k]
        for (pname, _), p, o, want in zip(R.param_list(case), params, ours, state["params"]):
            gate = 8 * max(E[k + 1], FLOOR) * np.abs(want).max()
            assert np.abs(host(p).astype(np.float64) - host(o)).max() <= gate and np.abs(host(o) - want).max() <= gate, (k, pname)
        assert float(twin.state[params[0]]["step"]) == k + 1 == int(mine.step_count)


# ---------------------------------------------------------------------------- (7) update() with a torch optimiser is untouched
def test_update_with_torch_adam_does_not_see_the_new_module():
    """two updates with torch.optim.Adam from the same weights and seed: one with tsid_control_amd.policy_optimizer absent from
    sys.modules - update() does not import it - one with it imported and a PolicyOptimizer built on the learner: the same bits"""
    case, ref, pa, st, pl, index, _ = setup("tanh_relu_17")
    params = pl.parameters()
    start = [p.detach().clone() for p in params]
    runs = []
    for with_module in (False, True):
        with torch.no_grad():
            for p, s in zip(params, start):
                p.copy_(s)
        if with_module:
            from tsid_control_amd import PolicyOptimizer
            PolicyOptimizer(pl, desired_kl=0.01)
        else:
            saved = sys.modules.pop("tsid_control_amd.policy_optimizer", None)
        adam = torch.optim.Adam(params, lr=1e-3)
        gen = torch.Generator(device=index.device).manual_seed(5)
        stats = pl.update(st, adam, epochs=2, minibatches=3, generator=gen).clone()
        torch.cuda.synchronize()
        if not with_module:
            assert "tsid_control_amd.policy_optimizer" not in sys.modules
            if saved is not None:
                sys.modules["tsid_control_amd.policy_optimizer"] = saved
        runs.append((stats, [p.detach().clone() for p in params]))
    assert torch.equal(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]) and not same_bits(start, runs[0][1])


# ---------------------------------------------------------------------------- (8) the library's own checks
def test_calls_are_rejected_with_a_message_and_launch_nothing():
    from tsid_control_amd import _lib
    case, ref, pa, st, pl, index, opt = setup("tanh_relu_17")
    wc = pa.env.wc
    load(pl, case, 0)
    opt.step()
    torch.cuda.synchronize()
    ag, cg, state, kl = opt._last
    a, c, cfg = pa.actor_net.struct, pa.critic_net.struct, opt._cfg
    start = snap(opt)
    opt.stats.fill_(-77.0)
    opt.workspace.fill_(-77.0)

    def copy(s, **kw):
        o = type(s).from_buffer_copy(s)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(o, k)[v[0]] = v[1]
            else:
                setattr(o, k, v)
        return o
    vp = lambda t: C.c_void_p(t.data_ptr())
    base = dict(actor=a, critic=c, ag=ag, cg=cg, log_std=vp(pa.log_std), log_std_grad=vp(pa.log_std.grad), cfg=cfg, state=state, kl=kl,
                ws=vp(opt.workspace), ws_bytes=opt.workspace.numel() * 8)

    def call(**kw):
        k = dict(base, **kw)
        ref_ = lambda s: C.byref(s) if s is not None else None
        wc._call("tsidb_policy_opt_step", ref_(k["actor"]), ref_(k["critic"]), ref_(k["ag"]), ref_(k["cg"]), k["log_std"], k["log_std_grad"],
                 ref_(k["cfg"]), ref_(k["state"]), ref_(k["kl"]), k["ws"], C.c_size_t(k["ws_bytes"]), wc._stream())
    NA = pa.env.NA
    nan = float("nan")
    bad = [
        (dict(actor=None), "null actor"), (dict(ag=None), "null actor_grads"), (dict(cg=None), "null critic_grads"), (dict(cfg=None), "null cfg"),
        (dict(state=None), "null state"), (dict(log_std=None), "null log_std"), (dict(log_std_grad=None), "null log_std"), (dict(ws=None), "null workspace"),
        (dict(state=copy(state, moments=None)), "null state pointer"), (dict(state=copy(state, lr=None)), "null state pointer"),
        (dict(state=copy(state, step=None)), "null state pointer"), (dict(state=copy(state, stats=None)), "null state pointer"),
        (dict(cfg=copy(cfg, b1=1.0)), "b1 and b2 must be in \\[0, 1\\)"), (dict(cfg=copy(cfg, b2=-0.1)), "b1 and b2"), (dict(cfg=copy(cfg, b1=nan)), "b1 and b2"),
        (dict(cfg=copy(cfg, eps=0.0)), "eps must be > 0"), (dict(cfg=copy(cfg, eps=-1e-8)), "eps must be > 0"),
        (dict(cfg=copy(cfg, max_norm=-1.0)), "max_norm must be >= 0"), (dict(cfg=copy(cfg, desired_kl=-0.01)), "desired_kl must be >= 0"),
        (dict(cfg=copy(cfg, lr_min=0.0)), "lr_min must be > 0 and <= lr_max"), (dict(cfg=copy(cfg, lr_min=0.5, lr_max=0.1)), "lr_min must be > 0 and <= lr_max"),
        (dict(kl=None), "the schedule needs kl"), (dict(kl=copy(kl, mean=None)), "the schedule needs kl"), (dict(kl=copy(kl, index=None)), "the schedule needs kl"),
        (dict(kl=copy(kl, mu=None)), "the schedule needs kl"), (dict(state=copy(state, log_std_old=None)), "the schedule needs kl .* and log_std_old"),
        (dict(kl=copy(kl, M=0)), "M must be >= 1"), (dict(kl=copy(kl, rows=0)), "rows must be >= 1"),
        (dict(ws_bytes=opt._ws_bytes - 8), "workspace of"),
        (dict(actor=copy(a, n_layers=5)), "actor: n_layers"), (dict(critic=copy(c, n_layers=0)), "critic: n_layers"),
        (dict(actor=copy(a, n_blocks=0)), "actor: n_blocks"), (dict(actor=copy(a, width=(0, 513))), "actor: width"),
        (dict(actor=copy(a, weight=(1, None))), "actor: null weight"), (dict(actor=copy(a, activation=3)), "actor: unknown activation"),
        (dict(actor=copy(a, width=(1, NA + 1))), "actor: the last width must be NA"), (dict(critic=copy(c, width=(1, 2))), "critic: the last width must be 1"),
        (dict(ag=copy(ag, weight=(0, None))), "actor: null weight gradient"), (dict(cg=copy(cg, bias=(1, None))), "critic: null bias gradient"),
    ]
    for kw, msg in bad:
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_opt_step: .*" + msg):
            call(**kw)
        assert wc._L.tsidb_last_error(wc._h).decode().startswith("tsidb_policy_opt_step: ")
    n = C.c_size_t(0)
    for args, msg in (((None, None, 4, C.byref(n)), "null actor"), ((C.byref(a), None, -1, C.byref(n)), "M must be >= 0"),
                      ((C.byref(a), None, 4, None), "null bytes"), ((C.byref(copy(a, n_layers=9)), None, 4, C.byref(n)), "actor: n_layers")):
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_opt_workspace: " + msg):
            wc._call("tsidb_policy_opt_workspace", *args)
    torch.cuda.synchronize()
    assert same_bits(start, snap(opt)) and bool((opt.stats == -77.0).all()) and bool((opt.workspace == -77.0).all())
    # the workspace: 8 bytes per chunk of every piece, 16 per KL segment, 32 for the scalars; without the schedule no KL inputs
    sizes = []
    for M in (0, 1, R.SEG_ROWS, R.SEG_ROWS + 1):
        wc._call("tsidb_policy_opt_workspace", C.byref(a), C.byref(c), M, C.byref(n))
        sizes.append(n.value)
    chunks = sum(-(-p.numel() // R.CHUNK) for p in pl.parameters())
    assert sizes == [8 * chunks + 32, 8 * chunks + 48, 8 * chunks + 48, 8 * chunks + 64]
    load(pl, case, 1)
    call(cfg=copy(cfg, desired_kl=0.0), kl=None, state=copy(state, log_std_old=None), ws_bytes=sizes[0])
    torch.cuda.synchronize()
    s = host(opt.stats)
    assert s[2] == 0 and s[4] == 2 and s[5] == 0 and s[6] == 0 and s[7] == 0 and 0 < s[1] < 1 and not same_bits(start, snap(opt))
