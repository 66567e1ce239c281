"""Imitation of the TSID teacher on the device (tsidb_policy_teacher_mix, tsidb_policy_learn_imit; RolloutStorage(teacher=True),
PolicyEnv.rollout(teacher_beta=...), PolicyLearner(imitation_coef=...)) against the float64 restatement
tests/policy_imitation_reference.py.  The gradients' gate is the learner's own (tests/test_gpu_policy_learner.py): max|g_dev - g64|
<= 8 max(E, 2^-22) max|g64| per parameter tensor with E = e32(case), the error of torch's CPU float32 autograd of the extended
loss on the same case; stats 0 .. 5 and imit_stats 0 .. 1 likewise relative to max(1, |ref|); every count exact.  The mix kernel
and the rollouts are held to bits."""
import ctypes as C
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_imitation_reference as RI  # noqa: E402
from policy_testlib import capture, conf_of, host, make_env, same  # noqa: E402
from test_gpu_policy_learner import N, build, gate_ratio, grads_of, padded, run  # noqa: E402
from test_policy_imitation_reference import e32  # noqa: E402

pytestmark = pytest.mark.gpu


def build_imit(case, **kw):
    """test_gpu_policy_learner.build of the case with the term's settings, and the three teacher tensors of the storage as views
    into NaN-filled (the flags: -1-filled) allocations"""
    kw = dict(dict(imitation_coef=case["imitation_coef"], surrogate_coef=case["surrogate_coef"], imitation_loss=case["imit_loss"]), **kw)
    pa, st, pl, index = build(case, **kw)
    dev, T, na = index.device, case["rows"] // N, case["na"]
    for name, key, shape, dtype in (("teacher_action", "target", (T, N, na), torch.float32), ("teacher_weight", "weight", (T, N), torch.float32),
                                    ("teacher_executed", "skip", (T, N), torch.int32)):
        if case[key] is None:
            setattr(st, name, None)
            continue
        big, view = padded(shape, dtype, dev)
        view.copy_(torch.from_numpy(case[key]).reshape(shape))
        setattr(st, name, view)
        st._keep.append(big)
    return pa, st, pl, index


def imit_gate(case, pl, got, stats, ev=None, E=None):
    """gate_ratio of the learner's test on the extended reference, then imit_stats: 0 and 1 in the same gate, the counts exact"""
    ev = RI.evaluate(case) if ev is None else ev
    E = max(e32(case) if E is None else E, 2.0 ** -22)
    worst, _ = gate_ratio(case, got, stats, ev=ev, E=E)
    ist = host(pl.imit_stats)
    for i in range(2):
        ratio = float(abs(ist[i] - ev["imit_stats"][i]) / (8 * E * max(1.0, abs(ev["imit_stats"][i]))))
        print(f"{case['name']} imit_stats[{i}] {RI.IMIT_STATS[i]}: error / gate {ratio:.3f}")
        worst = max(worst, ratio)
    assert list(ist[2:]) == list(ev["imit_stats"][2:]) and list(stats[6:]) == list(ev["stats"][6:])
    print(f"{case['name']}: with imit_stats, largest error / gate {worst:.3f}")
    return worst, ev


# ---------------------------------------------------------------------------- (1) gradients and stats against the restatement
@pytest.mark.parametrize("name", sorted(RI.CASES))
def test_gradients_and_stats_match_the_float64_reference(name):
    """every case of policy_imitation_reference.CASES on a synthetic storage of 33 envs: both robots; 1, 17, 33 and 512 + 17 (+ 2 bad)
    rows; MSE and Huber with |d| on both sides of 1; weights 0 (their labels NaN), 1 and fractional; executed rows; PPO with the
    term, a surrogate weight of 0.5, pure distillation with and without a critic (the 512-wide actor, whose LDS images exceed 64 KB);
    NULL weight and skip.  Measured (MI355X), E and the largest error / gate, imit_stats included: huber_17_plain 1.30e-6, 0.157;
    huber_33_nobias 1.57e-6, 0.103; huber_segments_bad 1.40e-6, 0.117; mse_17 1.34e-6, 0.148; mse_no_critic_distill 3.28e-7, 0.211;
    v0_huber_single_row 1.16e-6, 0.125; v0_mse_17_distill 3.36e-7, 0.124 (imit_stats alone: at most 0.023)."""
    case = RI.make_case(name)
    pa, st, pl, index = build_imit(case)
    got, stats = run(pl, st, index)
    worst, ev = imit_gate(case, pl, got, stats)
    assert worst <= 1.0
    assert np.isfinite(stats).all() and np.isfinite(host(pl.imit_stats)).all()
    if case["surrogate_coef"] == 0 and case["value_coef"] == 0 and case["entropy_coef"] == 0:
        assert not np.abs(got["log_std"]).max() and np.abs(got["actor.0.weight"]).max() > 0
    mu, _ = pl.outputs(len(case["index"]))
    j = case["index"][(case["index"] >= 0) & (case["index"] < case["rows"])]
    assert len(j) == len(ev["mu"])
    if len(j) == len(case["index"]):
        assert np.abs(host(mu) - ev["mu"]).max() <= 1e-4 * max(1.0, np.abs(ev["mu"]).max())


# ---------------------------------------------------------------------------- (2) the term-off path
def call_imit(pl, imit, ws, stats):
    """tsidb_policy_learn_imit on the arguments of pl's last backward(), with the given struct (None: NULL), workspace and stats"""
    pa, wc = pl.actor, pl.env.wc
    batch, ag, cg = pl._last
    wc._call("tsidb_policy_learn_imit", C.byref(pa.actor_net.struct), C.byref(pa.critic_net.struct) if pa.critic_net is not None else None,
             C.byref(batch), C.byref(ag), C.byref(cg) if cg is not None else None, C.c_void_p(pa.log_std.data_ptr()),
             C.c_void_p(pa.log_std.grad.data_ptr()), C.byref(pl._cfg), C.byref(imit) if imit is not None else None, C.c_void_p(ws.data_ptr()),
             C.c_size_t(ws.numel() * 4), C.c_void_p(stats.data_ptr()), wc._stream())
    torch.cuda.synchronize()


def imit_workspace(pl, M):
    pa, wc = pl.actor, pl.env.wc
    n = C.c_size_t(0)
    wc._call("tsidb_policy_learn_imit_workspace", C.byref(pa.actor_net.struct), C.byref(pa.critic_net.struct) if pa.critic_net is not None else None,
             M, C.byref(n))
    return torch.empty((n.value + 3) // 4, dtype=torch.float32, device=wc.device), n.value


def test_term_off_is_the_learners_call_bit_for_bit():
    """tsidb_policy_learn_imit with imitation_coef = 0, surrogate_coef = 1 and no skips - whatever the labels (NaN among them) and
    the weights hold -, and with a NULL struct: gradients and stats torch.equal to tsidb_policy_learn's on the same case"""
    from tsid_control_amd import _lib
    case = RI.make_case("mse_17")
    pa, st, pl, index = build_imit(case, imitation_coef=0.0, surrogate_coef=1.0)
    g0, s0 = run(pl, st, index)                                  # (the term is off: tsidb_policy_learn)
    assert np.abs(g0["actor.0.weight"]).max() > 0 and bool(torch.isnan(st.teacher_action).any())
    plain_bytes = pl._ws_bytes
    ws, nbytes = imit_workspace(pl, case["M"])
    Mp, nseg = (case["M"] + 15) // 16 * 16, 1
    assert nbytes == plain_bytes + 4 * 4 * (Mp + nseg)          # (four more floats per row and per segment)
    ist = torch.full((4,), -7.0, device=index.device)
    p = lambda t: t.data_ptr() if t is not None else None
    for weight, loss in ((st.teacher_weight, 0), (None, 1)):
        for q in pl.parameters():
            q.grad.fill_(5.0)
        stats = torch.full((8,), -7.0, device=index.device)
        imit = _lib.PolicyImit(p(st.teacher_action), p(weight), None, 0.0, 1.0, loss, p(ist))
        call_imit(pl, imit, ws, stats)
        g1 = grads_of(pl)
        assert all(torch.equal(torch.from_numpy(g0[k]), torch.from_numpy(g1[k])) for k in g0) and torch.equal(stats.cpu(), torch.from_numpy(s0))
        assert float(ist[3]) == 0 and float(ist[2]) == (float((case["weight"][case["index"]] > 0).sum()) if weight is not None else case["M"])
    # a NULL struct: the plain kernels on the plain workspace's bytes
    for q in pl.parameters():
        q.grad.fill_(5.0)
    stats = torch.full((8,), -7.0, device=index.device)
    small = torch.empty((plain_bytes + 3) // 4, dtype=torch.float32, device=index.device)
    call_imit(pl, None, small, stats)
    g2 = grads_of(pl)
    assert all(np.array_equal(g0[k], g2[k]) for k in g0) and np.array_equal(host(stats), s0)


# ---------------------------------------------------------------------------- (3) determinism
def test_two_calls_rows_outside_the_index_and_a_graph_replay_give_the_same_bits():
    """on the two-segment case with bad indices: two calls; NaN (the flags: 12345) in every stored row outside index, labels,
    weights and flags included; a captured backward() replayed"""
    case = RI.make_case("huber_segments_bad")
    pa, st, pl, index = build_imit(case)
    g1, s1 = run(pl, st, index)
    i1 = host(pl.imit_stats)
    for p in pl.parameters():
        p.grad.fill_(7.0)
    pl.imit_stats.fill_(7.0)
    g2, s2 = run(pl, st, index)
    assert all(np.array_equal(g1[k], g2[k]) for k in g1) and np.array_equal(s1, s2) and np.array_equal(i1, host(pl.imit_stats))
    assert i1[0] > 0 and i1[3] > 0 and s1[7] == 2
    unused = torch.ones(case["rows"], dtype=torch.bool, device=index.device)
    good = index[(index >= 0) & (index < case["rows"])]
    unused[good.long()] = False
    assert int(unused.sum()) > 50
    for k in ("actor_input", "critic_input", "action", "logp", "advantage", "returns", "teacher_action", "teacher_weight"):
        getattr(st, k).view(case["rows"], -1)[unused] = float("nan")
    st.value[:-1].view(-1)[unused] = float("nan")
    st.teacher_executed.view(-1)[unused] = 12345
    g3, s3 = run(pl, st, index)
    assert all(np.array_equal(g1[k], g3[k]) for k in g1) and np.array_equal(s1, s3) and np.array_equal(i1, host(pl.imit_stats))
    # captured
    buf = torch.zeros_like(index)
    g, _ = capture(lambda: pl.backward(st, buf, adv_stats=pl.adv_stats), pl.written())
    assert any(t is pl.imit_stats for t in pl.written())
    buf.copy_(index)
    g.replay()
    torch.cuda.synchronize()
    g4, s4 = grads_of(pl), host(pl.stats)
    assert all(np.array_equal(g1[k], g4[k]) for k in g1) and np.array_equal(s1, s4) and np.array_equal(i1, host(pl.imit_stats))


# ---------------------------------------------------------------------------- (4) the mix kernel against the restatement
def standing_env(n, dtype="f64", v0=False, **kw):
    kw = dict(dict(tsid="stand", mode="motor", decimation=2, action_scale=0.3, action_clip=0.8, seed=5), **kw)
    return make_env(n, conf_of(dtype, v0, closed_loop=True), **kw)


def driven(env, steps=2, key=1):
    """a few steps under small hashed torques, so that teacher_action is TSID's command on a moving robot"""
    from test_gpu_policy_tsid import hashed
    for t in range(steps):
        env.step(hashed((env.num_envs, env.NA), key + t, env, 0.2))
    torch.cuda.synchronize()
    assert float(env.teacher_action.abs().max()) > 1e-3


def mix_buffers(env):
    n, dev = env.num_envs, env.device
    return (torch.full((n, env.NA), float("nan"), dtype=torch.float32, device=dev), torch.full((n,), float("nan"), dtype=torch.float32, device=dev),
            torch.full((n,), -1, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("dtype,v0", [("f64", False), ("f64", True), ("f32", False), ("f32", True)])
def test_mix_kernel_matches_the_numpy_restatement(dtype, v0):
    """33 standing envs after two driven steps, ep_len 0 .. 2 and episodes 1 .. 4 written by hand so that every combination occurs;
    beta NULL, 0, 0.5 and 1: labels the float32 cast of teacher_action bit for bit, weights, flags, and the action equal to
    teacher_action in the path's bits where executed and untouched elsewhere; a beta changed on the device is seen by the next launch"""
    n = 33
    env = standing_env(n, dtype, v0)
    driven(env)
    env.ep_len.copy_(torch.arange(n, dtype=torch.int32) % 3)
    env.episode.copy_(1 + torch.arange(n, dtype=torch.int32) % 4)
    who = types.SimpleNamespace(seed=11, env_offset=7)
    ta = host(env.teacher_action)
    sampled = torch.randn(n, env.NA, generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(env.device, env.dtype)
    beta = torch.zeros(1, dtype=torch.float32, device=env.device)
    shares = []
    for b in (None, 0.0, 0.5, 1.0):
        label, weight, executed = mix_buffers(env)
        action = sampled.clone()
        if b is not None:
            beta.fill_(b)                                         # (a device op: no host call tells the library)
        env._teacher_mix(who, action, label, weight, executed, None if b is None else beta)
        torch.cuda.synchronize()
        want = RI.mix(ta, host(sampled), host(env.ep_len), host(env.episode), b, 11, 7)
        assert np.array_equal(host(label), want[0]) and host(label).dtype == np.float32
        assert np.array_equal(host(weight), want[1]) and np.array_equal(host(executed), want[2])
        assert np.array_equal(host(action), want[3])
        ex = host(executed) == 1
        assert np.array_equal(host(action)[ex], ta[ex]) and np.array_equal(host(action)[~ex], host(sampled)[~ex])
        assert not ex[host(env.ep_len) == 0].any()
        shares.append(int(ex.sum()))
    live = int((host(env.ep_len) > 0).sum())
    assert shares[0] == shares[1] == 0 and 0 < shares[2] < live and shares[3] == live == 22
    # labels alone: a NULL action
    label, weight, executed = mix_buffers(env)
    env._teacher_mix(who, None, label, weight, executed, beta)
    torch.cuda.synchronize()
    assert np.array_equal(host(label), ta.astype(np.float32)) and int(executed.sum()) == live
    assert torch.equal(env.teacher_action, torch.from_numpy(ta).to(env.device))


def test_mix_of_a_split_batch_draws_what_the_whole_batch_draws():
    """a 32-env launch equals two 16-env launches with env_offset 0 and 16 on the halves of its tensors"""
    whole, half = standing_env(32), standing_env(16)
    driven(whole)
    whole.ep_len.copy_(1 + torch.arange(32, dtype=torch.int32) % 2)
    whole.episode.copy_(1 + torch.arange(32, dtype=torch.int32) % 5)
    beta = torch.full((1,), 0.5, dtype=torch.float32, device=whole.device)
    sampled = torch.randn(32, whole.NA, generator=torch.Generator().manual_seed(4), dtype=torch.float64).to(whole.device)
    label, weight, executed = mix_buffers(whole)
    action = sampled.clone()
    whole._teacher_mix(types.SimpleNamespace(seed=3, env_offset=0), action, label, weight, executed, beta)
    for k in range(2):
        s = slice(16 * k, 16 * k + 16)
        half.teacher_action.copy_(whole.teacher_action[s])
        half.ep_len.copy_(whole.ep_len[s])
        half.episode.copy_(whole.episode[s])
        l2, w2, e2 = mix_buffers(half)
        a2 = sampled[s].clone()
        half._teacher_mix(types.SimpleNamespace(seed=3, env_offset=16 * k), a2, l2, w2, e2, beta)
        torch.cuda.synchronize()
        assert torch.equal(l2, label[s]) and torch.equal(w2, weight[s]) and torch.equal(e2, executed[s]) and torch.equal(a2, action[s])
    assert 0 < int(executed.sum()) < 32 and 0 < int(executed[:16].sum()) and 0 < int(executed[16:].sum())


# ---------------------------------------------------------------------------- (5) rollouts
def student(env, seed=0):
    from tsid_control_amd import PolicyActor
    torch.manual_seed(seed)
    mk = lambda k, out: torch.nn.Sequential(torch.nn.Linear(k, 32), torch.nn.ELU(), torch.nn.Linear(32, out)).to(env.device)
    return PolicyActor(env, mk(env.NOBS, env.NA), mk(env.NOBS + 4, 1), critic_inputs=("obs", "priv"),
                       log_std=torch.full((env.NA,), -1.0, device=env.device))


def rollout_env():
    return standing_env(17, max_episode_steps=4, reward_weights=dict(alive=0.2, termination=-5.0))


OLD = ("actor_input", "critic_input", "action", "mean", "logp", "value", "reward", "done", "timeout")


def test_teacher_rollout_is_the_hand_driven_loop_and_beta_zero_is_the_plain_rollout():
    """17 standing envs in motor mode, 6 steps, episodes of at most 4: a teacher rollout with beta = 0.5 is the act / mix / step
    loop by hand, bit for bit, storage and env; rows with ep_len == 0 - the first step and the step after the restarts - have
    weight 0 and are never executed, every other row has weight 1; with beta = 0, and with no beta, the sim state and every old
    storage tensor are those of a rollout into a plain storage"""
    from tsid_control_amd import RolloutStorage
    T = 6
    env, twin = rollout_env(), rollout_env()
    pa, pb = student(env), student(twin)
    st = env.rollout(pa, T, RolloutStorage(env, pa, T, teacher=True), teacher_beta=0.5)
    beta = torch.full((1,), 0.5, dtype=torch.float32, device=twin.device)
    lab, wgt, exe = (torch.zeros_like(x) for x in (st.teacher_action, st.teacher_weight, st.teacher_executed))
    lens = []
    for t in range(T):
        out = pb.act()
        assert torch.equal(out["action32"], st.action[t]) and torch.equal(out["logp"], st.logp[t])    # the policy's own sample and density
        lens.append(twin.ep_len.clone())
        sampled, teacher = pb.action.clone(), twin.teacher_action.clone()
        twin._teacher_mix(pb, pb.action, lab[t], wgt[t], exe[t], beta)
        rows = exe[t] == 1
        assert torch.equal(pb.action[rows], teacher[rows]) and torch.equal(pb.action[~rows], sampled[~rows])    # the path's bits
        assert torch.equal(lab[t], teacher.float())
        twin.step(pb.action)
        assert torch.equal(twin.reward, st.reward[t]) and torch.equal(twin.done, st.done[t])
    torch.cuda.synchronize()
    assert torch.equal(lab, st.teacher_action) and torch.equal(wgt, st.teacher_weight) and torch.equal(exe, st.teacher_executed)
    for a, b in zip(env.written(), twin.written()):
        assert same(a, b)
    lens = torch.stack(lens)
    assert bool((lens[0] == 0).all()) and int((lens == 0).sum()) >= 2 * 17 and int((lens > 0).sum()) > 17
    assert torch.equal(st.teacher_weight, (lens > 0).float()) and not bool(st.teacher_executed[lens == 0].any())
    assert 0 < int(st.teacher_executed.sum()) < int((lens > 0).sum())
    assert float(st.done.sum()) >= 17 and float(st.teacher_action.abs().max()) > 1e-3
    # beta = 0 and no beta against a plain storage
    plain_env = rollout_env()
    pc = student(plain_env)
    plain = plain_env.rollout(pc, T)
    for b in (0.0, None):
        e0 = rollout_env()
        p0 = student(e0)
        s0 = e0.rollout(p0, T, RolloutStorage(e0, p0, T, teacher=True), teacher_beta=b)
        torch.cuda.synchronize()
        assert all(torch.equal(getattr(s0, k), getattr(plain, k)) for k in OLD) and int(s0.teacher_executed.sum()) == 0
        for x, y in zip(e0.written(), plain_env.written()):
            assert same(x, y)
    assert any(not torch.equal(getattr(st, k), getattr(plain, k)) for k in ("reward", "actor_input"))      # beta = 0.5 did change the run


def test_captured_teacher_rollout_replays_bit_identically():
    from tsid_control_amd import RolloutStorage, rollout_written
    T = 6
    env, eager = rollout_env(), rollout_env()
    pa, pb = student(env), student(eager)
    st, se = RolloutStorage(env, pa, T, teacher=True), RolloutStorage(eager, pb, T, teacher=True)
    beta = torch.full((1,), 0.5, dtype=torch.float32, device=env.device)
    g, _ = capture(lambda: env.rollout(pa, T, st, teacher_beta=beta), list(env.written()) + list(rollout_written(st)))
    for b in (0.5, 1.0):                                         # the second replay: a beta a device op has changed
        beta.fill_(b)
        g.replay()
        eager.rollout(pb, T, se, teacher_beta=b)
        torch.cuda.synchronize()
        for x, y in zip(list(env.written()) + st.tensors(), list(eager.written()) + se.tensors()):
            assert same(x, y)
    assert int(st.teacher_executed.sum()) > 0


# ---------------------------------------------------------------------------- (6) it learns
def test_pure_distillation_lowers_the_imitation_loss():
    """one teacher storage of 33 envs x 8 steps collected with beta = 1, 20 full-batch pure-distillation steps with PolicyOptimizer:
    L_im falls, the actor's parameters move, log_std and the critic do not.  No ratio is asked for.  Measured (MI355X): L_im 0.01703
    -> 0.00159, ratio 0.093; 231 of the 264 rows carry a label (the first step follows reset()), all 231 executed."""
    from tsid_control_amd import PolicyLearner, PolicyOptimizer, RolloutStorage
    T = 8
    env = standing_env(33, max_episode_steps=0, action_scale=1.0, action_clip=100.0)    # (the teacher's torques pass unclipped)
    pa = student(env)
    st = env.rollout(pa, T, RolloutStorage(env, pa, T, teacher=True), teacher_beta=1.0)
    st.gae()
    pl = PolicyLearner(pa, imitation_coef=1.0, surrogate_coef=0.0, value_coef=0.0, entropy_coef=0.0)
    opt = PolicyOptimizer(pl, lr=1e-3)
    index = torch.arange(T * 33, dtype=torch.int32, device=env.device)
    start = [p.detach().clone() for p in pl.parameters()]
    losses = []
    for _ in range(20):
        pl.backward(st, index)
        losses.append(pl.imit_stats[0].clone())
        opt.step()
    pl.backward(st, index)
    losses.append(pl.imit_stats[0].clone())
    torch.cuda.synchronize()
    first, last = float(losses[0]), float(losses[-1])
    ist = host(pl.imit_stats)
    print(f"L_im {first:.5f} -> {last:.5f} after 20 steps: ratio {last / first:.3f}; rows with a label {ist[2]:.0f} of {T * 33}, executed {ist[3]:.0f}")
    assert np.isfinite(first) and first > 0 and last < first
    assert ist[2] == float(st.teacher_weight.sum()) >= 33 and ist[3] == float(st.teacher_executed.sum()) == ist[2] and host(pl.stats)[6] == T * 33
    assert not bool(st.teacher_weight[0].any())                  # (the first step follows reset(): no label yet)
    actor_params = [w for layer in pa.actor_net.layers for w in layer]
    assert all(not torch.equal(p, s) for p, s in zip(pl.parameters(), start) if any(p is q for q in actor_params))
    assert torch.equal(pa.log_std, start[-1])
    critic_params = [w for layer in pa.critic_net.layers for w in layer]
    assert all(torch.equal(p, s) for p, s in zip(pl.parameters(), start) if any(p is q for q in critic_params))


# ---------------------------------------------------------------------------- (7) the library's own checks
def test_calls_are_rejected_with_a_message_and_launch_nothing():
    from tsid_control_amd import _lib
    case = RI.make_case("mse_17")
    pa, st, pl, index = build_imit(case)
    run(pl, st, index)
    ws = pl.workspace
    for q in pl.parameters():
        q.grad.fill_(-77.0)
    pl.stats.fill_(-77.0)
    pl.imit_stats.fill_(-77.0)
    good = pl._last_imit

    def copy(**kw):
        o = _lib.PolicyImit.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    bad = [(copy(target=None), "imitation_coef > 0 needs target"), (copy(stats=None), "null imit stats"),
           (copy(imitation_coef=-1.0), "a coefficient is negative or not finite"), (copy(surrogate_coef=float("nan")), "a coefficient is negative or not finite"),
           (copy(imitation_coef=float("inf")), "a coefficient is negative or not finite"), (copy(loss=2), "unknown loss"), (copy(loss=-1), "unknown loss")]
    for imit, msg in bad:
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_learn_imit: " + msg):
            call_imit(pl, imit, ws, pl.stats)
    with pytest.raises(_lib.TsidbError, match="tsidb_policy_learn_imit: workspace of"):           # the plain query's bytes are too few
        call_imit(pl, good, torch.empty((ws.numel() * 4 - 16 * 4) // 4, dtype=torch.float32, device=ws.device), pl.stats)
    with pytest.raises(_lib.TsidbError, match="tsidb_policy_learn_imit: null stats"):             # what tsidb_policy_learn rejects
        call_imit(pl, good, ws, types.SimpleNamespace(data_ptr=lambda: None))
    torch.cuda.synchronize()
    assert all(bool((q.grad == -77.0).all()) for q in pl.parameters()) and bool((pl.stats == -77.0).all()) and bool((pl.imit_stats == -77.0).all())
    # the mix entry
    env = standing_env(4)
    who = types.SimpleNamespace(seed=1, env_offset=0)
    label, weight, executed = mix_buffers(env)
    action = torch.zeros(4, env.NA, dtype=env.dtype, device=env.device)
    for args, msg in (((who, action, None, weight, executed, None), "null buffer"), ((who, action, label, None, executed, None), "null buffer"),
                      ((who, action, label, weight, None, None), "null buffer"),
                      ((types.SimpleNamespace(seed=2 ** 32, env_offset=0), action, label, weight, executed, None), "seed must be below 2\\^32"),
                      ((types.SimpleNamespace(seed=1, env_offset=2 ** 31), action, label, weight, executed, None), "env_offset below 2\\^31")):
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_teacher_mix: .*" + msg):
            env._teacher_mix(*args)
    keep, env.teacher_action = env.teacher_action, None
    with pytest.raises(_lib.TsidbError, match="tsidb_policy_teacher_mix: null buffer"):
        env._teacher_mix(who, action, label, weight, executed, None)
    env.teacher_action = keep
    with pytest.raises(_lib.TsidbError, match="tsidb_policy_teacher_mix: null buffer in tsidb_policy_bufs"):
        env.wc._call("tsidb_policy_teacher_mix", None, C.c_void_p(keep.data_ptr()), None, C.c_void_p(label.data_ptr()), C.c_void_p(weight.data_ptr()),
                     C.c_void_p(executed.data_ptr()), None, C.c_uint64(0), C.c_uint64(0), env.wc._stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(label).all()) and bool(torch.isnan(weight).all()) and bool((executed == -1).all())
