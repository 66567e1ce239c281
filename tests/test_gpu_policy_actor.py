"""The policy actor on the device (tsidb_policy_actor / tsidb_policy_gae, PolicyActor, PolicyEnv.rollout) against the numpy
restatement tests/policy_actor_reference.py and its forward error bound: the kernel on the env's own buffers, the draws, the
parameters in place, a rollout against the hand-driven loop, the advantages, a captured rollout, and the library's own checks."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_actor_reference as R  # noqa: E402
from policy_testlib import capture, conf_of, host, make_env, same  # noqa: E402
from test_gpu_policy_dr import CMD, DR, driven  # noqa: E402
from test_gpu_policy_env import ALL_WEIGHTS  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ACT = {"elu": torch.nn.ELU, "tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}
SCAN = dict(scan_x=(-0.5, 0.5, 11), scan_y=(-0.3, 0.3, 7))


def torch_net(layers, act, device="cuda:0"):
    """the numpy layers as a torch.nn.Sequential on the device"""
    mods = []
    for i, (w, b) in enumerate(layers):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
        mods.append(lin)
        if i + 1 < len(layers):
            mods.append(ACT[act]())
    return torch.nn.Sequential(*mods).to(device)


def nets_for(env, rng, actor="tanh3", critic="relu_critic"):
    """(actor layers, critic layers, PolicyActor kwargs) of two named cases on env"""
    cases = R.network_cases(env.NA)
    out = []
    for name in (actor, critic):
        blocks, widths, act = cases[name]
        out.append((tuple(b for b, _ in blocks), R.make_layers(rng, sum(c for _, c in blocks), widths), act))
    return out


def small_actor(env, seed=0, critic=True, **kw):
    from tsid_control_amd import PolicyActor
    rng = np.random.default_rng(seed)
    (ai, al, aa), (ci, cl, ca) = nets_for(env, rng)
    ls = torch.from_numpy(rng.uniform(-1.5, 0.0, env.NA).astype(np.float32)).to(env.device)
    pa = PolicyActor(env, torch_net(al, aa), torch_net(cl, ca) if critic else None, actor_inputs=ai, critic_inputs=ci if critic else None,
                     log_std=ls, **kw)
    return pa, al, cl


def inputs_of(env, names):
    return R.assemble([host(getattr(env, k)) for k in names])


# ---------------------------------------------------------------------------- (1) the kernel against the restatement
@pytest.mark.parametrize("dtype,v0", [("f64", False), ("f64", True), ("f32", False), ("f32", True)])
def test_kernel_matches_the_numpy_restatement(dtype, v0):
    """1, 17 and 33 standing envs with TSID beside the policy, a height scan and observation noise, after 5 driven steps; the
    three actors and the critic of policy_actor_reference.network_cases on the device's own rows, sampled and deterministic,
    written into buffers 3 rows too long.  Every mean, value, action32 and logp within the restatement's bound element by
    element, the assembled rows and the env-dtype action exact.
    Measured (MI355X), largest error / bound over the three env counts, three actors and both modes - float64 v1: mean 0.045, value
    0.004, action32 0.045, logp 0.036; float64 v0: 0.030, 0.003, 0.044, 0.055; float32 v1: 0.046, 0.004, 0.046, 0.048; float32 v0: 0.034,
    0.003, 0.052, 0.031 (the printed lines)."""
    from tsid_control_amd import PolicyActor
    worst = dict(mean=0.0, value=0.0, action32=0.0, logp=0.0)
    for n in (1, 17, 33):
        env = make_env(n, conf_of(dtype, v0, closed_loop=True), tsid="stand", mode="position", decimation=2, action_scale=0.25, seed=11,
                       reward_weights=dict(alive=1.0), randomization=dict(seed=7, env_offset=5, noise_joint_vel=0.5, noise_ang_vel=0.1),
                       terrain=dict(tilt_deg=3.0, step_height=(0.0, 0.01), **SCAN))
        NA = env.NA
        assert env.NOBS == (65 if v0 else 71) and env.height_scan.shape == (n, 77)
        for t in range(5):
            env.step(driven(n, NA, 50 + t, env, 0.3))
        torch.cuda.synchronize()
        episode, ep_len = host(env.episode), host(env.ep_len)
        assert (ep_len == 5).all()
        rng = np.random.default_rng(1000 * n + 2 * (dtype == "f32") + v0)
        ls = rng.uniform(-1.5, 0.0, NA).astype(np.float32)
        eps64 = R.eps(3, np.arange(n) + 5, episode, ep_len, NA)
        for name in ("tanh3", "elu_wide", "single"):
            (ai, al, aa), (ci, cl, ca) = nets_for(env, rng, name)
            pa = PolicyActor(env, torch_net(al, aa), torch_net(cl, ca), actor_inputs=ai, critic_inputs=ci,
                             log_std=torch.from_numpy(ls).to(env.device), seed=3)
            assert pa.env_offset == 5
            xa, xc = inputs_of(env, ai), inputs_of(env, ci)
            assert np.isfinite(xa).all() and xa.shape[1] == pa.actor_net.K and np.abs(xa).max() > 0.1
            y, by = R.forward_bound(xa, al, aa)
            v, bv = R.forward_bound(xc, cl, ca)
            for sampled in (True, False):
                s = R.sample(y, by, ls, eps64 if sampled else None)
                big = lambda *shape, dt=torch.float32: torch.full((n + 3,) + shape, -77.0, dtype=dt, device=env.device)
                o = dict(action=big(NA, dt=env.dtype), action32=big(NA), mean=big(NA), logp=big(), value=big(),
                         actor_input=big(xa.shape[1]), critic_input=big(xc.shape[1]))
                pa._launch(sampled, **o)
                torch.cuda.synchronize()
                g = {k: host(t) for k, t in o.items()}
                for k, t in g.items():
                    assert (t[n:] == -77.0).all(), (k, "rows beyond N touched")
                    g[k] = t[:n]
                assert np.array_equal(g["actor_input"], xa.astype(np.float32)) and np.array_equal(g["critic_input"], xc.astype(np.float32))
                assert np.array_equal(g["action"], g["action32"].astype(g["action"].dtype))
                for k, got, want, bound in (("mean", g["mean"], y, by), ("value", g["value"], v[:, 0], bv[:, 0]),
                                            ("action32", g["action32"], s["action"], s["b_action"]), ("logp", g["logp"], s["logp"], s["b_logp"])):
                    ratio = float((np.abs(got.astype(np.float64) - want) / bound).max())
                    print(f"{dtype} v0={v0} n={n} {name} sampled={sampled} {k}: error / bound {ratio:.3f}")
                    worst[k] = max(worst[k], ratio)
                    assert ratio <= 1.0, (n, name, sampled, k, ratio)
                if not sampled:
                    assert np.array_equal(g["action32"], g["mean"])
    print(f"{dtype} v0={v0} largest error / bound: " + ", ".join(f"{k} {r:.3f}" for k, r in worst.items()))


# ---------------------------------------------------------------------------- (2) the draws
def test_draws_are_the_restatements_repeatable_and_split_invariant():
    """eps recovered from action32, mean and log_std against the restatement's float32 eps: 4 ulp plus the sample's own bound
    divided by sigma - and with log_std = 0 on a mean of exactly 0, where action32 is eps itself, 4 ulp alone; the same on a second
    call, another after a step; 32 envs = two runs of 16 with env_offset 0 / 16."""
    n = 32
    kw = dict(decimation=4, action_scale=1.0, command_range=CMD, max_episode_steps=9, reward_weights=ALL_WEIGHTS, seed=13)
    whole = make_env(n, randomization=DR, **kw)
    halves = [make_env(n // 2, randomization=dict(DR, env_offset=off), **kw) for off in (0, n // 2)]
    actors = [small_actor(e, seed=4)[0] for e in [whole] + halves]
    assert [a.env_offset for a in actors] == [0, 0, 16] and actors[0].seed == 13
    for t in range(11):                                     # (across the timeout at 9: episode 2, every env its own ep_len history)
        action = driven(n, whole.NA, 700 + t, whole, step=t)
        whole.step(action)
        for h, sl in zip(halves, (slice(0, 16), slice(16, 32))):
            h.step(action[sl].contiguous())
    outs = [{k: v.clone() for k, v in a.act().items()} for a in actors]
    torch.cuda.synchronize()
    for k in ("action32", "logp", "mean", "value", "action"):
        assert torch.equal(outs[0][k], torch.cat([outs[1][k], outs[2][k]])), k
    pa, o = actors[0], outs[0]
    episode, ep_len = host(whole.episode), host(whole.ep_len)
    assert episode.max() >= 2 and len(set(ep_len.tolist())) > 1
    e32 = R.eps(13, np.arange(n), episode, ep_len, whole.NA).astype(np.float32).astype(np.float64)
    sig = np.exp(host(pa.log_std).astype(np.float64))
    mean = host(o["mean"]).astype(np.float64)
    rec = (host(o["action32"]).astype(np.float64) - mean) / sig
    tol = 4 * 2.0 ** -23 * np.abs(e32) + 4 * U * (np.abs(mean) + np.abs(sig * e32)) / sig
    assert (np.abs(rec - e32) <= tol).all(), float((np.abs(rec - e32) / tol).max())
    assert np.abs(e32).max() > 2.0 and abs(e32.mean()) < 0.2
    # log_std = 0 and a mean of exactly 0 (one all-zero layer): action32 is eps itself - 4 float32 ulp and nothing else
    from tsid_control_amd import PolicyActor
    f32 = dict(dtype=torch.float32, device=whole.device)
    pz = PolicyActor(whole, [(torch.zeros(whole.NA, whole.NOBS, **f32), torch.zeros(whole.NA, **f32))], log_std=torch.zeros(whole.NA, **f32))
    oz = pz.act()
    torch.cuda.synchronize()
    assert (host(oz["mean"]) == 0).all()
    direct = host(oz["action32"]).astype(np.float64)
    assert (np.abs(direct - e32) <= 4 * 2.0 ** -23 * np.abs(e32)).all(), float((np.abs(direct - e32) / np.abs(e32)).max() / 2.0 ** -23)
    sz = R.sample(np.zeros_like(e32), np.zeros_like(e32), np.zeros(whole.NA, dtype=np.float32), direct)
    assert (np.abs(host(oz["logp"]) - sz["logp"]) <= sz["b_logp"]).all()
    again = pa.act()
    assert torch.equal(again["action32"], o["action32"]) and torch.equal(again["logp"], o["logp"])
    whole.step(o["action"])
    moved = pa.act()
    torch.cuda.synchronize()
    rec2 = (host(moved["action32"]).astype(np.float64) - host(moved["mean"])) / sig
    assert (np.abs(rec2 - rec) > 1e-3).mean() > 0.95


# ---------------------------------------------------------------------------- (3) the parameters in place
def test_an_in_place_update_of_a_weight_is_seen_by_the_next_launch():
    n = 17
    env = make_env(n, decimation=4, randomization=dict(seed=2, reset_joint_pos=0.1, noise_joint_vel=0.3))
    pa, al, cl = small_actor(env, seed=6)
    env.step(driven(n, env.NA, 5, env, 0.3))
    before = {k: v.clone() for k, v in pa.act(deterministic=True).items()}
    lin = pa.actor_net.layers[1][0]
    delta = torch.full_like(lin, 0.01)
    delta[::2] *= -1
    with torch.no_grad():
        lin.add_(delta)
    after = pa.act(deterministic=True)
    torch.cuda.synchronize()
    al[1] = (host(lin), al[1][1])
    y, by = R.forward_bound(inputs_of(env, ("obs",)), al, "tanh")
    assert (np.abs(host(after["mean"]).astype(np.float64) - y) <= by).all()
    assert float((after["mean"] - before["mean"]).abs().max()) > 1e-3 and torch.equal(after["value"], before["value"])


# ---------------------------------------------------------------------------- (4) (5) a rollout and its advantages
def gae_gate(T, adv64, value):
    return 8 * T * U * max(1.0, float(np.abs(adv64).max()), float(np.abs(value).max()))


def check_gae(st, T):
    reward, done, timeout, value = host(st.reward), host(st.done), host(st.timeout), host(st.value)
    for gamma, lam in ((0.99, 0.95), (0.99, 0.0), (0.0, 0.95)):
        adv, ret = st.gae(gamma, lam)
        torch.cuda.synchronize()
        want_adv, want_ret = R.gae(reward, done, timeout, value, gamma, lam)
        gate = gae_gate(T, want_adv, value)
        ea, er = np.abs(host(adv) - want_adv).max(), np.abs(host(ret) - want_ret).max()
        print(f"gae T={T} gamma={gamma} lam={lam}: advantage error {ea:.2e}, returns {er:.2e}, gate {gate:.2e}")
        assert ea <= gate and er <= gate
        if lam == 0.0:
            delta = reward + gamma * value[:-1] * timeout + gamma * value[1:] * (1 - done) - value[:-1]
            assert np.abs(host(adv) - delta).max() <= gate


def test_rollout_is_the_hand_driven_loop_and_its_advantages():
    """16 envs x 12 steps, decimation 2, episodes of 5 steps: every slot of the storage against act() / step() / clone() on a twin,
    bit for bit, the sim state at the end too; value[T] is the critic on the final observation; then the advantages.
    Measured (MI355X), gamma 0.99 / lam 0.95: advantage error 9.4e-7, returns 1.3e-6 against a gate of 8.6e-5."""
    n, T = 16, 12
    kw = dict(decimation=2, action_scale=0.5, command_range=CMD, max_episode_steps=5, reward_weights=ALL_WEIGHTS, seed=3, randomization=DR)
    env, twin = make_env(n, **kw), make_env(n, **kw)
    pa, pb = small_actor(env, seed=8)[0], small_actor(twin, seed=8)[0]
    st = env.rollout(pa, T)
    rec = {k: [] for k in ("actor_input", "critic_input", "action", "mean", "logp", "value", "reward", "done", "timeout")}
    for t in range(T):
        o = pb.act()
        for k, v in (("actor_input", pb.actor_input), ("critic_input", pb.critic_input), ("action", o["action32"]), ("mean", o["mean"]),
                     ("logp", o["logp"]), ("value", o["value"])):
            rec[k].append(v.clone())
        _, reward, done, info = twin.step(o["action"])
        rec["reward"].append(reward.clone()); rec["done"].append(done.clone()); rec["timeout"].append(info["timeout"].clone())
    rec["value"].append(pb.act()["value"].clone())
    torch.cuda.synchronize()
    for k, rows in rec.items():
        got = getattr(st, k)
        assert got.shape[0] == len(rows) and got.is_contiguous()
        for t, row in enumerate(rows):
            assert same(got[t], row), (k, t)
    for a, b in zip(env.written(), twin.written()):
        assert same(a, b)
    assert st.done.sum() >= 2 * n and st.timeout.sum() >= n and 0 < st.done[:, 0].sum()
    assert env.rollout(pa, T, st) is st                      # reused; the episode counters moved on
    check_gae(st, T)


def test_gae_on_a_synthetic_rollout():
    """[32, 33]: more than one step, a partial workgroup; random dones (a fifth) and timeouts (half of them), the last step too.
    Measured (MI355X), gamma 0.99 / lam 0.95: advantage error 3.0e-6, returns 2.9e-6 against a gate of 2.0e-4."""
    from tsid_control_amd.policy_actor import RolloutStorage
    T, n = 32, 33
    env = make_env(n, "f32", decimation=2)
    pa = small_actor(env, seed=1)[0]
    st = RolloutStorage(env, pa, T)
    rng = np.random.default_rng(9)
    done = rng.random((T, n)) < 0.2
    done[T - 1, ::3] = True
    timeout = done & (rng.random((T, n)) < 0.5)
    st.reward.copy_(torch.from_numpy(rng.normal(0, 1, (T, n))))
    st.done.copy_(torch.from_numpy(done.astype(np.float64)))
    st.timeout.copy_(torch.from_numpy(timeout.astype(np.int32)))
    st.value.copy_(torch.from_numpy(rng.normal(0, 3, (T + 1, n))))
    assert timeout[T - 1].any() and (done[T - 1] & ~timeout[T - 1]).any()
    check_gae(st, T)


# ---------------------------------------------------------------------------- (6) a captured rollout
def test_captured_rollout_replays_bit_identically():
    """rollout(4) on 16 envs captured in a torch.cuda.graph: the replay against the eager rollout from the same rewound state"""
    from tsid_control_amd import rollout_written
    n, T = 16, 4
    env = make_env(n, decimation=2, action_scale=0.5, command_range=CMD, max_episode_steps=3, reward_weights=ALL_WEIGHTS, seed=3, randomization=DR)
    pa = small_actor(env, seed=8)[0]
    from tsid_control_amd.policy_actor import RolloutStorage
    st = RolloutStorage(env, pa, T)
    written = list(env.written()) + list(rollout_written(st))
    g, rewind = capture(lambda: env.rollout(pa, T, st), written)
    g.replay()
    torch.cuda.synchronize()
    replayed = [x.clone() for x in written]
    assert st.done.sum() >= n and float(st.logp.abs().min()) > 0
    rewind()
    env.rollout(pa, T, st)
    torch.cuda.synchronize()
    for x, r in zip(written, replayed):
        assert same(x, r)
    g.replay()                                              # a second replay goes on from there: the next 4 steps, other draws
    torch.cuda.synchronize()
    assert not torch.equal(st.action, replayed[[x is st.action for x in written].index(True)])


# ---------------------------------------------------------------------------- (7) the library's own checks
def test_calls_are_rejected_with_a_message_and_launch_nothing():
    from tsid_control_amd import _lib
    n = 4
    env = make_env(n, decimation=2)
    wc, NA, NOBS = env.wc, env.NA, env.NOBS
    pa = small_actor(env, seed=2)[0]
    mean = torch.full((n, NA), -77.0, dtype=torch.float32, device=env.device)
    value = torch.full((n,), -77.0, dtype=torch.float32, device=env.device)
    out = _lib.PolicyActorOut(None, None, mean.data_ptr(), None, value.data_ptr(), None, None)
    ls = C.c_void_p(pa.log_std.data_ptr())

    def copy(s, **kw):
        c = _lib.PolicyNet.from_buffer_copy(s)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    def call(actor, critic, bufs=env._bufs, out=out, log_std=ls, seed=1, offset=0, flags=1):
        ref = lambda s: C.byref(s) if s is not None else None
        wc._call("tsidb_policy_actor", ref(bufs), ref(actor), ref(critic), ref(out), log_std, C.c_uint64(seed), C.c_uint64(offset), flags,
                 wc._stream())
    a, c = pa.actor_net.struct, pa.critic_net.struct
    bad = [
        (dict(actor=copy(a, n_layers=5), critic=c), "actor: n_layers"), (dict(actor=copy(a, n_layers=0), critic=c), "actor: n_layers"),
        (dict(actor=a, critic=copy(c, n_blocks=5)), "critic: n_blocks"), (dict(actor=copy(a, n_blocks=0), critic=c), "actor: n_blocks"),
        (dict(actor=copy(a, width=(0, 513)), critic=c), "actor: width"), (dict(actor=copy(a, width=(1, 0)), critic=c), "actor: width"),
        (dict(actor=copy(a, block_cols=(0, 513)), critic=c), "actor: block_cols"), (dict(actor=copy(a, block_cols=(0, 0)), critic=c), "actor: block_cols"),
        (dict(actor=copy(a, block_ld=(0, NOBS - 1)), critic=c), "actor: block_ld"),
        (dict(actor=copy(a, block=(0, None)), critic=c), "actor: null input block"),
        (dict(actor=copy(a, weight=(1, None)), critic=c), "actor: null weight"),
        (dict(actor=copy(a, activation=3), critic=c), "actor: unknown activation"),
        (dict(actor=copy(a, width=(2, NA + 1)), critic=c), "actor: the last width must be NA"),
        (dict(actor=a, critic=copy(c, width=(1, 2))), "critic: the last width must be 1"),
        (dict(actor=a, critic=c, bufs=None), "sampling needs bufs"), (dict(actor=a, critic=c, log_std=None), "sampling needs log_std"),
        (dict(actor=a, critic=c, seed=2 ** 32), "seed must be below"), (dict(actor=a, critic=c, offset=2 ** 31), "env_offset below"),
        (dict(actor=a, critic=c, seed=2 ** 32, flags=0), "seed must be below"), (dict(actor=None, critic=c, offset=2 ** 31), "env_offset below"),
        (dict(actor=None, critic=None), "null actor"), (dict(actor=a, critic=c, out=None), "null out"),
    ]
    for kw, msg in bad:
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_actor: .*" + msg):
            call(**kw)
        assert wc._L.tsidb_last_error(wc._h).decode().startswith("tsidb_policy_actor: ")
    # an input row of more than 512 columns in total, block by block legal
    wide = torch.zeros(n, 300, dtype=env.dtype, device=env.device)
    too = copy(a, n_blocks=2, block=(1, wide.data_ptr()), block_cols=(1, 300), block_ld=(1, 300))
    too.block[0], too.block_cols[0], too.block_ld[0] = wide.data_ptr(), 300, 300
    with pytest.raises(_lib.TsidbError, match="actor: the input blocks must hold 1 .. 512 columns"):
        call(too, c)
    vp = lambda t: C.c_void_p(t.data_ptr())
    z = torch.zeros(2, n, dtype=torch.float32, device=env.device)
    r = torch.zeros(1, n, dtype=env.dtype, device=env.device)
    to = torch.zeros(1, n, dtype=torch.int32, device=env.device)
    adv = torch.full((1, n), -77.0, dtype=torch.float32, device=env.device)
    for T, args, msg in ((0, (vp(r), vp(r), vp(to), vp(z)), "T must be >= 1"), (-3, (vp(r), vp(r), vp(to), vp(z)), "T must be >= 1"),
                         (1, (None, vp(r), vp(to), vp(z)), "null buffer"), (1, (vp(r), vp(r), None, vp(z)), "null buffer")):
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_gae: " + msg):
            wc._call("tsidb_policy_gae", T, *args, C.c_float(0.99), C.c_float(0.95), vp(adv), vp(adv), wc._stream())
    torch.cuda.synchronize()
    assert (mean == -77.0).all() and (value == -77.0).all() and (adv == -77.0).all()      # nothing was launched
    # and without the flag neither bufs nor log_std is needed; the critic alone is a call too
    call(a, c, bufs=None, log_std=None, flags=0)
    torch.cuda.synchronize()
    want = pa.act(deterministic=True)
    assert torch.equal(mean, want["mean"]) and torch.equal(value, want["value"])
    value.fill_(-77.0)
    mean.fill_(-77.0)
    call(None, c, bufs=None, log_std=None)
    torch.cuda.synchronize()
    assert torch.equal(value, want["value"]) and (mean == -77.0).all()
