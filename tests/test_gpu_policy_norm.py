"""The policy normaliser on the device (tsidb_policy_norm_update, tsidb_policy_actor_norm, PolicyNormalizer) against the numpy
restatement tests/policy_norm_reference.py and its derived bound: the statistics, the normalised rows bit for bit, the actor's
outputs on them, off is off, until and eval(), determinism, a rollout against the hand-driven loop and its capture, the learner
on the stored rows, a checkpoint, and the library's own checks."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_actor_reference as RA  # noqa: E402
import policy_learner_reference as RL  # noqa: E402
import policy_norm_reference as R  # noqa: E402
from policy_testlib import capture, conf_of, host, make_env, same  # noqa: E402
from test_gpu_policy_actor import small_actor, torch_net  # noqa: E402
from test_gpu_policy_dr import CMD, DR, driven  # noqa: E402
from test_gpu_policy_env import ALL_WEIGHTS  # noqa: E402

pytestmark = pytest.mark.gpu

NFREE = 6                                  # columns of the free [N, k] block: K = NOBS + 4 + 6 = 81 (v1) / 75 (v0), no multiple of 16
ROLL = dict(decimation=2, action_scale=0.5, command_range=CMD, max_episode_steps=3, reward_weights=ALL_WEIGHTS, seed=3, randomization=DR)


def three_block_actor(env, seed, **kw):
    """(PolicyActor, normaliser, free block, actor layers, critic layers): the actor on a strided obs view, priv and a free
    [N, 6] tensor (24 and 40 wide, tanh), the critic on obs and priv (33 wide, ReLU)"""
    from tsid_control_amd import PolicyActor, PolicyNormalizer
    rng = np.random.default_rng(seed)
    free = torch.zeros(env.num_envs, NFREE, dtype=env.dtype, device=env.device)
    Ka, Kc = env.NOBS + 4 + NFREE, env.NOBS + 4
    al, cl = RA.make_layers(rng, Ka, [24, 40, env.NA]), RA.make_layers(rng, Kc, [33, 1])
    ls = torch.from_numpy(rng.uniform(-1.5, 0.0, env.NA).astype(np.float32)).to(env.device)
    nz = PolicyNormalizer(**kw)
    pa = PolicyActor(env, torch_net(al, "tanh"), torch_net(cl, "relu"), actor_inputs=("obs", "priv", free), critic_inputs=("obs", "priv"),
                     log_std=ls, seed=3, normalizer=nz)
    assert pa.actor_net.K == Ka and Ka % 16 and env.obs.stride(0) == Kc
    return pa, nz, free, al, cl


def fill(env, free, x):
    """the case's rows into the env's own row buffer (obs | priv) and the free block, in the env's dtype"""
    t = torch.from_numpy(x).to(env.device).to(env.dtype)
    env._rows.copy_(t[:, :env.NOBS + 4])
    free.copy_(t[:, env.NOBS + 4:])


def state_of(st):
    s = host(st.stats)
    return s[0], s[1], int(host(st.count)[0])


def bits(tensors):
    return [t.clone() for t in tensors]


# ---------------------------------------------------------------------------- (1) (2) (3) statistics, rows, outputs
@pytest.mark.parametrize("dtype,v0", [("f64", False), ("f64", True), ("f32", False), ("f32", True)])
def test_statistics_rows_and_outputs_match_the_restatement(dtype, v0):
    """1, 17, 33 and TSIDB_POL_NORM_SEG_ROWS + 33 envs (two segments, the second ragged), three successive updates on different
    rows of policy_norm_reference.case_rows.  Per update, from the device's own previous state: stats inside the derived bound
    element by element, count exact, affine[0] the cast of the device's mean, affine[1] within 2 float32 ulps of the restatement
    on the device's variance.  Then one launch with clip = 1.5: the stored rows are numpy's float32 map on the device's affine
    bit for bit, clamped entries and free ones both present; mean, value, action32 and logp inside policy_actor_reference's
    forward bound on those rows; the env-dtype action exact; rows beyond N untouched.
    Measured (MI355X), largest error / bound over the four env counts, both networks and the three updates - float64 envs, either
    robot: mean 0.279, var 0.318; float32 envs: mean 0.267, var 0.250 (the printed line)."""
    worst = dict(mean=0.0, var=0.0)
    for n in R.ENVS:
        env = make_env(n, conf_of(dtype, v0), decimation=2, seed=11, randomization=dict(seed=7, env_offset=5))
        NA = env.NA
        pa, nz, free, al, cl = three_block_actor(env, 100 + n, clip=1.5)
        for step in range(3):
            x = R.case_rows(n, pa.actor_net.K, 1000 * n + 10 * step + (dtype == "f32"))
            fill(env, free, x)
            torch.cuda.synchronize()
            blocks = np.concatenate([host(env.obs), host(env.priv), host(free)], axis=1)
            assert np.array_equal(blocks, x.astype(blocks.dtype))
            before = [state_of(nz.actor), state_of(nz.critic)]
            nz.update()
            torch.cuda.synchronize()
            for st, prev, K in ((nz.actor, before[0], pa.actor_net.K), (nz.critic, before[1], pa.critic_net.K)):
                eb = R.exact_and_bound(R.seen(blocks[:, :K]), *prev)
                mean, var, count = state_of(st)
                assert count == eb["count"] == (step + 1) * n
                for k, got in (("mean", mean), ("var", var)):
                    ratio = np.abs(got - eb[k]) / eb["b_" + k]
                    worst[k] = max(worst[k], float(ratio.max()))
                    assert (ratio <= 1.0).all(), (n, step, k, int(ratio.argmax()), float(ratio.max()))
                aff = host(st.affine)
                want = R.affine32(mean, var, nz.eps)
                assert np.array_equal(aff[0], mean.astype(np.float32))
                assert (np.abs(aff[1].astype(np.float64) - want[1].astype(np.float64)) <= 2 * np.spacing(want[1]).astype(np.float64)).all()
        # ---- the launch on the last rows
        episode, ep_len = host(env.episode), host(env.ep_len)
        eps64 = RA.eps(3, np.arange(n) + 5, episode, ep_len, NA)
        big = lambda *shape, dt=torch.float32: torch.full((n + 3,) + shape, -77.0, dtype=dt, device=env.device)
        for sampled in (True, False):
            o = dict(action=big(NA, dt=env.dtype), action32=big(NA), mean=big(NA), logp=big(), value=big(),
                     actor_input=big(pa.actor_net.K), critic_input=big(pa.critic_net.K))
            pa._launch(sampled, **o)
            torch.cuda.synchronize()
            got = {k: host(t) for k, t in o.items()}
            for k, t in got.items():
                assert (t[n:] == -77.0).all(), (k, "rows beyond N touched")
                got[k] = t[:n]
            xa = R.normalise32(blocks, host(nz.actor.affine), 1.5)
            xc = R.normalise32(blocks[:, :pa.critic_net.K], host(nz.critic.affine), 1.5)
            assert xa.dtype == np.float32 and np.array_equal(got["actor_input"], xa) and np.array_equal(got["critic_input"], xc)
            if n >= 17:
                assert (np.abs(xa) == 1.5).any() and (np.abs(xa) < 1.5).any() and (np.abs(xc) == 1.5).any() and (np.abs(xc) < 1.5).any()
            y, by = RA.forward_bound(xa, al, "tanh")
            v, bv = RA.forward_bound(xc, cl, "relu")
            s = RA.sample(y, by, host(pa.log_std), eps64 if sampled else None)
            assert np.array_equal(got["action"], got["action32"].astype(got["action"].dtype))
            for k, have, want, bound in (("mean", got["mean"], y, by), ("value", got["value"], v[:, 0], bv[:, 0]),
                                         ("action32", got["action32"], s["action"], s["b_action"]), ("logp", got["logp"], s["logp"], s["b_logp"])):
                ratio = float((np.abs(have.astype(np.float64) - want) / bound).max())
                assert ratio <= 1.0, (n, sampled, k, ratio)
    print(f"{dtype} v0={v0} largest error / bound: mean {worst['mean']:.3f}, var {worst['var']:.3f}")


# ---------------------------------------------------------------------------- (4) off is off
def test_off_is_off_and_the_initial_state_is_a_plain_scale():
    """No normaliser: PolicyActor's launch (tsidb_policy_actor) and tsidb_policy_actor_norm with no norm, and with norms whose
    affine is NULL, write the same bits everywhere.  A normaliser in its initial state, in eval mode: rows = x * float32(1 / (1 + eps))."""
    from tsid_control_amd import PolicyNormalizer, _lib
    n = 33
    env = make_env(n, decimation=2, seed=5, randomization=dict(seed=2, reset_joint_pos=0.1, noise_joint_vel=0.3))
    for t in range(3):
        env.step(driven(n, env.NA, 20 + t, env, 0.3))
    pa = small_actor(env, seed=6)[0]
    assert pa.normalizer is None
    names = ("action", "action32", "mean", "logp", "value", "actor_input", "critic_input")
    want = bits([pa.act()[k] for k in names[:5]] + [pa.actor_input, pa.critic_input])
    wc = env.wc
    for norms in ((None, None), (_lib.PolicyNorm(), _lib.PolicyNorm())):
        outs = [torch.full_like(t, -77.0) for t in want]
        out = _lib.PolicyActorOut(*[t.data_ptr() for t in outs])
        ref = lambda s: C.byref(s) if s is not None else None
        wc._call("tsidb_policy_actor_norm", C.byref(env._bufs), C.byref(pa.actor_net.struct), C.byref(pa.critic_net.struct), ref(norms[0]),
                 ref(norms[1]), C.byref(out), C.c_void_p(pa.log_std.data_ptr()), C.c_uint64(pa.seed), C.c_uint64(pa.env_offset), 1, wc._stream())
        torch.cuda.synchronize()
        for k, a, b in zip(names, outs, want):
            assert same(a, b), k
    pn = small_actor(env, seed=6, normalizer=PolicyNormalizer(eps=0.25))[0]
    nz = pn.normalizer.eval()
    pn.act()
    torch.cuda.synchronize()
    scale = np.float32(1.0 / 1.25)
    assert np.array_equal(host(pn.actor_input), host(pa.actor_input) * scale) and np.array_equal(host(pn.critic_input), host(pa.critic_input) * scale)
    assert int(nz.actor.count) == 0 and not torch.equal(pn.mean, pa.mean)


# ---------------------------------------------------------------------------- (5) (6) until, eval(), determinism
def test_until_eval_and_two_updates_from_one_state():
    n = 17
    env = make_env(n, "f32", decimation=2, seed=5)
    pa, nz, free, _, _ = three_block_actor(env, 1, until=30)
    K = pa.actor_net.K
    state = lambda: bits(nz.written()[:-1])
    counts = []
    for step in range(4):
        fill(env, free, R.case_rows(n, K, 50 + step))
        before = state()
        nz.update()
        torch.cuda.synchronize()
        counts.append((int(nz.actor.count), int(nz.critic.count)))
        changed = [not torch.equal(a, b) for a, b in zip(before, state())]
        assert all(changed) if step < 2 else not any(changed), (step, changed)
    assert counts == [(17, 17), (34, 34), (34, 34), (34, 34)]       # the first value >= until, and never past it
    # eval(): act() and a rollout leave every bit
    pb, nb, fb, _, _ = three_block_actor(env, 1)
    fill(env, fb, R.case_rows(n, K, 60))
    pb.act()
    nb.eval()
    before = bits(nb.written()[:-1])
    pb.act()
    env.rollout(pb, 2)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, bits(nb.written()[:-1]))) and int(nb.actor.count) == n
    # two updates from the same rewound state: the same bits, workspace included
    nb.train()
    saved = bits(nb.written())
    nb.update()
    torch.cuda.synchronize()
    first = bits(nb.written())
    for t, s in zip(nb.written(), saved):
        t.copy_(s)
    nb.workspace.fill_(float("nan"))
    nb.update()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, nb.written())) and int(nb.actor.count) == 2 * n
    assert not torch.equal(first[0], saved[0])


# ---------------------------------------------------------------------------- (7) (8) a rollout, its capture, the learner
def norm_actor(env, seed=8, **kw):
    from tsid_control_amd import PolicyNormalizer
    pa, al, cl = small_actor(env, seed=seed, normalizer=PolicyNormalizer(**kw))
    return pa, pa.normalizer, al, cl


def test_rollout_is_the_hand_driven_loop_and_the_learner_reads_its_rows():
    """16 envs x 4 steps in training mode against update() / _launch / step() on a twin, bit for bit, storage and normaliser state;
    count = 4 N: the closing value launch did not update.  Then PolicyLearner.backward over all rows: mu and v are storage.mean
    and storage.value[:T] bit for bit, the gradients inside the learner test's gate (8 x e32) of policy_learner_reference on the
    stored, normalised rows.
    Measured (MI355X): largest error / gate 0.135 (actor.0.weight)."""
    from tsid_control_amd import PolicyLearner
    from test_policy_learner_reference import e32
    n, T = 16, 4
    env, twin = make_env(n, **ROLL), make_env(n, **ROLL)
    (pa, nz, al, cl), (pb, nb, _, _) = norm_actor(env, clip=5.0), norm_actor(twin, clip=5.0)
    st = env.rollout(pa, T)
    rec = {k: [] for k in ("actor_input", "critic_input", "action", "mean", "logp", "value", "reward", "done", "timeout")}
    for t in range(T):
        nb.update()
        pb._launch(True, action=pb.action, action32=pb.action32, mean=pb.mean, logp=pb.logp, value=pb.value, actor_input=pb.actor_input,
                   critic_input=pb.critic_input)
        for k, v in (("actor_input", pb.actor_input), ("critic_input", pb.critic_input), ("action", pb.action32), ("mean", pb.mean),
                     ("logp", pb.logp), ("value", pb.value)):
            rec[k].append(v.clone())
        _, reward, done, info = twin.step(pb.action)
        rec["reward"].append(reward.clone()); rec["done"].append(done.clone()); rec["timeout"].append(info["timeout"].clone())
    pb._launch(False, actor=False, value=pb.value)
    rec["value"].append(pb.value.clone())
    torch.cuda.synchronize()
    for k, rows in rec.items():
        for t, row in enumerate(rows):
            assert same(getattr(st, k)[t], row), (k, t)
    for a, b in zip(list(env.written()) + nz.written(), list(twin.written()) + nb.written()):
        assert same(a, b)
    assert int(nz.actor.count) == int(nz.critic.count) == T * n and st.done.sum() >= n
    assert float((nz.actor.stats[1] - 1.0).abs().min()) > 0 and float(st.actor_input.abs().max()) <= 5.0
    # ---- the learner
    st.gae()
    pl = PolicyLearner(pa, clip=0.2, value_coef=0.7, entropy_coef=0.01, value_clip=False)
    index = torch.randperm(n * T, generator=torch.Generator().manual_seed(1)).to(torch.int32).to(env.device)
    pl.fill_adv_stats(st)
    stats = host(pl.backward(st, index, adv_stats=pl.adv_stats))
    mu, v = pl.outputs(n * T)
    j = index.long()
    assert torch.equal(mu, st.mean.reshape(-1, env.NA)[j]) and torch.equal(v, st.value[:T].reshape(-1)[j])
    flat = lambda t, *s: host(t).reshape(n * T, *s)
    case = dict(name="rollout", v0=False, na=env.NA, M=n * T, rows=n * T, clip=0.2, value_coef=0.7, entropy_coef=0.01, value_clip=False,
                actor=(al, "tanh"), critic=(cl, "relu"), actor_input=flat(st.actor_input, -1), critic_input=flat(st.critic_input, -1),
                action=flat(st.action, -1), logp=flat(st.logp), value=flat(st.value[:T]), advantage=flat(st.advantage),
                returns=flat(st.returns), adv_stats=host(pl.adv_stats), log_std=host(pa.log_std), index=host(index))
    ev = RL.evaluate(case)
    E = max(e32(case), 2.0 ** -22)
    got = {}
    for name, net in (("actor", pa.actor_net), ("critic", pa.critic_net)):
        for l, (w, b) in enumerate(net.layers):
            got[f"{name}.{l}.weight"], got[f"{name}.{l}.bias"] = host(w.grad), host(b.grad)
    got["log_std"] = host(pa.log_std.grad)
    for k, g64 in RL.grad_list(ev):
        ratio = float(np.abs(got[k] - g64).max() / (8 * E * np.abs(g64).max()))
        print(f"{k}: error / gate {ratio:.3f}")
        assert ratio <= 1.0, (k, ratio)
    assert list(stats[6:]) == [n * T, 0]


def test_captured_rollout_replays_bit_identically():
    """rollout(4) on 16 envs in training mode captured in a torch.cuda.graph: the replay against the eager rollout from the same
    rewound state, the normaliser's state among the rewound tensors"""
    from tsid_control_amd import rollout_written
    from tsid_control_amd.policy_actor import RolloutStorage
    n, T = 16, 4
    env = make_env(n, **ROLL)
    pa, nz, _, _ = norm_actor(env)
    st = RolloutStorage(env, pa, T)
    written = list(env.written()) + list(rollout_written(st))
    assert all(any(t is w for w in written) for t in nz.written())
    g, rewind = capture(lambda: env.rollout(pa, T, st), written)
    g.replay()
    torch.cuda.synchronize()
    replayed = bits(written)
    assert int(nz.actor.count) == T * n
    rewind()
    assert int(nz.actor.count) == 0
    env.rollout(pa, T, st)
    torch.cuda.synchronize()
    for x, r in zip(written, replayed):
        assert same(x, r)
    g.replay()
    torch.cuda.synchronize()
    assert int(nz.actor.count) == 2 * T * n


# ---------------------------------------------------------------------------- (9) a checkpoint
def test_a_loaded_state_dict_reproduces_the_actor():
    n = 33
    env = make_env(n, **ROLL)
    pa, nz, _, _ = norm_actor(env, clip=4.0)
    env.rollout(pa, 3)
    nz.eval()
    want = {k: v.clone() for k, v in pa.act(deterministic=True).items()}
    pb, nb, _, _ = norm_actor(env, clip=4.0)
    nb.load_state_dict(nz.state_dict())
    nb.eval()
    got = pb.act(deterministic=True)
    torch.cuda.synchronize()
    for a, b in zip(nz.written()[:-1], nb.written()[:-1]):
        assert torch.equal(a, b)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(pa.actor_input, pb.actor_input) and int(nb.actor.count) == 3 * n and float(want["mean"].abs().max()) > 1e-3


# ---------------------------------------------------------------------------- (10) the library's own checks
def test_calls_are_rejected_with_a_message_and_launch_nothing():
    from tsid_control_amd import _lib
    n = 4
    env = make_env(n, decimation=2)
    wc, NOBS = env.wc, env.NOBS
    pa, nz, _, _ = norm_actor(env, clip=3.0)
    pa.act()
    torch.cuda.synchronize()
    a, c, an, cn = pa.actor_net.struct, pa.critic_net.struct, nz.actor.struct, nz.critic.struct
    ws = nz.workspace
    before = bits(pa.written())

    def copy(s, **kw):
        o = type(s).from_buffer_copy(s)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(o, k)[v[0]] = v[1]
            else:
                setattr(o, k, v)
        return o
    ref = lambda s: C.byref(s) if s is not None else None

    def update(actor=a, critic=c, actor_norm=an, critic_norm=cn, workspace=ws.data_ptr(), nbytes=ws.numel() * 8):
        wc._call("tsidb_policy_norm_update", ref(actor), ref(critic), ref(actor_norm), ref(critic_norm), C.c_void_p(workspace), C.c_size_t(nbytes),
                 wc._stream())
    bad = [
        (dict(actor=None, critic=None), "null actor and critic"),
        (dict(actor_norm=None), "actor: no normaliser"), (dict(critic_norm=None), "critic: no normaliser"),
        (dict(actor_norm=copy(an, stats=None)), "actor: no normaliser"), (dict(critic_norm=copy(cn, count=None)), "critic: no normaliser"),
        (dict(actor_norm=copy(an, affine=None)), "actor: no normaliser"),
        (dict(actor_norm=copy(an, eps=0.0)), "actor: eps must be > 0"), (dict(critic_norm=copy(cn, eps=float("nan"))), "critic: eps must be > 0"),
        (dict(actor_norm=copy(an, until=-1)), "actor: until must be >= 0"),
        (dict(workspace=None), "null workspace"), (dict(nbytes=ws.numel() * 8 - 8), "workspace of .* bytes, .* needed"),
        (dict(actor=copy(a, n_blocks=0)), "actor: n_blocks"), (dict(critic=copy(c, n_blocks=5)), "critic: n_blocks"),
        (dict(actor=copy(a, block_cols=(0, 0))), "actor: block_cols"), (dict(actor=copy(a, block_cols=(0, 513))), "actor: block_cols"),
        (dict(actor=copy(a, block_ld=(0, NOBS - 1))), "actor: block_ld"), (dict(critic=copy(c, block=(0, None))), "critic: null input block"),
    ]
    for kw, msg in bad:
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_norm_update: " + msg):
            update(**kw)
    size = C.c_size_t(0)
    wc._call("tsidb_policy_norm_workspace", ref(a), ref(c), C.byref(size))
    assert size.value == ws.numel() * 8 == 16 * (pa.actor_net.K + pa.critic_net.K)
    with pytest.raises(_lib.TsidbError, match="tsidb_policy_norm_workspace: null bytes"):
        wc._call("tsidb_policy_norm_workspace", ref(a), ref(c), None)
    out = _lib.PolicyActorOut(*[t.data_ptr() for t in (pa.action, pa.action32, pa.mean, pa.logp, pa.value, pa.actor_input, pa.critic_input)])

    def launch(actor=a, critic=c, actor_norm=an, critic_norm=cn):
        wc._call("tsidb_policy_actor_norm", C.byref(env._bufs), ref(actor), ref(critic), ref(actor_norm), ref(critic_norm), C.byref(out),
                 C.c_void_p(pa.log_std.data_ptr()), C.c_uint64(1), C.c_uint64(0), 1, wc._stream())
    for kw, msg in ((dict(actor=None), "actor_norm without an actor"), (dict(critic=None), "critic_norm without a critic"),
                    (dict(actor_norm=copy(an, clip=-1.0)), "actor_norm: clip must be >= 0"),
                    (dict(critic_norm=copy(cn, clip=float("nan"))), "critic_norm: clip must be >= 0"),
                    (dict(actor=copy(a, n_layers=5)), "actor: n_layers")):
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_actor_norm: " + msg):
            launch(**kw)
    torch.cuda.synchronize()
    for x, b in zip(pa.written(), before):
        assert same(x, b)                                   # nothing was launched: every state tensor keeps its bits
    # the actor alone, and the critic alone, are calls too
    update(critic=None, critic_norm=None)
    update(actor=None, actor_norm=None)
    torch.cuda.synchronize()
    assert int(nz.actor.count) == int(nz.critic.count) == 2 * n
