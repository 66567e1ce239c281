"""The observation history on the GPU (tsidb_policy_obs_history; PolicyEnv(obs_history=), "obs_history" as a PolicyActor
block): the kernel against the numpy restatement on the device's own rows, the frames against what the caller saw, partial
resets, off-is-off against twins, a captured step, the actor and rollout() on the stacked row, and a split batch.

Every comparison of the history is bit for bit (policy_testlib.same: NaN equals NaN): the kernel only copies, so there is no
tolerance anywhere in this file."""
import ctypes as C
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_obs_history_reference as hr  # noqa: E402
from policy_testlib import capture, host, make_env, replay_against_eager, same  # noqa: E402
from test_gpu_policy_dr import CMD  # noqa: E402
from test_gpu_policy_env import rand  # noqa: E402

pytestmark = pytest.mark.gpu

# observation noise on (frames must be copies of the noisy rows, not redraws), reset noise so that first observations differ
NOISE = dict(seed=7, reset_joint_pos=0.1, reset_joint_vel=0.5, noise_ang_vel=0.2, noise_gravity=0.05, noise_joint_pos=0.01, noise_joint_vel=1.5)
ENV = dict(decimation=2, mode="motor", action_scale=1.0, command_range=CMD, max_episode_steps=5, seed=3,
           reward_weights=dict(track_lin_vel=1.0, alive=0.2, action_rate=-0.01, termination=-5.0), randomization=NOISE)
ROBOTS = [("f64", False), ("f64", True), ("f32", False), ("f32", True)]
FRAMES = (1, 2, 7)


def source_cases(nobs):
    """K = 3: fewer columns than lanes; NOBS = 71 / 65: one over a wavefront; two strided views of one row; two ranges that skip
    the command"""
    return [("command",), ("obs",), ("obs", "priv"), (("obs", 0, 6), ("obs", 9, nobs))]


def tensors_of(env):
    return {k: host(getattr(env, k)) for k in ("obs", "priv", "command")}


def columns_of(env):
    return dict(obs=env.NOBS, priv=4, command=3)


def small(n, na, seed, env):
    """actions nobody falls from in the few sim steps of a test: restarts come from the timeout and from the test's own NaNs"""
    return rand((n, na), seed, env, 0.05)


def want_equal(t, want, what):
    assert same(t.cpu(), torch.from_numpy(np.ascontiguousarray(want))), what


class Shadow:
    """one more history on an env's rows, driven through the entry point directly: its own tensor and block"""

    def __init__(self, env, frames, sources):
        from tsid_control_amd import _lib
        self.frames, self.resolved = frames, hr.resolve(sources, columns_of(env))
        self.K = sum(hi - lo for _, lo, hi in self.resolved)
        self.hist = torch.zeros(env.num_envs, frames * self.K, dtype=env.dtype, device=env.device)
        h = self.block = _lib.PolicyObsHistory()
        h.history, h.frames, h.n_src = self.hist.data_ptr(), frames, len(self.resolved)
        item = self.hist.element_size()
        for i, (name, lo, hi) in enumerate(self.resolved):
            t = getattr(env, name)
            h.src[i], h.src_ld[i], h.src_cols[i] = t.data_ptr() + lo * item, t.stride(0), hi - lo
        self.want = host(self.hist)

    def launch(self, env, push):
        wc = env.wc
        wc._call("tsidb_policy_obs_history", C.byref(self.block), C.c_void_p(wc.rows.data_ptr()), wc.NROW, push, wc._stream())

    def check(self, env, done, push, what):
        self.want = hr.update(self.want, hr.select(tensors_of(env), self.resolved), done, push)
        want_equal(self.hist, self.want, what)


# ---------------------------------------------------------------------------- (1) against the restatement
@pytest.mark.parametrize("n", [1, 17, 65])
@pytest.mark.parametrize("dtype,v0", ROBOTS)
def test_history_is_the_restatement_on_the_devices_own_rows(dtype, v0, n):
    """14 steps, episodes of 5, observation noise on, a NaN action for env n // 2 at steps 6 and 8 (the header's rule ends exactly
    that env's episode), one reset(env_ids) after step 10.  Every (frames, sources) pair of the table runs on the same rows: one
    of them is the env's own obs_history (a different one in each case of the test), the others are launched through the entry
    point on tensors of the test's.  After every call each history equals the restatement applied to its previous value, the
    env's current source tensors and the done flags."""
    nobs = 65 if v0 else 71
    combos = list(itertools.product(FRAMES, source_cases(nobs)))
    own = combos[(ROBOTS.index((dtype, v0)) * 3 + [1, 17, 65].index(n)) % len(combos)]
    env = make_env(n, dtype, v0, obs_history=dict(frames=own[0], sources=own[1]), **ENV)
    assert env.NOBS == nobs and env.obs_history.shape == (n, own[0] * sum(hi - lo for _, lo, hi in env.obs_history_sources))
    assert env.obs_history.dtype == env.dtype and env.obs_history.is_contiguous()
    shadows = [Shadow(env, f, s) for f, s in combos]
    mine = shadows[combos.index(own)]
    # the constructor's reset(): every env holds `frames` copies of its first observation
    ones = np.ones(n)
    env.wc.done.fill_(1)
    for s in shadows:
        s.launch(env, 0)
    env.wc.done.zero_()
    torch.cuda.synchronize()
    for s in shadows:
        s.check(env, ones, 0, "first")
    assert same(env.obs_history, mine.hist)
    m, seen = n // 2, dict(some=0, every=0, none=0, partial_reset=0)
    for t in range(14):
        action = small(n, env.NA, 100 + t, env)
        if t in (6, 8):
            action[m, 0] = float("nan")
        obs, reward, done, info = env.step(action)
        assert info["obs_history"] is env.obs_history
        for s in shadows:
            s.launch(env, 1)
        torch.cuda.synchronize()
        d = host(done)
        fresh = d != 0
        if t in (6, 8):
            assert fresh.tolist() == [e == m for e in range(n)]
        seen["every" if fresh.all() else "some" if fresh.any() else "none"] += 1
        for s in shadows:
            s.check(env, d, 1, (t, s.frames, s.resolved))
        assert same(env.obs_history, mine.hist), t
        if t == 10:
            ids = sorted({0, n - 1})
            before = env.obs_history.clone()
            env.reset(ids)
            d = np.zeros(n)
            d[ids] = 1
            env.wc.done[ids] = 1                       # (as reset() had them while its launches ran)
            for s in shadows:
                s.launch(env, 0)
            env.wc.done.zero_()
            torch.cuda.synchronize()
            for s in shadows:
                s.check(env, d, 0, ("reset", s.frames, s.resolved))
            assert same(env.obs_history, mine.hist)
            rest = [e for e in range(n) if e not in ids]
            assert same(env.obs_history[rest], before[rest])
            seen["partial_reset"] += 1
    # conditions, not measurements: every kind of call occurred (one env alone cannot restart "some but not all")
    assert seen["every"] >= 1 and seen["none"] >= 1 and seen["partial_reset"] == 1 and (seen["some"] >= 1 or n == 1), seen


# ---------------------------------------------------------------------------- (2) frames are the rows the caller saw
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_frames_are_the_observations_the_steps_returned(dtype):
    n, H = 17, 4
    env = make_env(n, dtype, obs_history=dict(frames=H, sources=("obs",)), **ENV)
    K = env.NOBS
    frame = lambda h: env.obs_history[:, h * K:(h + 1) * K]
    assert same(frame(H - 1), env.obs) and same(frame(0), env.obs)
    seen_obs, seen_done, checked = [], [], 0
    for t in range(12):
        obs, reward, done, info = env.step(small(n, env.NA, 200 + t, env))
        torch.cuda.synchronize()
        seen_obs.append(obs.clone())
        seen_done.append(done.clone() != 0)
        assert same(frame(H - 1), obs), t                               # the newest frame is the current selection
        if t >= 2:
            kept = ~(seen_done[t] | seen_done[t - 1])                   # not restarted since step t - 2 returned
            assert same(frame(H - 2)[kept], seen_obs[t - 1][kept]) and same(frame(H - 3)[kept], seen_obs[t - 2][kept]), t
            assert not torch.equal(seen_obs[t - 1][kept], seen_obs[t][kept]) or not kept.any()   # (noise and motion: no two rows alike)
            checked += int(kept.sum())
        new = seen_done[t]
        assert same(env.obs_history[new], obs[new].repeat(1, H))       # a restarted env: H copies of its first observation
        if t == 7:
            env.reset([3])
            assert same(frame(H - 1), env.obs) and same(env.obs_history[3], env.obs[3].repeat(H))
            seen_done[t][3] = True
            seen_obs[t] = env.obs.clone()
    assert checked >= 4 * n and sum(int(d.sum()) for d in seen_done) >= 2 * n
    env.reset()
    assert same(env.obs_history, env.obs.repeat(1, H))


# ---------------------------------------------------------------------------- (3) reset(env_ids)
def test_a_partial_reset_leaves_the_other_histories_alone():
    n, H = 17, 3
    env = make_env(n, obs_history=dict(frames=H, sources=("obs", "priv")), **ENV)
    for t in range(3):
        env.step(small(n, env.NA, 300 + t, env))
    before, obs_before = env.obs_history.clone(), env._rows.clone()
    ids = [2, 5, 16]
    rest = [e for e in range(n) if e not in ids]
    env.reset(ids)
    torch.cuda.synchronize()
    assert same(env.obs_history[rest], before[rest])
    assert same(env.obs_history[ids], env._rows[ids].repeat(1, H)) and not torch.equal(env._rows[ids], obs_before[ids])
    # the others' newest frame still is their current selection: reset() recomputed their rows to the same bits
    assert same(env.obs_history[:, -env._rows.shape[1]:], env._rows)
    env.reset(torch.tensor([], dtype=torch.long))                       # nobody: nothing moves
    torch.cuda.synchronize()
    assert same(env.obs_history[rest], before[rest])


# ---------------------------------------------------------------------------- (4) off is the parent
def test_off_is_the_env_without_the_argument():
    n = 17
    plain, none = make_env(n, **ENV), make_env(n, obs_history=None, **ENV)
    on = make_env(n, obs_history=dict(frames=3, sources=("obs", "command")), **ENV)
    assert plain.obs_history is None and none.obs_history is None and none._obs_history is None
    restarts = 0
    for t in range(12):
        action = small(n, plain.NA, 400 + t, plain)
        if t == 7:
            action[4, 0] = float("nan")
        outs = [e.step(action) for e in (plain, none, on)]
        torch.cuda.synchronize()
        restarts += int(plain.done.sum())
        assert sorted(outs[0][3]) == sorted(outs[1][3]) and sorted(set(outs[2][3]) - set(outs[0][3])) == ["obs_history"]
        a, b, c = (list(e.written()) for e in (plain, none, on))
        assert len(a) == len(b) == len(c) - 1 and c[-1] is on.obs_history
        for x, y, z in zip(a, b, c):
            assert same(x, y) and same(x, z), t
    assert restarts >= 2 * n


# ---------------------------------------------------------------------------- (5) a captured step
def test_captured_step_replays_the_history_bit_identically():
    n, steps = 17, 10
    kw = dict(obs_history=dict(frames=3, sources=("obs", "priv")), **ENV)
    eager, env = make_env(n, **kw), make_env(n, **kw)
    assert any(x is env.obs_history for x in env.written())
    actions = [small(n, env.NA, 500 + t, env) for t in range(steps)]
    restarts = 0
    for t in replay_against_eager(env, eager, actions):
        restarts += int(env.done.sum())
    assert t == steps - 1 and restarts >= n                             # (the timeout of step 5 lies inside the replays)
    assert same(env.obs_history, eager.obs_history) and float(env.obs_history.abs().sum()) > 0


# ---------------------------------------------------------------------------- (6) the actor and rollout()
def nets(k_actor, k_critic, na, seed=0):
    torch.manual_seed(seed)
    mlp = lambda k, out: torch.nn.Sequential(torch.nn.Linear(k, 32), torch.nn.ELU(), torch.nn.Linear(32, out)).to("cuda:0")
    return mlp(k_actor, na), mlp(k_critic, 1)


def history_actor(env, shared, **kw):
    from tsid_control_amd import PolicyActor
    return PolicyActor(env, shared[0], shared[1], actor_inputs=("obs_history", "command"), critic_inputs=("obs_history", "priv"), seed=8, **kw)


ROLL = dict(obs_history=dict(frames=7, sources=("obs",)), **ENV)      # 7 x 71 = 497 columns: with the command 500 of the actor's 512


def test_actor_reads_the_stacked_row():
    from tsid_control_amd import PolicyActor, _lib
    n = 17
    env = make_env(n, **ROLL)
    assert env.obs_history.shape == (n, 497)
    shared = nets(500, 501, env.NA)
    pa = history_actor(env, shared)
    for t in range(3):
        out = pa.act()
        torch.cuda.synchronize()
        assert torch.equal(pa.actor_input, torch.cat([env.obs_history, env.command], 1).float())
        assert torch.equal(pa.critic_input, torch.cat([env.obs_history, env.priv], 1).float())
        env.step(out["action"])
    # 7 x 71 alone is accepted; 8 x 71 is the env's to accept and the actor's to refuse
    PolicyActor(env, torch.nn.Sequential(torch.nn.Linear(497, env.NA)).to("cuda:0"), actor_inputs=("obs_history",))
    wide = make_env(2, obs_history=dict(frames=8, sources=("obs",)))
    assert wide.obs_history.shape == (2, 568)
    with pytest.raises(_lib.TsidbError, match="PolicyActor: actor_inputs: the input row has 568 columns, 1 .. 512 allowed"):
        PolicyActor(wide, torch.nn.Sequential(torch.nn.Linear(568, wide.NA)).to("cuda:0"), actor_inputs=("obs_history",))
    plain = make_env(2)
    with pytest.raises(_lib.TsidbError, match="the env has no obs_history"):
        PolicyActor(plain, shared[0], actor_inputs=("obs_history", "command"))


@pytest.mark.parametrize("normalizer", [False, True])
def test_rollout_is_the_hand_driven_loop(normalizer):
    """16 envs x 6 steps: every slot of the storage, actor_input among them, against act() / step() on a twin, bit for bit; with a
    PolicyNormalizer in training mode too (its update reads the stacked row)"""
    from tsid_control_amd import PolicyNormalizer
    n, T = 16, 6
    env, twin = make_env(n, **ROLL), make_env(n, **ROLL)
    shared = nets(500, 501, env.NA)
    kw = lambda: dict(normalizer=PolicyNormalizer(clip=5.0)) if normalizer else {}
    pa, pb = history_actor(env, shared, **kw()), history_actor(twin, shared, **kw())
    st = env.rollout(pa, T)
    rec = {k: [] for k in ("actor_input", "critic_input", "action", "mean", "logp", "value", "reward", "done", "timeout")}
    for t in range(T):
        o = pb.act()
        for k, v in (("actor_input", pb.actor_input), ("critic_input", pb.critic_input), ("action", o["action32"]), ("mean", o["mean"]),
                     ("logp", o["logp"]), ("value", o["value"])):
            rec[k].append(v.clone())
        _, reward, done, info = twin.step(o["action"])
        rec["reward"].append(reward.clone()); rec["done"].append(done.clone()); rec["timeout"].append(info["timeout"].clone())
    pb._launch(False, actor=False, value=pb.value)
    rec["value"].append(pb.value.clone())
    torch.cuda.synchronize()
    for k, rows in rec.items():
        for t, row in enumerate(rows):
            assert same(getattr(st, k)[t], row), (k, t)
    state = lambda e, p: list(e.written()) + [p.action] + (p.normalizer.written() if normalizer else [])   # (what a rollout writes outside its storage)
    for a, b in zip(state(env, pa), state(twin, pb)):
        assert same(a, b)
    assert st.done.sum() >= n
    if not normalizer:
        # the stored rows are the env's history as it stood: slot 2's newest frame is slot 3's second newest where step 2 restarted nothing
        kept = st.done[2] == 0
        assert torch.equal(st.actor_input[3][kept][:, 5 * 71:6 * 71], st.actor_input[2][kept][:, 6 * 71:7 * 71]) and kept.all()


def test_captured_rollout_replays_bit_identically():
    from tsid_control_amd import rollout_written
    from tsid_control_amd.policy_actor import RolloutStorage
    n, T = 16, 4
    env = make_env(n, **ROLL)
    pa = history_actor(env, nets(500, 501, env.NA))
    st = RolloutStorage(env, pa, T)
    written = list(env.written()) + list(rollout_written(st))
    assert any(x is env.obs_history for x in written)
    g, rewind = capture(lambda: env.rollout(pa, T, st), written)
    g.replay()
    g.replay()                                                          # 8 steps: the timeout of step 5 among them
    torch.cuda.synchronize()
    replayed = [x.clone() for x in written]
    assert st.done.sum() >= n
    rewind()
    env.rollout(pa, T, st)
    env.rollout(pa, T, st)
    torch.cuda.synchronize()
    for x, r in zip(written, replayed):
        assert same(x, r)


# ---------------------------------------------------------------------------- (7) a split batch
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_split_batch_keeps_the_histories_of_the_whole_batch(dtype):
    n, steps = 32, 12
    kw = dict(ENV, obs_history=dict(frames=3, sources=(("obs", 0, 6), ("obs", 9, 71), "priv")))
    whole = make_env(n, dtype, **kw)
    halves = [make_env(n // 2, dtype, **dict(kw, randomization=dict(NOISE, env_offset=off))) for off in (0, n // 2)]
    slices = (slice(0, n // 2), slice(n // 2, n))
    rows = lambda t, sl: t[:, sl] if t.dim() == 3 and t.shape[0] == 8 and t.shape[1] != 8 else t[sl]   # (the action ring is [8, N, NA])
    restarts = 0
    for t in range(steps):
        action = small(n, whole.NA, 700 + t, whole)
        if t in (3, 8):
            action[20, 0] = float("nan")
        whole.step(action)
        for h, sl in zip(halves, slices):
            h.step(action[sl].contiguous())
        torch.cuda.synchronize()
        restarts += int(whole.done.sum())
        for h, sl in zip(halves, slices):
            assert same(whole.obs_history[sl], h.obs_history), t
            for a, b in zip(whole.written(), h.written()):
                assert same(rows(a, sl), b), (t, tuple(a.shape))
    assert restarts >= 2 * n
