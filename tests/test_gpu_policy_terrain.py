"""Per-episode terrain and dynamics of the policy environment and its height scan on the GPU (PolicyEnv(terrain=...);
tsidb_policy_terrain_reset / tsidb_policy_height_scan): the kernels against the numpy restatement
(tests/policy_terrain_reference.py) from the device's own states, odd shapes, the sim reading the rewritten tables, off is off,
splittable and replayable draws, degenerate ranges and the C-ABI's errors.

Gates.  float64: 1e-12 * max(1, |x|) on every value of the two tables and of the scan (a draw is exact; around it are a
product-then-add that may contract to an FMA, a cos / sin, a square root and a division: a few ulp of values of at most 25);
which rows a step rewrote, which strips are raised and the rows of the other envs exact.  float32: the device against the float64
restatement fed the same float32 states; gate = 2 x the error the restatement run in np.float32 shows against its float64 self
on those states (computed in the test, printed).  A scan point whose float64 (direction . (X, Y) - phase) / L lies within 1e-9
(float64) / 1e-4 (float32) of a whole number may fall on either strip and is left out of the scan comparison - the restatement
alone decides which; at most 0.1 % / 1 % of the points may be."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_terrain_reference import PolicyTerrainReference  # noqa: E402
from policy_testlib import conf_of, host, make_env, rel, replay_against_eager, same  # noqa: E402
from test_gpu_policy_dr import CMD, DR, driven  # noqa: E402
from test_gpu_policy_env import ALL_WEIGHTS  # noqa: E402

pytestmark = pytest.mark.gpu

# everything on: 11 x 7 = 77 scan points (more than one wave of lanes), three levels
TER = dict(seed=5, mass=(0.9, 1.1), friction=(0.4, 1.0), tilt_deg=5.0, step_height=(0.005, 0.02), step_length=(0.04, 0.12), step_prob=0.5,
           flat_cells=1, num_levels=3, scan_x=(-0.5, 0.5, 11), scan_y=(-0.3, 0.3, 7), scan_clip=(0.1, 0.3), scan_noise=0.01)


def terrain_reference_of(env, dtype=np.float64):
    """the numpy restatement configured as env's library is (from the parameter vector it was given)"""
    from tsid_control_amd import _lib
    p = env.ter_params
    pair = lambda name: (p[getattr(_lib, "POL_TER_" + name + "_LO")], p[getattr(_lib, "POL_TER_" + name + "_HI")])
    nx, ny = int(p[_lib.POL_TER_SCAN_NX]), int(p[_lib.POL_TER_SCAN_NY])
    cfg = dict(seed=int(p[_lib.POL_TER_SEED]), env_offset=int(p[_lib.POL_TER_ENV_OFFSET]), mass=pair("MASS"), friction=pair("FRICTION"),
               tilt_max=p[_lib.POL_TER_TILT_MAX], step_height=pair("STEP_HEIGHT"), step_length=pair("STEP_LENGTH"), step_prob=p[_lib.POL_TER_STEP_PROB],
               flat_cells=int(p[_lib.POL_TER_FLAT_CELLS]), num_levels=int(p[_lib.POL_TER_NUM_LEVELS]),
               scan_x=(p[_lib.POL_TER_SCAN_X0], p[_lib.POL_TER_SCAN_X1], nx) if nx else None,
               scan_y=(p[_lib.POL_TER_SCAN_Y0], p[_lib.POL_TER_SCAN_Y1], ny) if ny else None, scan_clip=pair("SCAN_CLIP"),
               scan_noise=p[_lib.POL_TER_SCAN_NOISE])
    return PolicyTerrainReference(env.num_envs, cfg, dtype)


def off_boundary(frac, tol):
    """the scan points the comparison keeps: not within tol of a strip's edge"""
    return np.abs(frac - np.round(frac)) >= tol


# ---------------------------------------------------------------------------- (1) the kernels against the restatement
@pytest.mark.parametrize("dtype,v0", [("f64", False), ("f64", True), ("f32", False), ("f32", True)])
def test_kernels_match_the_numpy_restatement(dtype, v0):
    """32 envs x 60 policy steps, decimation 4, episodes of at most 11 steps, half of the envs driven hard with NaN-action
    restarts, the whole randomisation on (reset_xy = 0.5 and reset_yaw = pi move and turn the restarted robots), terrain_level =
    env % 3; the restatement follows the device's own qpos, done flags, episode and ep_len and keeps its own tables.
    Measured (MI355X), 192 restarts, 150 304 scan points, a compared point over a raised strip in all 32 envs.  float64, both
    robots: env_params 2.2e-16, terrain 2.5e-16, scan 5.6e-17, no point left out.  float32: env_params 5.5e-8 and terrain 5.4e-8,
    equal to the np.float32 restatement's (a draw is formed in float64 and cast once on both sides); scan 3.3e-8 against 3.5e-8
    of the restatement (v0 3.6e-8 / 3.5e-8), 31 (v0 26) points left out; the float32 gates are computed from the states of the
    run."""
    n, steps = 32, 60
    env = make_env(n, dtype, v0, decimation=4, action_scale=1.0, command_range=CMD, max_episode_steps=11, seed=11, randomization=DR,
                   terrain=TER, reward_weights=dict(track_lin_vel=1.0, alive=0.2, termination=-5.0))
    wc = env.wc
    assert env.height_scan.shape == (n, 77) and wc.env_params.shape == (n, 8) and wc.terrain.shape == (n, 20)
    torch.cuda.synchronize()
    tol = 1e-9 if dtype == "f64" else 1e-4
    ref = terrain_reference_of(env)
    low = terrain_reference_of(env, np.float32) if dtype == "f32" else None
    err = dict(env_params=0.0, terrain=0.0, scan=0.0)
    base = dict(err)
    seen = dict(restarts=0, points=0, left_out=0)
    raised_envs = set()

    def compare_tables(fresh, before):
        after = host(wc.env_params), host(wc.terrain)
        for a, b in zip(after, before):
            assert np.array_equal(a[~fresh], b[~fresh])                              # the other envs' rows: bit for bit
        assert np.array_equal((after[0] != before[0]).any(1), fresh) and np.array_equal((after[1] != before[1]).any(1), fresh)
        assert np.array_equal(after[1][:, 4:] != 0, ref.raised)                       # which strips are raised: exact
        err["env_params"], err["terrain"] = max(err["env_params"], rel(after[0], ref.env_params)), max(err["terrain"], rel(after[1], ref.terrain))
        if low is not None:
            base["env_params"] = max(base["env_params"], rel(low.env_params, ref.env_params))
            base["terrain"] = max(base["terrain"], rel(low.terrain, ref.terrain))

    def compare_scan():
        qpos, episode, ep_len = host(wc.qpos), host(env.episode), host(env.ep_len)
        s64, frac, over = ref.scan(qpos, episode, ep_len)
        keep = off_boundary(frac, tol)
        got = host(env.height_scan)
        err["scan"] = max(err["scan"], rel(got[keep], s64[keep]))
        seen["points"] += keep.size
        seen["left_out"] += int((~keep).sum())
        raised_envs.update(np.nonzero((keep & (over > 0)).any(1))[0].tolist())
        if low is not None:
            base["scan"] = max(base["scan"], rel(low.scan(qpos, episode, ep_len)[0][keep], s64[keep]))

    # the constructor's reset drew episode 1 for every env, at level 0, from the nominal tables
    nominal = ref.env_params.copy(), ref.terrain.copy()
    first = host(wc.qpos)
    for r in (ref, low):
        if r is not None:
            r.reset(np.ones(n), np.zeros(n, int), first, np.zeros(n, int))
    compare_tables(np.ones(n, bool), nominal)
    compare_scan()
    env.terrain_level.copy_(torch.arange(n, dtype=torch.int32, device=wc.device) % 3)
    level = host(env.terrain_level)
    for t in range(steps):
        action = driven(n, wc.NA, 100 + t, env, step=t)
        env._act(action)
        env._perturb()
        wc.sim_steps(env.decimation)
        env._reward()
        wc.reset_done()
        env._reset_noise()
        torch.cuda.synchronize()
        done, qpos, episode = host(env.done), host(wc.qpos), host(env.episode)
        before = host(wc.env_params), host(wc.terrain)
        env._terrain_reset()
        torch.cuda.synchronize()
        for r in (ref, low):
            if r is not None:
                fresh = r.reset(done, episode, qpos, level)
        seen["restarts"] += int(fresh.sum())
        compare_tables(fresh, before)
        env._obs()
        env._height_scan()
        torch.cuda.synchronize()
        assert np.array_equal(host(wc.qpos), qpos)                                    # neither kernel touches the state
        compare_scan()
    seen["raised_envs"] = len(raised_envs)
    print(f"policy terrain vs numpy, {dtype} v0={v0}: device", {k: f"{v:.3e}" for k, v in err.items()},
          "float32 numpy vs float64 numpy", {k: f"{v:.3e}" for k, v in base.items()}, seen)
    assert seen["restarts"] >= 50 and seen["raised_envs"] >= 10
    assert seen["left_out"] <= (0.001 if dtype == "f64" else 0.01) * seen["points"]
    for k, v in err.items():
        gate = 1e-12 if dtype == "f64" else 2 * base[k]
        assert v <= gate, (k, v, gate)


# ---------------------------------------------------------------------------- (2) odd shapes
def test_tail_workgroup_one_point_scan_and_padded_rows():
    """N = 5 (a workgroup with one env) with a 1 x 1 scan; N = 8 with 16 x 16 = 256 points (four passes of the lanes) into rows
    of 300 columns whose padding stays untouched"""
    env = make_env(5, randomization=dict(seed=3, reset_xy=0.5, reset_yaw=np.pi), terrain=dict(TER, scan_x=(0.1, 0.1, 1), scan_y=(-0.05, 0.0, 1)))
    torch.cuda.synchronize()
    ref = terrain_reference_of(env)
    ref.reset(np.ones(5), np.zeros(5, int), host(env.wc.qpos), np.zeros(5, int))
    assert env.height_scan.shape == (5, 1)
    assert rel(host(env.wc.env_params), ref.env_params) <= 1e-12 and rel(host(env.wc.terrain), ref.terrain) <= 1e-12
    s64, frac, _ = ref.scan(host(env.wc.qpos), host(env.episode), host(env.ep_len))
    assert off_boundary(frac, 1e-9).all() and rel(host(env.height_scan), s64) <= 1e-12

    n = 8
    env = make_env(n, randomization=dict(seed=3, reset_xy=0.5, reset_yaw=np.pi), terrain=dict(TER, scan_x=(-0.4, 0.4, 16), scan_y=(-0.4, 0.4, 16)))
    wc = env.wc
    wide = torch.full((n, 300), -7.0, dtype=wc.dtype, device=wc.device)
    wc._call("tsidb_policy_height_scan", C.byref(env._bufs), C.c_void_p(wc.qpos.data_ptr()), C.c_void_p(wide.data_ptr()), 300, wc._stream())
    torch.cuda.synchronize()
    assert env.height_scan.shape == (n, 256) and (wide[:, 256:] == -7.0).all() and torch.equal(wide[:, :256], env.height_scan)
    ref = terrain_reference_of(env)
    ref.reset(np.ones(n), np.zeros(n, int), host(wc.qpos), np.zeros(n, int))
    s64, frac, over = ref.scan(host(wc.qpos), host(env.episode), host(env.ep_len))
    keep = off_boundary(frac, 1e-9)
    assert (~keep).sum() <= 2 and rel(host(env.height_scan)[keep], s64[keep]) <= 1e-12 and (over > 0).any()


def test_scan_without_tables_is_the_clipped_base_height():
    """no table registered: the nominal floor; no randomisation needed.  Heights 0.31, 0.5 (clipped), NaN (passes)"""
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyTerrain
    n = 6
    env = make_env(n)
    wc = env.wc
    assert wc.env_params is None and wc.terrain is None
    p = PolicyTerrain(scan_x=(-0.5, 0.5, 9), scan_y=(-0.2, 0.2, 3), scan_clip=(0.0, 0.4)).params()
    wc._call("tsidb_policy_terrain_config", p.ctypes.data_as(C.c_void_p), _lib.POL_TER_NPARAMS)
    wc.qpos[:, 2] = torch.tensor([0.31, 0.5, float("nan"), 0.2, -0.1, 0.4], dtype=wc.dtype, device=wc.device)
    wc.qpos[3, 3:7] = torch.tensor([0.6, 0.0, 0.0, 0.8], dtype=wc.dtype, device=wc.device)     # a yaw: the same over a level floor
    scan = torch.full((n, 27), -7.0, dtype=wc.dtype, device=wc.device)
    wc._call("tsidb_policy_height_scan", C.byref(env._bufs), C.c_void_p(wc.qpos.data_ptr()), C.c_void_p(scan.data_ptr()), 27, wc._stream())
    torch.cuda.synchronize()
    want = torch.tensor([0.31, 0.4, float("nan"), 0.2, 0.0, 0.4], dtype=wc.dtype, device=wc.device)[:, None].expand(n, 27)
    assert same(scan, want)


# ---------------------------------------------------------------------------- (3) the sim reads what was written
def test_sim_steps_on_the_rewritten_tables():
    """a twin without terrain=, its own tables registered by hand (set_env_params) and the env's two tables copied into them
    device-to-device after every step: bit-identical qpos, qvel and contact lists over 40 steps with restarts"""
    n, steps = 16, 40
    kw = dict(decimation=5, action_scale=0.5, filter_alpha=0.6, max_episode_steps=9, command_range=CMD, seed=4,
              randomization=dict(seed=5, reset_xy=0.5, reset_yaw=np.pi, reset_joint_pos=0.05))
    env, twin = make_env(n, terrain=TER, **kw), make_env(n, **kw)
    twin.wc.set_env_params(mass_scale=1.0, terrain="flat")
    mirror = lambda: (twin.wc.env_params.copy_(env.wc.env_params), twin.wc.terrain.copy_(env.wc.terrain))
    mirror()
    assert (env.wc.env_params[:, 0] != 1).all() and (env.wc.env_params[:, 2] != 0).all() and (env.wc.terrain[:, 4:] != 0).any(1).sum() > n // 2
    restarts = 0
    for t in range(steps):
        action = driven(n, env.NA, 500 + t, env, step=t)
        env.step(action)
        twin.step(action)
        restarts += int(env.done.sum())
        for k in ("qpos", "qvel", "ncon", "con_pairs"):
            assert same(getattr(env.wc, k), getattr(twin.wc, k)), (t, k)
        assert torch.equal(env.done, twin.done)
        mirror()
        if t == 2:
            early = env.wc.qpos.clone()
    assert restarts >= 2 * n
    # and it matters: the same env on the nominal floor moves differently
    flat = make_env(n, **kw)
    for t in range(3):
        flat.step(driven(n, env.NA, 500 + t, env, step=t))
    assert not torch.equal(flat.wc.qpos, early)


def test_terrain_with_tsid_in_the_loop_steps_the_rewritten_tables():
    """tsid = "stand", residual mode: the closed-loop tick + sim reads the rewritten tables as the plain sim does - the same twin
    identity over 16 steps with restarts; the controller itself is not told about the floor"""
    from test_gpu_policy_tsid import TEACH
    n, steps = 16, 16
    kw = dict(decimation=4, mode="residual", action_scale=0.05, max_episode_steps=5, tsid="stand", teacher_weights=TEACH,
              randomization=dict(seed=5, reset_joint_pos=0.05))
    ter = dict(TER, tilt_deg=2.0, step_height=(0.0, 0.005))
    env, twin = make_env(n, conf_of(closed_loop=True), terrain=ter, **kw), make_env(n, conf_of(closed_loop=True), **kw)
    twin.wc.set_env_params(mass_scale=1.0, terrain="flat")
    mirror = lambda: (twin.wc.env_params.copy_(env.wc.env_params), twin.wc.terrain.copy_(env.wc.terrain))
    mirror()
    restarts = 0
    for t in range(steps):
        action = driven(n, env.NA, 700 + t, env, 0.5)
        out, _ = env.step(action), twin.step(action)
        assert sorted(out[3]) == ["env_params", "episode_length", "height_scan", "teacher_action", "teacher_obs", "teacher_terms", "terms",
                                  "terrain_level", "timeout"]
        restarts += int(env.done.sum())
        for k in ("qpos", "qvel", "ncon", "con_pairs", "tau"):
            assert same(getattr(env.wc, k), getattr(twin.wc, k)), (t, k)
        assert torch.equal(env.done, twin.done) and torch.equal(env.teacher_obs, twin.teacher_obs)
        assert bool(torch.isfinite(env.height_scan).all())
        mirror()
    assert restarts >= 3 * n and (env.wc.env_params[:, 2] != 0).all()


# ---------------------------------------------------------------------------- (4) off is off
def test_no_terrain_is_the_env_built_without_the_argument():
    n, steps = 32, 20
    kw = dict(decimation=5, action_scale=1.0, filter_alpha=0.8, command_range=CMD, max_episode_steps=8, reward_weights=ALL_WEIGHTS, seed=3,
              randomization=DR)
    plain, off = make_env(n, **kw), make_env(n, terrain=None, **kw)
    assert off.terrain is None and off.height_scan is None and off.wc.env_params is None and off.wc.terrain is None
    restarts = 0
    for t in range(steps):
        action = driven(n, plain.NA, 200 + t, plain, step=t)
        out_a, out_b = plain.step(action), off.step(action)
        assert sorted(out_a[3]) == sorted(out_b[3]) == ["episode_length", "push", "terms", "timeout"]
        restarts += int(plain.done.sum())
        for a, b in zip(out_a[:3], out_b[:3]):
            assert same(a, b), t
        for a, b in zip(plain.written(), off.written()):
            assert same(a, b), t
    assert restarts >= 2 * n and len(list(plain.written())) == len(list(off.written()))


# ---------------------------------------------------------------------------- (5) split and replay
def test_a_split_batch_draws_the_tables_and_the_scan_of_the_whole_batch():
    """32 envs against two runs of 16 with env_offset 0 / 16 (the terrain takes the randomisation's offset): every written
    tensor, the two tables and the scan among them, bit-identical"""
    n, steps = 32, 24
    kw = dict(decimation=4, action_scale=1.0, command_range=CMD, max_episode_steps=9, reward_weights=ALL_WEIGHTS, seed=13, terrain=TER)
    whole = make_env(n, randomization=DR, **kw)
    halves = [make_env(n // 2, randomization=dict(DR, env_offset=off), **kw) for off in (0, n // 2)]
    slices = (slice(0, n // 2), slice(n // 2, n))
    level = torch.arange(n, dtype=torch.int32, device=whole.device) % 3
    whole.terrain_level.copy_(level)
    for h, sl in zip(halves, slices):
        assert h.ter_params[1] == sl.start
        h.terrain_level.copy_(level[sl])
    rows = lambda t, sl: t[:, sl] if t.dim() == 3 and t.shape[0] == 8 and t.shape[1] != 8 else t[sl]
    restarts = 0
    for t in range(steps):
        action = driven(n, whole.NA, 400 + t, whole, step=t)
        whole.step(action)
        for h, sl in zip(halves, slices):
            h.step(action[sl].contiguous())
        torch.cuda.synchronize()
        restarts += int(whole.done.sum())
        for h, sl in zip(halves, slices):
            for a, b in zip(whole.written(), h.written()):
                assert same(rows(a, sl), b), (t, sl, tuple(a.shape))
    written = list(whole.written())
    assert restarts >= 2 * n and all(any(x is y for y in written) for x in (whole.wc.env_params, whole.wc.terrain, whole.height_scan))
    assert len({row.tobytes() for row in host(whole.wc.terrain)}) == n


def test_captured_step_with_a_terrain_replays_bit_identically():
    """step() with the randomisation and the terrain on, captured in a torch.cuda.graph; 16 replays against 16 eager steps of a
    twin, bit for bit, across restarts (timeouts at 7 and 14, NaN actions between)"""
    n, steps = 32, 16
    kw = dict(decimation=5, action_scale=1.0, filter_alpha=0.8, max_episode_steps=7, reward_weights=ALL_WEIGHTS, command_range=CMD,
              randomization=DR, terrain=TER)
    eager, env = make_env(n, **kw), make_env(n, **kw)
    for e in (eager, env):
        e.terrain_level.copy_(torch.arange(n, dtype=torch.int32, device=e.device) % 3)
    actions = [driven(n, env.NA, 900 + t, env, 0.5, step=t) for t in range(steps)]
    restarts = 0
    for t in replay_against_eager(env, eager, actions):
        restarts += int(env.done.sum())
    assert t == steps - 1 and restarts >= 2 * n


# ---------------------------------------------------------------------------- (6) degenerate ranges
def test_degenerate_ranges_write_their_value():
    """lo == hi everywhere, no tilt, no height: every restarted row is exactly (mass, friction, 0, 0, 1, 0, 0, 0), level"""
    n = 16
    env = make_env(n, decimation=4, max_episode_steps=3, randomization=dict(seed=2, reset_xy=0.5),
                   terrain=dict(mass=(1.05, 1.05), friction=(0.7, 0.7), tilt_deg=0.0, step_height=(0.0, 0.0), step_length=(0.1, 0.1), step_prob=1.0,
                                scan_x=(-0.2, 0.2, 3), scan_y=(0.0, 0.0, 1)))
    wc = env.wc
    zeros = torch.zeros(n, env.NA, dtype=wc.dtype, device=wc.device)
    row = torch.tensor([1.05, 0.7, 0, 0, 1, 0, 0, 0], dtype=wc.dtype, device=wc.device)
    for t in range(7):
        env.step(zeros)
        assert (wc.env_params == row).all() and (wc.terrain[:, 4:] == 0).all() and (wc.terrain[:, 3] == 1.0 / 0.1).all()
        assert torch.equal(env.height_scan, wc.qpos[:, 2:3].expand(n, 3))
    assert int(env.episode.min()) >= 3
    assert len({float(x) for x in wc.terrain[:, 2]}) == n           # (the phase follows the randomised position)


# ---------------------------------------------------------------------------- (7) errors
def test_calls_are_rejected_with_a_message():
    """the library's own checks (PolicyTerrain checks the same on the host first): a rejected vector changes nothing, a reset
    needs both tables and a configuration, NULL / 0 switches everything off again"""
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_env import PolicyTerrain
    n = 4
    env = make_env(n, decimation=4, terrain=dict(TER, scan_noise=0.0))
    wc, vp = env.wc, C.c_void_p
    config = lambda p, k=_lib.POL_TER_NPARAMS: wc._call("tsidb_policy_terrain_config", p.ctypes.data_as(vp) if p is not None else None, k)
    good = env.ter_params.copy()

    def changed(**kw):
        p = good.copy()
        for k, v in kw.items():
            p[getattr(_lib, "POL_TER_" + k)] = v
        return p
    bad = [changed(TILT_MAX=float("nan")), changed(MASS_HI=float("inf")), changed(MASS_LO=2.0), changed(FRICTION_LO=0.0), changed(MASS_LO=-1.0),
           changed(TILT_MAX=np.pi / 4), changed(TILT_MAX=-0.1), changed(STEP_HEIGHT_LO=-0.01), changed(STEP_HEIGHT_LO=0.5), changed(STEP_LENGTH_LO=0.0),
           changed(STEP_LENGTH_LO=1.0), changed(STEP_PROB=1.01), changed(STEP_PROB=-0.01), changed(FLAT_CELLS=0.5), changed(FLAT_CELLS=8),
           changed(NUM_LEVELS=0), changed(NUM_LEVELS=1.5), changed(SEED=2.0 ** 32), changed(SEED=0.5), changed(ENV_OFFSET=2.0 ** 31),
           changed(SCAN_NX=17, SCAN_NY=16), changed(SCAN_NX=0), changed(SCAN_NY=0), changed(SCAN_NX=2.5), changed(SCAN_CLIP_LO=2.0),
           changed(SCAN_NOISE=-0.1)]
    for p in bad:
        with pytest.raises(_lib.TsidbError, match="tsidb_policy_terrain_config"):
            config(p)
    with pytest.raises(_lib.TsidbError, match="TSIDB_POL_TER_NPARAMS"):
        config(good, _lib.POL_TER_NPARAMS - 1)
    with pytest.raises(_lib.TsidbError, match="TSIDB_POL_TER_NPARAMS"):
        config(None, 3)
    # nothing of the rejected vectors was taken: a step draws what a twin draws
    twin = make_env(n, decimation=4, terrain=dict(TER, scan_noise=0.0))
    zeros = torch.zeros(n, env.NA, dtype=wc.dtype, device=wc.device)
    env.reset()
    twin.reset()
    env.step(zeros)
    twin.step(zeros)
    assert torch.equal(wc.terrain, twin.wc.terrain) and torch.equal(wc.env_params, twin.wc.env_params) and torch.equal(env.height_scan, twin.height_scan)
    args = lambda: (C.byref(env._bufs), vp(wc.rows.data_ptr()), wc.NROW, vp(wc.qpos.data_ptr()), vp(env.terrain_level.data_ptr()), wc._stream())
    with pytest.raises(_lib.TsidbError, match="TSIDB_NROW"):
        wc._call("tsidb_policy_terrain_reset", C.byref(env._bufs), vp(wc.rows.data_ptr()), 3, vp(wc.qpos.data_ptr()), None, wc._stream())
    with pytest.raises(_lib.TsidbError, match="null buffer"):
        wc._call("tsidb_policy_terrain_reset", C.byref(env._bufs), vp(wc.rows.data_ptr()), wc.NROW, None, None, wc._stream())
    with pytest.raises(_lib.TsidbError, match="scan row stride"):
        wc._call("tsidb_policy_height_scan", C.byref(env._bufs), vp(wc.qpos.data_ptr()), vp(env.height_scan.data_ptr()), 76, wc._stream())
    # level NULL = the top level: what level num_levels - 1 draws
    wc.done.fill_(1)
    wc._call("tsidb_policy_terrain_reset", C.byref(env._bufs), vp(wc.rows.data_ptr()), wc.NROW, vp(wc.qpos.data_ptr()), None, wc._stream())
    top = wc.terrain.clone()
    env.terrain_level.fill_(7)                              # (clamped to num_levels - 1)
    wc._call("tsidb_policy_terrain_reset", *args())
    torch.cuda.synchronize()
    assert torch.equal(top, wc.terrain) and not torch.equal(top, twin.wc.terrain)
    wc.done.zero_()
    # one table alone is not enough; none neither
    tables = wc.env_params, wc.terrain
    wc._call("tsidb_set_env_params", vp(tables[0].data_ptr()), None)
    with pytest.raises(_lib.TsidbError, match="both the env_params and the terrain table"):
        wc._call("tsidb_policy_terrain_reset", *args())
    wc._call("tsidb_set_env_params", vp(tables[0].data_ptr()), vp(tables[1].data_ptr()))
    wc._call("tsidb_policy_terrain_reset", *args())
    config(None, 0)                                        # everything off again
    with pytest.raises(_lib.TsidbError, match="call tsidb_policy_terrain_config first"):
        wc._call("tsidb_policy_terrain_reset", *args())
    scan = torch.full((n, 77), -7.0, dtype=wc.dtype, device=wc.device)
    wc._call("tsidb_policy_height_scan", C.byref(env._bufs), vp(wc.qpos.data_ptr()), vp(scan.data_ptr()), 77, wc._stream())
    torch.cuda.synchronize()
    assert (scan == -7.0).all()                            # no scan configured: nothing launched
    assert PolicyTerrain.of(TER).params().shape == good.shape
