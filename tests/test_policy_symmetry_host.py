"""PolicySymmetry without a GPU: the actuator tables of both model blobs, checked against the oracle's sim - a position target on
one actuator against the mirrored target, in free fall - the observation's column tables checked on the same probes through the
numpy restatement of the observation (tests/policy_reference.py), the assembly of a network's table from its input blocks, what
is rejected, and the launches a PolicyLearner with a symmetry makes."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_reference import PolicyReference  # noqa: E402
from policy_testlib import assert_prototypes, header_enums  # noqa: E402
from test_policy_actor_host import actor_env, mlp  # noqa: E402

# the tables PolicySymmetry must derive from the blobs' geometry (mirror normal: the base x axis)
TABLES = {
    False: ([6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5, 15, 16, 17, 12, 13, 14, 18, 19], [-1.0] * 19 + [1.0]),
    True: ([3, 4, 5, 0, 1, 2, 6, 7, 13, 14, 15, 16, 17, 8, 9, 10, 11, 12], [1.0] * 6 + [-1.0, 1.0] + [-1.0] * 10),
}
STEPS, TARGET = 25, 0.3


def blob_of(v0):
    from tsid_control_amd import op3_v0_conf
    from tsid_control_amd.model import ModelBlob
    return ModelBlob(op3_v0_conf().model_blob if v0 else None)


@pytest.mark.parametrize("v0", [False, True])
def test_actuator_tables_are_the_pinned_involutions(v0):
    from tsid_control_amd.policy_symmetry import actuator_table
    perm, sign, n = actuator_table(blob_of(v0))
    assert perm.dtype == np.int32 and sign.dtype == np.float32
    assert perm.tolist() == TABLES[v0][0] and sign.tolist() == TABLES[v0][1] and n.tolist() == [1.0, 0.0, 0.0]
    assert np.array_equal(perm[perm], np.arange(len(perm))) and np.array_equal(sign[perm], sign)


def test_a_tree_that_is_not_symmetric_is_rejected():
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_symmetry import actuator_table
    blob = blob_of(False)
    model = {k: np.array(blob[k], dtype=np.float64 if k in ("mj_pos", "mj_quat") else np.int64) for k in ("mj_parent", "mj_pos", "mj_quat", "mj_act_dof")}
    nb = len(model["mj_parent"])
    quat = model["mj_quat"].reshape(nb, 4)
    quat[3] = [np.sqrt(0.5), np.sqrt(0.5), 0.0, 0.0]      # one leg joint turned about x: its chain has no partner any more
    with pytest.raises(_lib.TsidbError, match="PolicySymmetry: "):
        actuator_table(model)


# ---------------------------------------------------------------------------- the oracle probes
def _probe(orc, blob, target, self_collision=True):
    """the sim state after STEPS steps from the zero pose in free fall with a constant position target"""
    nq, nv = int(blob["model_dims"][1]), int(blob["model_dims"][2])
    qpos, qvel, ws = np.zeros(nq), np.zeros(nv), np.zeros(nv)
    qpos[2], qpos[3] = 2.0, 1.0
    for _ in range(STEPS):
        r = orc.sim_step(qpos, qvel, target, ws, self_collision=self_collision)
        assert r["rc"] == 0 and (self_collision or r["ncon"] == 0)
    return qpos, qvel


@pytest.fixture(scope="module", params=[False, True], ids=["v1", "v0"])
def probes(request):
    """per actuator a: the states of target +TARGET on a, of the mirrored target, and of the mirrored target with sign[a] flipped;
    and the first two again with the sim's self-collision off (`free`: no contact of any kind)"""
    from oracle.oracle import Oracle, build
    from tsid_control_amd.policy_symmetry import actuator_table
    v0 = request.param
    build()
    blob = blob_of(v0)
    orc = Oracle(blob.raw)
    perm, sign, n = actuator_table(blob)
    sign = sign.astype(np.float64)
    na = len(perm)
    runs, free = [], []
    for a in range(na):
        t = np.zeros(na)
        t[a] = TARGET
        tm = sign * t[perm]                                  # mirror_action(t)
        assert tm[perm[a]] == sign[a] * TARGET and np.count_nonzero(tm) == 1
        runs.append((_probe(orc, blob, t), _probe(orc, blob, tm), _probe(orc, blob, -tm)))
        free.append((_probe(orc, blob, t, False), _probe(orc, blob, tm, False)))
    return v0, blob, perm, sign, n, runs, free


def test_a_mirrored_target_gives_the_mirrored_motion(probes):
    """residual = the mismatch of one run's joint positions and the mirror of the other's; with the table's sign against with
    sign[a] flipped: at most 1/4 for every actuator (a wrong sign or pair gives a ratio of order 1)"""
    v0, blob, perm, sign, n, runs, _ = probes
    dof = np.asarray(blob["mj_act_dof"]).astype(np.int64)
    worst = 0.0
    for a, ((qa, _), (qb, _), (qf, _)) in enumerate(runs):
        ja, jb, jf = qa[dof + 1], qb[dof + 1], qf[dof + 1]
        res, flipped = np.abs(ja - sign * jb[perm]).max(), np.abs(ja - sign * jf[perm]).max()
        print(f"{'v0' if v0 else 'v1'} actuator {a}: residual {res:.3g}, with the sign flipped {flipped:.3g}, ratio {res / flipped:.3g}")
        assert flipped > 0 and res <= 0.25 * flipped, a
        worst = max(worst, res / flipped)
    print("worst ratio", worst)


def test_the_observation_tables_mirror_the_probes_rows(probes):
    """obs and priv rows of the probes' states by the numpy restatement: per column the largest residual over the probes is at
    most 1/4 of the largest |value|.  Skipped, their largest value below 1e-6: the contact flags (in the air), the command and the
    last action (inputs, not dynamics) - checked against their definition below.
    The probes of this test run with the sim's self-collision off.  Free fall is there to keep contact out of the probes, and at
    the zero pose of the v1 robot two probes still make contact: the arm of actuator 16 and the legs of actuator 1 (hip roll)
    touch the body, and the sim's contacts of the two sides are not mirror images (joint velocity of actuator 16: 1.44 rad/s in
    one run, 0.94 rad/s in its mirror).  Measured, worst share over the columns: v1 0.0079 (0.345 at the joint velocity of
    actuator 16 with self-collision on, 0.295 at that of actuator 5, 0.24 at the angular velocity's y), v0 4.5e-5 (0.0012)."""
    from tsid_control_amd import policy_symmetry as PS
    v0, blob, perm, sign, n, _, runs = probes
    na = len(perm)
    nobs = 11 + 3 * na
    dof = np.asarray(blob["mj_act_dof"]).astype(np.int64)
    ref = PolicyReference(1, dof, np.asarray(blob["mj_geom_body"]), (1, 2), np.ones(na), np.zeros(na))
    none = np.zeros((1, 32), dtype=np.int32)
    row = lambda s: ref.obs_stage(np.zeros(1), s[0][None], s[1][None], np.zeros(1, dtype=np.int32), none)[0].copy()
    act = (perm.astype(np.int64), sign)
    op, osg = PS._cat(PS.obs_table(n, act), PS.priv_table(n))
    assert len(op) == nobs + 4
    A = np.stack([row(r[0]) for r in runs])
    B = np.stack([row(r[1]) for r in runs])
    res = np.abs(A - osg * B[:, op]).max(0)
    big = np.maximum(np.abs(A).max(0), np.abs(B).max(0))
    skipped = np.flatnonzero(big < 1e-6)
    allowed = set(range(6, 9)) | set(range(9 + 2 * na, 11 + 3 * na))        # command, last action, the two flags
    assert set(skipped.tolist()) <= allowed, skipped
    share = res / np.where(big < 1e-6, 1.0, big)
    share[skipped] = 0.0
    print(f"{'v0' if v0 else 'v1'}: worst share {share.max():.3g} at column {int(share.argmax())}, skipped {skipped.tolist()}")
    assert share.max() <= 0.25
    # the skipped columns by their definition: LF / RF swap, (vx, vy) polar and the yaw rate flips, last action = the actuator table
    assert op[nobs - 2:nobs].tolist() == [nobs - 1, nobs - 2] and osg[nobs - 2:nobs].tolist() == [1.0, 1.0]
    assert op[6:9].tolist() == [6, 7, 8] and osg[6:9].tolist() == [-1.0, 1.0, -1.0]
    for base in (9, 9 + na, 9 + 2 * na):
        assert (op[base:base + na] - base).tolist() == perm.tolist() and osg[base:base + na].tolist() == sign.tolist()
    assert osg[0:6].tolist() == [1.0, -1.0, -1.0, -1.0, 1.0, 1.0]            # angular velocity axial, gravity polar
    assert osg[nobs:].tolist() == [-1.0, 1.0, 1.0, 1.0] and op[nobs:].tolist() == list(range(nobs, nobs + 4))


# ---------------------------------------------------------------------------- assembly
def sym_env(n=3, scan=(7, 11, -0.3, 0.3, -0.5, 0.5)):
    from tsid_control_amd import _lib
    env, calls = actor_env(n)
    ter = np.zeros(_lib.POL_TER_NPARAMS)
    ter[[_lib.POL_TER_SCAN_NX, _lib.POL_TER_SCAN_NY, _lib.POL_TER_SCAN_X0, _lib.POL_TER_SCAN_X1, _lib.POL_TER_SCAN_Y0, _lib.POL_TER_SCAN_Y1]] = scan
    env.ter_params = ter
    env.height_scan = torch.zeros(n, int(scan[0] * scan[1]), dtype=torch.float64)
    return env, calls


def is_involution(perm, sign):
    perm, sign = perm.long(), sign
    return torch.equal(perm[perm], torch.arange(len(perm))) and torch.equal(sign[perm], sign) and bool((sign.abs() == 1).all())


def test_a_three_block_input_and_the_mirror_is_an_involution_bit_for_bit():
    import tsid_control_amd
    from tsid_control_amd import PolicyActor
    from tsid_control_amd.policy_symmetry import PolicySymmetry
    assert tsid_control_amd.PolicySymmetry is PolicySymmetry
    env, _ = sym_env()
    NA, nobs = env.NA, env.NOBS
    K = nobs + 77 + 3
    pa = PolicyActor(env, mlp(K, 8, NA), mlp(nobs + 4 + 14 + NA, 8, 1), actor_inputs=("obs", "height_scan", "command"),
                     critic_inputs=("obs", "priv", "teacher_obs"))
    sy = PolicySymmetry(env, pa)
    assert sy.actor_perm.dtype == torch.int32 and sy.actor_sign.dtype == torch.float32 and sy.actor_perm.shape == (K,)
    assert sy.critic_perm.shape == (nobs + 4 + 14 + NA,) and sy.action_perm.tolist() == TABLES[False][0] and sy.action_sign.tolist() == TABLES[False][1]
    for p, s in ((sy.actor_perm, sy.actor_sign), (sy.critic_perm, sy.critic_sign), (sy.action_perm, sy.action_sign)):
        assert is_involution(p, s)
    # every block's perm stays inside the block
    for lo, hi in ((0, nobs), (nobs, nobs + 77), (nobs + 77, K)):
        assert int(sy.actor_perm[lo:hi].min()) >= lo and int(sy.actor_perm[lo:hi].max()) < hi
    # the scan: point ix * ny + iy, the index along x reverses; the command block as inside obs
    ix, iy = np.divmod(np.arange(77), 11)
    assert (sy.actor_perm[nobs:nobs + 77] - nobs).tolist() == ((6 - ix) * 11 + iy).tolist() and bool((sy.actor_sign[nobs:nobs + 77] == 1).all())
    assert torch.equal(sy.actor_sign[nobs + 77:], sy.actor_sign[6:9]) and sy.actor_sign[6:9].tolist() == [-1.0, 1.0, -1.0]
    # teacher_obs: contact_active swaps, CoM error and velocity polar, the foot errors swap and are polar, tau the actuator table
    t0 = nobs + 4
    tp, ts = (sy.critic_perm[t0:] - t0).tolist(), sy.critic_sign[t0:].tolist()
    assert tp[:14] == [1, 0, 2, 3, 4, 5, 6, 7, 11, 12, 13, 8, 9, 10] and ts[:14] == [1, 1] + [-1, 1, 1] * 4
    assert tp[14:] == [14 + p for p in TABLES[False][0]] and ts[14:] == TABLES[False][1]
    g = torch.Generator().manual_seed(0)
    for which, k in (("actor", K), ("critic", nobs + 4 + 14 + NA)):
        x = torch.randn(5, k, generator=g)
        m = sy.mirror_obs(x, which)
        assert not torch.equal(m, x) and torch.equal(sy.mirror_obs(m, which), x)
    a = torch.randn(2, 3, NA, generator=g, dtype=torch.float64)
    assert torch.equal(sy.mirror_action(sy.mirror_action(a)), a) and torch.equal(sy.mirror_action(a)[..., 19], a[..., 19])
    assert torch.equal(sy.mirror_action(a)[..., 0], -a[..., 6])


def history_env(sources, frames=2):
    from tsid_control_amd.policy_env import PolicyObsHistory
    env, calls = sym_env()
    env.obs_history_spec = PolicyObsHistory(frames, sources)
    env.obs_history_sources = env.obs_history_spec.resolve(dict(obs=env.NOBS, priv=4, command=3, height_scan=77, teacher_obs=14 + env.NA))
    k = sum(hi - lo for _, lo, hi in env.obs_history_sources)
    env.obs_history = torch.zeros(env.num_envs, frames * k, dtype=torch.float64)
    return env, k


def test_a_history_over_a_column_range_and_what_is_rejected():
    from tsid_control_amd import PolicyActor, PolicyLearner, PolicyNormalizer, _lib
    from tsid_control_amd.policy_symmetry import PolicySymmetry
    # two frames of (angular velocity + gravity, the joint positions): both ranges are closed under the mirror
    env, k = history_env([("obs", 0, 6), ("obs", 9, 9 + 20)])
    assert k == 26
    pa = PolicyActor(env, mlp(2 * k, 8, env.NA), actor_inputs=("obs_history",))
    sy = PolicySymmetry(env, pa)
    frame = list(range(6)) + [6 + p for p in TABLES[False][0]]
    assert sy.actor_perm.tolist() == frame + [k + c for c in frame]
    assert sy.actor_sign.tolist() == ([1.0, -1.0, -1.0, -1.0, 1.0, 1.0] + TABLES[False][1]) * 2 and sy.critic_perm is None
    # a range that cuts a pair of legs apart
    env, k = history_env([("obs", 9, 9 + 6)])
    pa = PolicyActor(env, mlp(2 * k, 8, env.NA), actor_inputs=("obs_history",))
    with pytest.raises(_lib.TsidbError, match="PolicySymmetry: obs_history source obs: the column range \\(9, 15\\) is not closed under the mirror"):
        PolicySymmetry(env, pa)
    # a scan grid that is not symmetric along the mirror normal (y may be: the normal is x)
    env, _ = sym_env(scan=(7, 11, -0.2, 0.3, -0.1, 0.5))
    pa = PolicyActor(env, mlp(env.NOBS + 77, 8, env.NA), actor_inputs=("obs", "height_scan"))
    with pytest.raises(_lib.TsidbError, match="PolicySymmetry: height_scan: the grid must be symmetric about 0"):
        PolicySymmetry(env, pa)
    env, _ = sym_env(scan=(7, 11, -0.3, 0.3, -0.1, 0.5))
    PolicySymmetry(env, PolicyActor(env, mlp(env.NOBS + 77, 8, env.NA), actor_inputs=("obs", "height_scan")))
    # a raw tensor needs its table, of its size, an involution inside the block
    env, _ = sym_env()
    raw = torch.zeros(env.num_envs, 4, dtype=torch.float64)
    pa = PolicyActor(env, mlp(env.NOBS + 4, 8, env.NA), mlp(4, 8, 1), actor_inputs=("obs", raw), critic_inputs=(raw,))
    with pytest.raises(_lib.TsidbError, match="PolicySymmetry: actor input block 1 is a raw \\[N, 4\\] tensor: give its table"):
        PolicySymmetry(env, pa)
    for table, msg in ((([1, 0, 2], [1, 1, 1]), "a table of 3 columns for a block of 4"), (([1, 2, 0, 3], [1, 1, 1, 1]), "is not an involution"),
                       (([1, 0, 2, 3], [1, -1, 1, 1]), "is not an involution"), (([1, 0, 2, 4], [1, 1, 1, 1]), "perm must stay inside its block"),
                       (([1, 0, 2, 3], [1, 1, 0.5, 1]), "sign must be")):
        with pytest.raises(_lib.TsidbError, match="PolicySymmetry: .*" + msg):
            PolicySymmetry(env, pa, blocks={1: table, ("critic", 0): ([0, 1, 2, 3], [1, 1, 1, 1])})
    sy = PolicySymmetry(env, pa, blocks={("actor", 1): ([1, 0, 2, 3], [-1, -1, 1, -1]), ("critic", 0): ([0, 1, 3, 2], [1, 1, 1, 1])})
    assert (sy.actor_perm[env.NOBS:] - env.NOBS).tolist() == [1, 0, 2, 3] and sy.critic_perm.tolist() == [0, 1, 3, 2]
    # a normaliser; the imitation term; another actor's symmetry; a coefficient without a symmetry
    other = PolicyActor(env, mlp(env.NOBS, 8, env.NA))
    with pytest.raises(_lib.TsidbError, match="PolicyLearner: symmetry must be a PolicySymmetry of this learner's actor"):
        PolicyLearner(other, symmetry=sy)
    osy = PolicySymmetry(env, other)
    for kw, msg in ((dict(imitation_coef=0.5), "imitation term"), (dict(surrogate_coef=0.0), "imitation term"),
                    (dict(mirror_coef=-1.0), "mirror_coef must be >= 0"), (dict(symmetry_augment=1), "symmetry_augment must be a bool")):
        with pytest.raises(_lib.TsidbError, match="PolicyLearner: .*" + msg):
            PolicyLearner(other, symmetry=osy, **kw)
    with pytest.raises(_lib.TsidbError, match="PolicyLearner: mirror_coef needs a symmetry"):
        PolicyLearner(other, mirror_coef=0.5)
    normed = PolicyActor(env, mlp(env.NOBS, 8, env.NA), normalizer=PolicyNormalizer())
    with pytest.raises(_lib.TsidbError, match="PolicySymmetry: an actor with a PolicyNormalizer is not supported"):
        PolicySymmetry(env, normed)


# ---------------------------------------------------------------------------- the binding and the launches
def test_binding_matches_the_header_and_backward_goes_through_the_sym_entry():
    import re
    from policy_testlib import HEADER
    from tsid_control_amd import PolicyActor, PolicyLearner, RolloutStorage, _lib
    from tsid_control_amd.policy_symmetry import PolicySymmetry
    assert len(_lib.POL_SYM_STATS) == header_enums("TSIDB_POL_SYM_")["TSIDB_POL_SYM_NSTATS"] == 2
    m = re.search(r"typedef struct tsidb_policy_symmetry \{(.*?)\} tsidb_policy_symmetry;", HEADER, re.S)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f[0] for f in _lib.PolicySymmetryTables._fields_] and C.sizeof(_lib.PolicySymmetryTables) == 6 * 8 + 4 + 4 + 8
    assert_prototypes(("tsidb_policy_learn_sym_workspace", "tsidb_policy_learn_sym"))
    env, calls = sym_env()
    pa = PolicyActor(env, mlp(env.NOBS, 8, env.NA), mlp(env.NOBS + 4, 8, 1), critic_inputs=("obs", "priv"))
    st = RolloutStorage(env, pa, 2)
    st.gae()
    sy = PolicySymmetry(env, pa)
    index = torch.tensor([4, 0, 5, 5], dtype=torch.int32)
    # symmetry = None: the parent's calls
    del calls[:]
    PolicyLearner(pa).backward(st, index)
    assert [c[0] for c in calls] == ["tsidb_policy_learn_workspace", "tsidb_policy_learn"]
    del calls[:]
    pl = PolicyLearner(pa, symmetry=sy, symmetry_augment=False, mirror_coef=0.25)
    pl.backward(st, index)
    assert [c[0] for c in calls] == ["tsidb_policy_learn_sym_workspace", "tsidb_policy_learn_sym"]
    a = calls[1][1]
    assert len(a) == 13
    t = C.cast(a[8], C.POINTER(_lib.PolicySymmetryTables)).contents
    assert (t.actor_perm, t.actor_sign, t.critic_perm, t.critic_sign, t.action_perm, t.action_sign, t.stats) == \
        tuple(x.data_ptr() for x in (sy.actor_perm, sy.actor_sign, sy.critic_perm, sy.critic_sign, sy.action_perm, sy.action_sign, pl.sym_stats))
    assert (t.augment, t.mirror_coef) == (0, 0.25) and pl.sym_stats.shape == (2,)
    assert a[9].value == pl.workspace.data_ptr() and a[11].value == pl.stats.data_ptr()
    assert id(pl.sym_stats) in {id(x) for x in pl.written()}
    assert C.cast(PolicyLearner(pa, symmetry=sy).backward(st, index) is not None and calls[-1][1][8], C.POINTER(_lib.PolicySymmetryTables)).contents.augment == 1
