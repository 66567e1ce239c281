"""tests/policy_teacher_reference.py, the numpy restatement of tsidb_policy_teacher / tsidb_policy_teacher_obs, pinned by
hand-made states whose results are known in closed form; no GPU.  It is also the first user of PolicyEnv's tsid arguments that
needs no device: the argument checks run before anything is built."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_teacher_reference import TEACH_TERMS, TeacherReference, foot_contacts  # noqa: E402

NQ, NV, NA = 27, 26, 20
QIDX = np.array([7 + (3 * a + 5) % NA for a in range(NA)])     # a permutation: actuator a drives TSID joint (3 a + 5) % 20
GEOM_BODY = np.arange(21)                                       # one geom per body
FEET = (6, 12)


def make(mode="residual", n=4, **kw):
    kw.setdefault("scale", np.full(NA, 0.5))
    kw.setdefault("default", np.zeros(NA))
    ref = TeacherReference(QIDX, GEOM_BODY, FEET, kw.pop("scale"), kw.pop("default"), nq=NQ, nv=NV, mode=mode, **kw)
    s = dict(rows=np.zeros((n, NQ + NV + 14)), q=np.zeros((n, NQ)), tau=np.zeros((n, NA)), status=np.zeros(n, np.int32), ctrl=np.zeros((n, NA)),
             ncon=np.full(n, 2, np.int32), con_pairs=np.full((n, 32), -1, np.int32), com_ref=np.zeros((n, 9)), foot_ref=np.zeros((n, 2, 24)),
             contact_active=np.ones((n, 2), np.uint8), reward=np.zeros(n), done=np.zeros(n), timeout=np.zeros(n, np.int32), terms=np.zeros((n, 12)))
    s["con_pairs"][:, 0], s["con_pairs"][:, 1] = (FEET[0] << 16) | 3, (FEET[1] << 16) | 5     # both soles on the floor
    s["rows"][:, NQ + NV:NQ + NV + 3] = s["com_ref"][:, :3] = (0.01, -0.02, 0.24)
    s["rows"][:, NQ + NV + 6:NQ + NV + 9] = s["foot_ref"][:, 0, :3] = (0.0, 0.04, 0.0)
    s["rows"][:, NQ + NV + 9:NQ + NV + 12] = s["foot_ref"][:, 1, :3] = (0.0, -0.04, 0.0)
    return ref, s


def test_everything_on_its_reference_scores_full_marks():
    ref, s = make(weights=dict(track_com=2.0, track_feet=3.0, contact_match=0.5, deviation=-1.0))
    s["reward"][:] = 0.25
    out = ref.teacher(**s)
    assert np.array_equal(out["teacher_terms"], np.tile([1.0, 1.0, 2.0, 0.0], (4, 1)))
    assert np.array_equal(out["reward"], np.full(4, 0.25 + 2 + 3 + 1))
    assert not out["done"].any() and not out["timeout"].any() and not out["terms"].any() and not out["teacher_action"].any()
    assert TEACH_TERMS == ("track_com", "track_feet", "contact_match", "deviation")


def test_a_foot_three_centimetres_off_and_a_com_one_sigma_off():
    ref, s = make(sigma_com=0.05, sigma_foot=0.05)
    s["rows"][1, NQ + NV + 9 + 1] += 0.03            # env 1: the right foot 3 cm to the side
    s["rows"][2, NQ + NV + 2] -= 0.05                # env 2: the CoM one sigma low
    s["rows"][3, NQ + NV + 6] += 0.03                # env 3: both feet 3 cm off, in different directions
    s["rows"][3, NQ + NV + 9 + 2] += 0.03
    t = ref.teacher(**s)["teacher_terms"]
    assert t[0, 0] == 1 and t[0, 1] == 1
    assert abs(t[1, 1] - np.exp(-0.36)) < 1e-15 and t[1, 0] == 1
    assert abs(t[2, 0] - np.exp(-1.0)) < 1e-15 and t[2, 1] == 1
    assert abs(t[3, 1] - np.exp(-0.72)) < 1e-15
    # the reference's velocity and orientation columns play no part
    s["foot_ref"][:, :, 3:] = 7.0
    s["com_ref"][:, 3:] = -3.0
    assert np.array_equal(ref.teacher(**s)["teacher_terms"], t)


def test_contact_match_counts_the_feet_that_agree():
    ref, s = make()
    s["contact_active"][1] = (1, 0)                  # env 1: TSID has lifted the right foot, the sim still has it down
    s["contact_active"][2] = (0, 0)                  # env 2: both wrong
    s["con_pairs"][3, 0] = (5 << 16) | 1             # env 3: the left sole is off the floor (a shin contact instead): one wrong
    t = ref.teacher(**s)["teacher_terms"]
    assert t[:, 2].tolist() == [2, 1, 0, 1]
    # rows beyond ncon, robot<->robot rows and empty rows are no floor contacts
    s["ncon"][0] = 1
    assert foot_contacts(s["ncon"], s["con_pairs"], GEOM_BODY, FEET)[0].tolist() == [True, False]
    s["ncon"][0] = 2
    s["con_pairs"][0, 1] = (FEET[1] << 16) | 0x8000 | 4
    assert foot_contacts(s["ncon"], s["con_pairs"], GEOM_BODY, FEET)[0].tolist() == [True, False]
    assert ref.teacher(**s)["teacher_terms"][0, 2] == 1


@pytest.mark.parametrize("mode", ["residual", "motor", "position"])
def test_deviation_and_teacher_action(mode):
    scale = np.full(NA, 0.5)
    scale[4] = 0.0                                   # an actuator the policy does not drive
    default = np.linspace(-0.1, 0.1, NA)
    ref, s = make(mode, scale=scale, default=default, clip=2.0)
    rng = np.random.default_rng(3)
    s["tau"][:] = rng.uniform(-0.8, 0.8, (4, NA))
    s["q"][:, 7:] = rng.uniform(-0.5, 0.5, (4, NA))
    s["ctrl"][:] = rng.uniform(-0.3, 0.3, (4, NA))
    s["tau"][0, QIDX[7] - 7] = 5.0                   # (5 - default) / 0.5 is past the clip
    s["q"][0, QIDX[7]] = -5.0
    out = ref.teacher(**s)
    ta = s["tau"][:, QIDX - 7]
    assert np.array_equal(ref.tau_act(s["tau"]), ta)
    if mode == "residual":
        assert np.allclose(out["teacher_terms"][:, 3], (s["ctrl"] ** 2).sum(1), rtol=1e-15) and not out["teacher_action"].any()
        return
    want = (ta if mode == "motor" else s["q"][:, QIDX]) - default
    assert np.allclose(out["teacher_terms"][:, 3], ((s["ctrl"] - ta) ** 2).sum(1) if mode == "motor" else 0.0, rtol=1e-15)
    act = out["teacher_action"]
    assert (act[:, 4] == 0).all() and act[0, 7] == (2.0 if mode == "motor" else -2.0)
    on = np.ones(NA, bool)
    on[4] = False
    inside = on[None, :] & (np.abs(want / 0.5) <= 2.0)
    # the action reproduces TSID's command through the action map default + scale * action
    assert np.allclose((default + scale * act)[inside], (want + default)[inside], rtol=0, atol=1e-15)
    assert (np.abs(act) <= 2.0).all()


def test_a_failed_qp_terminates_the_env():
    ref, s = make(weights=dict(contact_match=0.25), term_weight=-5.0)
    s["reward"][:] = 1.0
    s["status"][:] = (0, 1, 3, 1)
    s["terms"][2, 11], s["done"][2], s["reward"][2] = 1, 1, -4.0       # env 2: the reward stage had terminated it (1 - 5)
    s["timeout"][3], s["done"][3] = 1, 1                               # env 3: timed out in the same step
    keep = {k: np.copy(v) for k, v in s.items()}
    out = ref.teacher(**s)
    assert out["done"].tolist() == [0, 1, 1, 1] and out["timeout"].tolist() == [0, 0, 0, 0] and out["terms"][:, 11].tolist() == [0, 1, 1, 1]
    assert out["reward"].tolist() == [1.5, 1.5 - 5.0, -4.0 + 0.5, 1.5 - 5.0]
    assert all(np.array_equal(s[k], keep[k]) for k in s)               # the inputs are not written


def test_teacher_obs_is_in_the_base_frame_and_blank_for_restarted_envs():
    ref, s = make()
    n = 4
    qpos = np.zeros((n, NQ))
    qpos[:, 3] = 1.0
    c, sn = np.cos(np.pi / 4), np.sin(np.pi / 4)
    qpos[1, 3:7] = qpos[3, 3:7] = (2 * c, 0, 0, 2 * sn)                # yawed by 90 degrees, not normalised
    s["com_ref"][:, 0] += 0.02                                         # the CoM reference 2 cm ahead in world x
    s["com_ref"][:, 3:6] = (0.1, 0.0, -0.05)
    s["foot_ref"][:, 1, 1] -= 0.01
    s["contact_active"][:, 0] = 0
    s["tau"][:] = np.arange(NA)[None, :] + 1.0
    done = np.array([0, 0, 1, 1.0])
    o = ref.teacher_obs(done, s["rows"], qpos, s["tau"], s["com_ref"], s["foot_ref"], s["contact_active"])
    assert o.shape == (n, 14 + NA) and np.array_equal(o[:, 0:2], np.tile([0.0, 1.0], (n, 1)))
    assert np.allclose(o[0, 2:14], [0.02, 0, 0, 0.1, 0, -0.05, 0, 0, 0, 0, -0.01, 0], atol=1e-16)
    # yawed by +90 degrees: world x is the base's -y, world y the base's x
    assert np.allclose(o[1, 2:14], [0, -0.02, 0, 0, -0.1, -0.05, 0, 0, 0, -0.01, 0, 0], atol=1e-16)
    assert np.array_equal(o[0, 14:], (np.arange(NA) + 1.0)[QIDX - 7])
    # restarted: errors and tau exactly 0, contact_active and the CoM velocity reference stay
    for e in (2, 3):
        assert not o[e, 2:5].any() and not o[e, 8:].any() and np.array_equal(o[e, 0:2], [0.0, 1.0])
    assert np.allclose(o[2, 5:8], [0.1, 0, -0.05], atol=1e-16) and np.allclose(o[3, 5:8], [0, -0.1, -0.05], atol=1e-16)


def test_float32_restatement_stays_float32():
    ref, s = make("motor", dtype=np.float32, weights=dict(track_com=1.0))
    s["rows"][:, NQ + NV] += 0.01
    out = ref.teacher(**s)
    assert all(out[k].dtype == np.float32 for k in ("teacher_terms", "teacher_action", "reward", "done", "terms"))
    assert abs(float(out["teacher_terms"][0, 0]) - np.exp(-0.04)) < 1e-6
    qpos = np.zeros((4, NQ))
    qpos[:, 3] = 1
    assert ref.teacher_obs(s["done"], s["rows"], qpos, s["tau"], s["com_ref"], s["foot_ref"], s["contact_active"]).dtype == np.float32


def test_policy_env_knows_the_teacher_terms():
    """what ties this file to the package: the restatement's term order is the binding's"""
    from tsid_control_amd import _lib
    assert _lib.POL_TEACH_TERMS == TEACH_TERMS
