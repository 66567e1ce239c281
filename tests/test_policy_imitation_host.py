"""Imitation of the TSID teacher (tsidb_policy_teacher_mix, tsidb_policy_learn_imit; RolloutStorage(teacher=True),
PolicyEnv.rollout(teacher_beta=...), PolicyLearner(imitation_coef=...)), the parts that need no GPU: the binding against the
header, both libraries' exports, the launches a teacher rollout and an imitation backward() make with their arguments, the
unchanged launches of the plain ones, and what the host rejects.  (What the library itself rejects needs a handle:
tests/test_gpu_policy_imitation.py.)"""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_testlib import HEADER, assert_prototypes, header_enums  # noqa: E402
from test_policy_actor_host import mlp  # noqa: E402
from test_policy_tsid_host import tsid_env  # noqa: E402

NAMES = ("tsidb_policy_teacher_mix", "tsidb_policy_learn_imit_workspace", "tsidb_policy_learn_imit")


def teacher_env(mode="motor", tsid="stand"):
    """the recording env with TSID in the loop and what a PolicyActor reads"""
    from tsid_control_amd import _lib
    env, calls = tsid_env(tsid, 4)
    env.mode = mode
    env.params = np.zeros(_lib.POL_NPARAMS)
    env.params[_lib.POL_P_SEED] = 9
    return env, calls


def setup(teacher=True, T=2, critic=True, **kw):
    """(env, calls, PolicyActor, RolloutStorage with gae() run, PolicyLearner)"""
    from tsid_control_amd import PolicyActor, PolicyLearner, RolloutStorage
    env, calls = teacher_env()
    pa = PolicyActor(env, mlp(env.NOBS, 8, env.NA), mlp(env.NOBS + 4, 8, 1) if critic else None, critic_inputs=("obs", "priv") if critic else None,
                     seed=5, env_offset=16)
    st = RolloutStorage(env, pa, T, teacher=teacher)
    st.gae()
    del calls[:]
    return env, calls, pa, st, PolicyLearner(pa, **kw)


def test_binding_matches_the_header():
    from tsid_control_amd import _lib
    import policy_imitation_reference as RI
    en = header_enums("TSIDB_POL_IMIT_")
    assert [en["TSIDB_POL_IMIT_" + k.upper()] for k in _lib.POL_IMIT_LOSSES] == [0, 1] and _lib.POL_IMIT_LOSSES == RI.LOSSES
    assert len(_lib.POL_IMIT_STATS) == en["TSIDB_POL_IMIT_NSTATS"] == 4 and _lib.POL_IMIT_STATS == RI.IMIT_STATS
    assert header_enums("TSIDB_POL_LEARN_")["TSIDB_POL_LEARN_NSTATS"] == 8            # (the learner's stats did not grow)
    m = re.search(r"typedef struct tsidb_policy_imit \{(.*?)\} tsidb_policy_imit;", HEADER, re.S)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f[0] for f in _lib.PolicyImit._fields_] == ["target", "weight", "skip_surrogate", "imitation_coef", "surrogate_coef",
                                                                   "loss", "stats"]
    assert C.sizeof(_lib.PolicyImit) == 3 * 8 + 3 * 4 + 4 + 8               # (three floats / ints, padding, the pointer)
    assert C.sizeof(_lib.PolicyLearnBatch) == 8 * 8 + 4 + 4 + 8 and C.sizeof(_lib.PolicyLearnCfg) == 16      # (neither grew)
    # the stream continues the header's table, behind the action noise
    assert _lib.POL_TEACHER_MIX_STREAM == RI.STREAM == 23 == max(_lib.POL_ACTOR_STREAMS) + 1
    assert re.search(r"^ \*   23  ", HEADER, re.M)
    assert_prototypes(NAMES)
    # the new entry is the old one's twelve arguments and the struct
    old = re.search(r"\bint tsidb_policy_learn\(([^;]*)\);", HEADER).group(1).split(",")
    new = re.search(r"\bint tsidb_policy_learn_imit\(([^;]*)\);", HEADER).group(1).split(",")
    assert len(old) == 13 and len(new) == 14 and "tsidb_policy_imit *imit" in new[9]
    # without a handle nothing is looked at
    for lib in sorted((Path(_lib.__file__).parent).glob("libtsidb*.so")):
        L = _lib.load(lib)
        assert L.tsidb_policy_teacher_mix(*([None] * 8), 0, 0, None) == -1
        assert L.tsidb_policy_learn_imit(*([None] * 11), 0, None, None) == -1


def test_teacher_storage_holds_three_more_tensors():
    from tsid_control_amd import PolicyActor, RolloutStorage, _lib
    from tsid_control_amd.policy_actor import rollout_written
    env, calls = teacher_env()
    pa = PolicyActor(env, mlp(env.NOBS, 8, env.NA))
    plain, st = RolloutStorage(env, pa, 2), RolloutStorage(env, pa, 2, teacher=True)
    assert plain.teacher_action is None and plain.teacher_weight is None and plain.teacher_executed is None
    assert len(st.tensors()) == len(plain.tensors()) + 3
    assert st.teacher_action.shape == (2, 3, env.NA) and st.teacher_action.dtype == torch.float32
    assert st.teacher_weight.shape == (2, 3) and st.teacher_weight.dtype == torch.float32
    assert st.teacher_executed.shape == (2, 3) and st.teacher_executed.dtype == torch.int32
    ids = {id(t) for t in rollout_written(st)}
    assert {id(st.teacher_action), id(st.teacher_weight), id(st.teacher_executed)} <= ids
    assert not {id(t) for t in rollout_written(plain)} & {id(st.teacher_action), id(st.teacher_weight), id(st.teacher_executed)}
    for mode, tsid, msg in (("residual", "stand", "needs mode 'position' or 'motor', got 'residual'"), ("motor", None, "needs an env with tsid")):
        env.mode, env.tsid = mode, tsid
        with pytest.raises(_lib.TsidbError, match="RolloutStorage: teacher = True " + msg):
            RolloutStorage(env, pa, 2, teacher=True)
    env.mode, env.tsid = "position", "stand"
    assert RolloutStorage(env, pa, 2, teacher=True).teacher_action is not None
    with pytest.raises(_lib.TsidbError, match="RolloutStorage: teacher must be a bool"):
        RolloutStorage(env, pa, 2, teacher=1)
    assert not calls


def test_teacher_rollout_launches_the_mix_between_the_actor_and_the_act():
    from tsid_control_amd import PolicyActor, RolloutStorage, _lib
    env, calls = teacher_env()
    pa = PolicyActor(env, mlp(env.NOBS, 8, env.NA), mlp(env.NOBS + 4, 8, 1), critic_inputs=("obs", "priv"), seed=5, env_offset=16)
    env.rollout(pa, 2)
    plain = [c[0] for c in calls]
    assert plain.count("tsidb_policy_actor") == 3 and "tsidb_policy_teacher_mix" not in plain and env._teacher_beta is None
    # a teacher storage: the same list with the mix behind each sampling actor launch
    del calls[:]
    st = RolloutStorage(env, pa, 2, teacher=True)
    assert env.rollout(pa, 2, st, teacher_beta=0.25) is st
    names = [c[0] for c in calls]
    want, k = [], 0
    for name in plain:
        want.append(name)
        if name == "tsidb_policy_actor" and k < 2:
            want.append("tsidb_policy_teacher_mix")
            k += 1
    assert names == want
    for i, name in enumerate(names):
        if name == "tsidb_policy_teacher_mix":
            assert names[i - 1] == "tsidb_policy_actor" and names[i + 1] == "tsidb_policy_act"
    mixes = [c[1] for c in calls if c[0] == "tsidb_policy_teacher_mix"]
    beta = env._teacher_beta
    assert beta.shape == (1,) and beta.dtype == torch.float32 and float(beta) == 0.25
    for t, a in enumerate(mixes):
        assert len(a) == 10                                             # (+ the handle: the header's 11)
        assert a[0]._obj is env._bufs
        assert [x.value for x in a[1:7]] == [x.data_ptr() for x in (env.teacher_action, pa.action, st.teacher_action[t], st.teacher_weight[t],
                                                                     st.teacher_executed[t], beta)]
        assert (a[7].value, a[8].value) == (5, 16)
    # the env's tensor is reused and refilled; a tensor of the caller's is passed as it is; None = no beta
    env.rollout(pa, 2, st, teacher_beta=1)
    assert env._teacher_beta is beta and float(beta) == 1.0
    mine = torch.tensor([0.5])
    del calls[:]
    env.rollout(pa, 2, st, teacher_beta=mine)
    assert [c[1][6].value for c in calls if c[0] == "tsidb_policy_teacher_mix"] == [mine.data_ptr()] * 2 and float(beta) == 1.0
    del calls[:]
    env.rollout(pa, 2, st)
    assert [c[1][6] for c in calls if c[0] == "tsidb_policy_teacher_mix"] == [None, None]
    # rejected: a beta without a teacher storage, and what is no beta
    del calls[:]
    for args, kw, msg in (((pa, 2), dict(teacher_beta=0.5), "teacher_beta needs a storage built with teacher = True"),
                          ((pa, 2, RolloutStorage(env, pa, 2)), dict(teacher_beta=0.5), "teacher_beta needs a storage built with teacher = True"),
                          ((pa, 2, st), dict(teacher_beta=1.5), "teacher_beta must be None, a number in"),
                          ((pa, 2, st), dict(teacher_beta=-0.1), "teacher_beta must be None, a number in"),
                          ((pa, 2, st), dict(teacher_beta=True), "teacher_beta must be None, a number in"),
                          ((pa, 2, st), dict(teacher_beta="all"), "teacher_beta must be None, a number in"),
                          ((pa, 2, st), dict(teacher_beta=torch.zeros(2)), "a teacher_beta tensor must be"),
                          ((pa, 2, st), dict(teacher_beta=torch.zeros(1, dtype=torch.float64)), "a teacher_beta tensor must be")):
        with pytest.raises(_lib.TsidbError, match="PolicyEnv.rollout: " + msg):
            env.rollout(*args, **kw)
    assert not calls


def test_backward_with_the_term_off_makes_the_old_two_calls():
    for kw in ({}, dict(imitation_coef=0.0, surrogate_coef=1.0, imitation_loss="huber")):
        env, calls, pa, st, pl = setup(**kw)
        pl.backward(st, torch.tensor([4, 0, 5, 5], dtype=torch.int32))
        assert [c[0] for c in calls] == ["tsidb_policy_learn_workspace", "tsidb_policy_learn"] and len(calls[1][1]) == 12
        assert id(pl.imit_stats) not in {id(t) for t in pl.written()}
    # and on a plain storage
    env, calls, pa, st, pl = setup(teacher=False)
    pl.backward(st, torch.tensor([1, 2], dtype=torch.int32))
    assert [c[0] for c in calls] == ["tsidb_policy_learn_workspace", "tsidb_policy_learn"]


def test_backward_with_the_term_on_makes_the_new_entry_with_the_storage_behind_the_struct():
    from tsid_control_amd import _lib
    env, calls, pa, st, pl = setup(imitation_coef=0.5, imitation_loss="huber", surrogate_coef=0.25, clip=0.1, value_coef=0.5)
    assert pl.imit_stats.shape == (4,) and pl.imit_stats.dtype == torch.float32
    index = torch.tensor([4, 0, 5, 5], dtype=torch.int32)
    stats = pl.backward(st, index)
    assert stats is pl.stats and stats.shape == (8,)
    assert [c[0] for c in calls] == ["tsidb_policy_learn_imit_workspace", "tsidb_policy_learn_imit"]
    q, a = calls[0][1], calls[1][1]
    assert len(q) == 4 and q[2] == 4 and len(a) == 13                      # (+ the handle: the header's 5 and 14)
    batch = C.cast(a[2], C.POINTER(_lib.PolicyLearnBatch)).contents
    assert (batch.action, batch.logp, batch.index, batch.rows, batch.M) == (st.action.data_ptr(), st.logp.data_ptr(), index.data_ptr(), 6, 4)
    cfg = C.cast(a[7], C.POINTER(_lib.PolicyLearnCfg)).contents
    assert (round(cfg.clip, 6), round(cfg.value_coef, 6)) == (0.1, 0.5)
    im = C.cast(a[8], C.POINTER(_lib.PolicyImit)).contents
    assert (im.target, im.weight, im.skip_surrogate, im.stats) == (st.teacher_action.data_ptr(), st.teacher_weight.data_ptr(),
                                                                   st.teacher_executed.data_ptr(), pl.imit_stats.data_ptr())
    assert (im.imitation_coef, im.surrogate_coef, im.loss) == (0.5, 0.25, 1)
    assert a[9].value == pl.workspace.data_ptr() and a[10].value == pl.workspace.numel() * 4 and a[11].value == stats.data_ptr()
    assert id(pl.imit_stats) in {id(t) for t in pl.written()}
    # a surrogate weight alone needs no labels: the new entry with NULLs behind the struct
    env, calls, pa, st, pl = setup(teacher=False, surrogate_coef=0.0, critic=False)
    pl.backward(st, index)
    assert [c[0] for c in calls] == ["tsidb_policy_learn_imit_workspace", "tsidb_policy_learn_imit"]
    im = C.cast(calls[1][1][8], C.POINTER(_lib.PolicyImit)).contents
    assert (im.target, im.weight, im.skip_surrogate, im.imitation_coef, im.surrogate_coef, im.loss) == (None, None, None, 0.0, 0.0, 0)
    # update(): a backward and a step per slice, as ever
    env, calls, pa, st, pl = setup(T=3, imitation_coef=1.0, surrogate_coef=0.0, value_coef=0.0)

    class Steps:
        n = 0

        def step(self):
            assert calls[-1][0] == "tsidb_policy_learn_imit"
            self.n += 1
    opt = Steps()
    out = pl.update(st, opt, epochs=2, minibatches=2, generator=torch.Generator().manual_seed(3))
    assert opt.n == 4 and out.shape == (4, 8) and not [c for c in calls if c[0] == "tsidb_policy_learn"]


def test_rejected_arguments_raise_with_a_message():
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_learner import PolicyLearner
    env, calls, pa, st, pl = setup()
    for kw, msg in ((dict(imitation_coef=-1), "imitation_coef must be >= 0"), (dict(imitation_coef=float("nan")), "imitation_coef must be a finite number"),
                    (dict(imitation_coef="a"), "imitation_coef must be a finite number"), (dict(surrogate_coef=-0.5), "surrogate_coef must be >= 0"),
                    (dict(surrogate_coef=float("inf")), "surrogate_coef must be a finite number"), (dict(imitation_loss="l1"), "imitation_loss must be one of"),
                    (dict(imitation_loss=1), "imitation_loss must be one of")):
        with pytest.raises(_lib.TsidbError, match="PolicyLearner: " + msg):
            PolicyLearner(pa, **kw)
    env, calls, pa, st, pl = setup(teacher=False, imitation_coef=0.5)
    with pytest.raises(_lib.TsidbError, match="PolicyLearner: imitation_coef > 0 needs a storage with the teacher's labels"):
        pl.backward(st, torch.zeros(4, dtype=torch.int32))
    assert not calls
