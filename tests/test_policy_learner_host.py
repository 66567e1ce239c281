"""The policy learner (tsidb_policy_learn, PolicyLearner), the parts that need no GPU: the binding against the header, both
libraries' exports, the launches backward() and update() make with their arguments, the .grad tensors, and what the host rejects."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_testlib import HEADER, assert_prototypes, header_enums  # noqa: E402
from test_policy_actor_host import actor_env, mlp  # noqa: E402

NAMES = ("tsidb_policy_learn_workspace", "tsidb_policy_learn")
ROOT_CSRC = Path(__file__).resolve().parent.parent / "tsid_control_amd" / "csrc"


def learner_setup(critic=True, T=2, gae=True, **kw):
    """(env, calls, PolicyActor, RolloutStorage, PolicyLearner) on the recording env"""
    from tsid_control_amd import PolicyActor, PolicyLearner, RolloutStorage
    env, calls = actor_env()
    pa = PolicyActor(env, mlp(env.NOBS, 8, env.NA), mlp(env.NOBS + 4, 8, 1) if critic else None, critic_inputs=("obs", "priv") if critic else None)
    st = RolloutStorage(env, pa, T)
    if gae:
        st.gae()
    del calls[:]
    return env, calls, pa, st, PolicyLearner(pa, **kw)


def test_binding_matches_the_header():
    from tsid_control_amd import _lib
    import policy_learner_reference as R
    en = header_enums("TSIDB_POL_LEARN_")
    assert _lib.POL_LEARN_SEG_ROWS == en["TSIDB_POL_LEARN_SEG_ROWS"] == R.SEG_ROWS and _lib.POL_LEARN_SEG_ROWS % 16 == 0
    assert len(_lib.POL_LEARN_STATS) == en["TSIDB_POL_LEARN_NSTATS"] == 8 and _lib.POL_LEARN_STATS == R.STATS
    for cname, struct in (("tsidb_policy_learn_batch", _lib.PolicyLearnBatch), ("tsidb_policy_grads", _lib.PolicyGrads),
                          ("tsidb_policy_learn_cfg", _lib.PolicyLearnCfg)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), HEADER, re.S)
        fields = re.findall(r"\b(\w+)(?:\[4\])?;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
        assert fields == [f[0] for f in struct._fields_], cname
    assert C.sizeof(_lib.PolicyLearnBatch) == 8 * 8 + 4 + 4 + 8 and C.sizeof(_lib.PolicyGrads) == 64 and C.sizeof(_lib.PolicyLearnCfg) == 16
    assert C.sizeof(_lib.PolicyNet) == 4 + 16 + 4 + 32 + 32 + 4 + 4 + 32 + 16 + 16          # (tsidb_policy_net did not grow)
    assert_prototypes(NAMES)
    assert (ROOT_CSRC / "tsidb_learner.hpp").exists()


def test_backward_is_a_workspace_query_and_one_call_with_the_storage_behind_it():
    import tsid_control_amd
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_learner import PolicyLearner
    assert tsid_control_amd.PolicyLearner is PolicyLearner
    env, calls, pa, st, pl = learner_setup(clip=0.1, value_coef=0.5, entropy_coef=0.01)
    assert len(pl.parameters()) == 2 * 2 + 2 * 2 + 1 and pl.parameters()[-1] is pa.log_std
    assert all(p.grad is None for p in pl.parameters())
    index = torch.tensor([4, 0, 5, 5], dtype=torch.int32)
    stats = pl.backward(st, index)
    assert stats is pl.stats and stats.shape == (8,) and stats.dtype == torch.float32
    assert [c[0] for c in calls] == ["tsidb_policy_learn_workspace", "tsidb_policy_learn"]
    q = calls[0][1]
    assert len(q) == 4 and q[2] == 4                               # (+ the handle: the header's 5)
    a = calls[1][1]
    assert len(a) == 12
    batch = C.cast(a[2], C.POINTER(_lib.PolicyLearnBatch)).contents
    assert (batch.actor_input, batch.critic_input, batch.action, batch.logp, batch.value, batch.advantage, batch.returns, batch.index) == \
        tuple(t.data_ptr() for t in (st.actor_input, st.critic_input, st.action, st.logp, st.value, st.advantage, st.returns, index))
    assert (batch.rows, batch.M, batch.adv_stats) == (2 * 3, 4, pl.adv_stats.data_ptr())
    for arg, net in ((a[3], pa.actor_net), (a[4], pa.critic_net)):
        g = C.cast(arg, C.POINTER(_lib.PolicyGrads)).contents
        for l, (w, b) in enumerate(net.layers):
            assert w.grad.dtype == torch.float32 and w.grad.shape == w.shape and float(w.grad.abs().max()) == 0
            assert (g.weight[l], g.bias[l]) == (w.grad.data_ptr(), b.grad.data_ptr())
        assert g.weight[2] is None and g.bias[2] is None
    assert a[0]._obj is pa.actor_net.struct and a[1]._obj is pa.critic_net.struct
    assert (a[5].value, a[6].value) == (pa.log_std.data_ptr(), pa.log_std.grad.data_ptr()) and not pa.log_std.requires_grad
    cfg = C.cast(a[7], C.POINTER(_lib.PolicyLearnCfg)).contents
    assert (round(cfg.clip, 6), round(cfg.value_coef, 6), round(cfg.entropy_coef, 6), cfg.value_clip) == (0.1, 0.5, 0.01, 1)
    assert a[8].value == pl.workspace.data_ptr() and a[9].value == pl.workspace.numel() * 4 and a[10].value == stats.data_ptr()
    # a smaller minibatch reuses the workspace, a larger one asks again; zero_grad(set_to_none=True) is harmless: new tensors, new pointers
    del calls[:]
    old = pa.actor_net.layers[0][0].grad
    for p in pl.parameters():
        p.grad = None
    pl.backward(st, index[:2])
    pl.backward(st, torch.zeros(5, dtype=torch.int32))
    assert [c[0] for c in calls] == ["tsidb_policy_learn", "tsidb_policy_learn_workspace", "tsidb_policy_learn"]
    g = C.cast(calls[0][1][3], C.POINTER(_lib.PolicyGrads)).contents
    new = pa.actor_net.layers[0][0].grad
    assert new is not None and new is not old and g.weight[0] == new.data_ptr() and calls[0][1][2] is not None
    assert C.cast(calls[0][1][2], C.POINTER(_lib.PolicyLearnBatch)).contents.M == 2
    # a .grad the caller gave is used as it is
    mine = torch.zeros_like(pa.log_std)
    pa.log_std.grad = mine
    pl.backward(st, index)
    assert calls[-1][1][6].value == mine.data_ptr()
    ids = {id(t) for t in pl.written()}
    assert {id(p.grad) for p in pl.parameters()} | {id(pl.stats), id(pl.adv_stats), id(pl.workspace)} == ids
    # no critic, no normalisation: NULLs
    env, calls, pa, st, pl = learner_setup(critic=False, normalize_advantage=False, value_clip=False)
    pl.backward(st, index)
    a = calls[-1][1]
    assert a[1] is None and a[4] is None and C.cast(a[2], C.POINTER(_lib.PolicyLearnBatch)).contents.adv_stats is None
    assert C.cast(a[7], C.POINTER(_lib.PolicyLearnCfg)).contents.value_clip == 0
    assert C.cast(a[2], C.POINTER(_lib.PolicyLearnBatch)).contents.critic_input is None


def test_update_is_a_backward_and_a_step_per_slice():
    from tsid_control_amd import _lib
    env, calls, pa, st, pl = learner_setup(T=3)

    class Steps:
        n = 0

        def step(self):
            assert calls[-1][0] == "tsidb_policy_learn"
            self.n += 1
    opt = Steps()
    gen = torch.Generator().manual_seed(3)
    out = pl.update(st, opt, epochs=2, minibatches=4, generator=gen)
    learn = [c[1] for c in calls if c[0] == "tsidb_policy_learn"]
    assert len(learn) == opt.n == 8 and out.shape == (8, 8) and out.dtype == torch.float32
    Ms = [C.cast(a[2], C.POINTER(_lib.PolicyLearnBatch)).contents.M for a in learn]
    assert Ms == [2, 2, 2, 3] * 2 and sum(Ms[:4]) == 9
    assert [a[10].value for a in learn] == [out[k].data_ptr() for k in range(8)]
    assert len({a[2] is not None and C.cast(a[2], C.POINTER(_lib.PolicyLearnBatch)).contents.adv_stats for a in learn}) == 1
    for kw, msg in ((dict(epochs=0), "epochs"), (dict(minibatches=2.0), "minibatches"), (dict(minibatches=10), "10 minibatches of 9")):
        with pytest.raises(_lib.TsidbError, match="PolicyLearner: .*" + msg):
            pl.update(st, opt, **kw)


def test_rejected_arguments_raise_with_a_message():
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_learner import PolicyLearner
    env, calls, pa, st, pl = learner_setup()
    for kw, msg in ((dict(clip=0), "clip must be > 0"), (dict(clip=-0.1), "clip must be > 0"), (dict(clip="a"), "clip must be a finite number"),
                    (dict(clip=float("nan")), "clip must be a finite number"), (dict(value_coef=-1), "value_coef must be >= 0"),
                    (dict(entropy_coef=float("inf")), "entropy_coef must be a finite number"), (dict(value_clip=1), "value_clip must be a bool"),
                    (dict(normalize_advantage=None), "normalize_advantage must be a bool")):
        with pytest.raises(_lib.TsidbError, match="PolicyLearner: " + msg):
            PolicyLearner(pa, **kw)
    with pytest.raises(_lib.TsidbError, match="PolicyLearner: actor must be a PolicyActor"):
        PolicyLearner(object())
    good = torch.zeros(4, dtype=torch.int32)
    for index, msg in ((torch.zeros(4, dtype=torch.int64), "index must be"), (torch.zeros(0, dtype=torch.int32), "index must be"),
                       (torch.zeros(2, 2, dtype=torch.int32), "index must be"), (torch.zeros(8, dtype=torch.int32)[::2], "index must be"),
                       ([0, 1], "index must be")):
        with pytest.raises(_lib.TsidbError, match="PolicyLearner: " + msg):
            pl.backward(st, index)
    with pytest.raises(_lib.TsidbError, match="PolicyLearner: stats must be"):
        pl.backward(st, good, stats=torch.zeros(7))
    with pytest.raises(_lib.TsidbError, match="PolicyLearner: storage must be a RolloutStorage of this learner's actor"):
        pl.backward(object(), good)
    other = learner_setup()[3]
    with pytest.raises(_lib.TsidbError, match="PolicyLearner: storage must be a RolloutStorage of this learner's actor"):
        pl.backward(other, good)
    fresh = learner_setup(gae=False)
    with pytest.raises(_lib.TsidbError, match="PolicyLearner: storage.gae\\(\\) has not run"):
        fresh[4].backward(fresh[3], good)
    with pytest.raises(_lib.TsidbError, match="PolicyLearner: update needs a RolloutStorage whose gae"):
        fresh[4].update(fresh[3], None)
    pa.actor_net.layers[0][0].grad = torch.zeros(env.NOBS, 8).t()
    with pytest.raises(_lib.TsidbError, match="PolicyLearner: a .grad must be a contiguous float32"):
        pl.backward(st, good)
    assert not [c for c in calls if c[0] == "tsidb_policy_learn"]
