"""The policy actor (tsidb_policy_actor / tsidb_policy_gae, PolicyActor, PolicyEnv.rollout), the parts that need no GPU: the
binding against the header, both libraries' exports, everything the host rejects, and the launches act() and rollout() make."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_testlib import HEADER, assert_prototypes, header_enums  # noqa: E402
from test_policy_host import bare_env  # noqa: E402

NAMES = ("tsidb_policy_actor", "tsidb_policy_gae")


def actor_env(n=3):
    """bare_env with what a PolicyActor reads: the env's seed, a height scan, teacher rows, a command"""
    import numpy as np
    from tsid_control_amd import _lib
    env, calls = bare_env(n=n, decimation=4)
    env.params = np.zeros(_lib.POL_NPARAMS)
    env.params[_lib.POL_P_SEED] = 9
    env.command = torch.zeros(n, 3, dtype=torch.float64)
    env.height_scan = torch.zeros(n, 77, dtype=torch.float64)
    env.teacher_obs = torch.zeros(n, 14 + env.NA, dtype=torch.float64)
    return env, calls


def mlp(*sizes, act=torch.nn.ELU):
    mods = []
    for i in range(len(sizes) - 1):
        mods.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i + 2 < len(sizes):
            mods.append(act())
    return torch.nn.Sequential(*mods)


def test_binding_matches_the_header():
    from tsid_control_amd import _lib
    text, en = HEADER, header_enums("TSIDB_POL_")
    assert (_lib.POL_NET_MAXLAYERS, _lib.POL_NET_MAXBLOCKS, _lib.POL_NET_MAXWIDTH) == \
        (en["TSIDB_POL_NET_MAXLAYERS"], en["TSIDB_POL_NET_MAXBLOCKS"], en["TSIDB_POL_NET_MAXWIDTH"]) == (4, 4, 512)
    assert [en["TSIDB_POL_ACT_" + k.upper()] for k in _lib.POL_ACTIVATIONS] == [0, 1, 2]
    assert _lib.POL_ACTOR_SAMPLE == en["TSIDB_POL_ACTOR_SAMPLE"] == 1
    # the two streams continue the header's table
    for stream in _lib.POL_ACTOR_STREAMS:
        assert re.search(r"^ \*   %d  " % stream, text, re.M), stream
    assert _lib.POL_ACTOR_STREAMS == (21, 22)
    # the structs: the header's fields in order
    for cname, struct in (("tsidb_policy_net", _lib.PolicyNet), ("tsidb_policy_actor_out", _lib.PolicyActorOut)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), text, re.S)
        fields = re.findall(r"\b(\w+)(?:\[4\])?;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
        assert fields == [f[0] for f in struct._fields_], cname
    assert C.sizeof(_lib.PolicyNet) == 4 + 16 + 4 + 32 + 32 + 4 + 4 + 32 + 16 + 16 and C.sizeof(_lib.PolicyActorOut) == 56
    assert_prototypes(NAMES)


def test_policy_actor_is_exported_and_resolves_its_inputs():
    import tsid_control_amd
    from tsid_control_amd.policy_actor import PolicyActor, RolloutStorage, rollout_written
    assert tsid_control_amd.PolicyActor is PolicyActor and tsid_control_amd.RolloutStorage is RolloutStorage
    assert tsid_control_amd.rollout_written is rollout_written
    env, calls = actor_env()
    NA, NOBS = env.NA, env.NOBS
    actor, critic = mlp(NOBS + 77, 32, NA), mlp(NOBS + 4 + 77 + 14 + NA, 16, 1, act=torch.nn.ReLU)
    pa = PolicyActor(env, actor, critic, actor_inputs=("obs", "height_scan"), critic_inputs=("obs", "priv", "height_scan", "teacher_obs"))
    a, c = pa.actor_net.struct, pa.critic_net.struct
    assert (a.n_layers, list(a.width)[:2], a.activation, a.n_blocks) == (2, [32, NA], 0, 2)
    assert (c.n_layers, list(c.width)[:2], c.activation, c.n_blocks) == (2, [16, 1], 2, 4)
    # the parameters in place, nn.Linear's own tensors; obs and priv as strided views of one row
    assert a.weight[0] == actor[0].weight.data_ptr() and a.bias[1] == actor[2].bias.data_ptr()
    assert list(a.block)[:2] == [env.obs.data_ptr(), env.height_scan.data_ptr()] and list(a.block_ld)[:2] == [NOBS + 4, 77]
    assert list(a.block_cols)[:2] == [NOBS, 77]
    assert c.block[1] == env.priv.data_ptr() == env.obs.data_ptr() + 8 * NOBS and c.block_ld[1] == NOBS + 4 and c.block_cols[1] == 4
    assert pa.seed == 9 and pa.env_offset == 0
    assert pa.action.dtype == torch.float64 and pa.action32.dtype == torch.float32 and pa.value.shape == (3,)
    assert pa.actor_input.shape == (3, NOBS + 77) and pa.critic_input.shape == (3, NOBS + 4 + 77 + 14 + NA)
    # act(): one launch
    out = pa.act()
    assert [k[0] for k in calls] == ["tsidb_policy_actor"]
    args = calls[0][1]
    assert len(args) == 9 and args[7] == 1 and args[5].value == 9 and args[6].value == 0 and args[4].value == pa.log_std.data_ptr()
    assert sorted(out) == ["action", "action32", "logp", "mean", "value"] and out["action"] is pa.action
    pa.act(deterministic=True)
    assert calls[1][1][7] == 0
    # lists of (weight, bias) with a named activation; a direct tensor as a block; no critic
    w = [(torch.zeros(8, 5), torch.zeros(8)), (torch.zeros(NA, 8), None)]
    extra = torch.zeros(3, 9, dtype=torch.float64)[:, 2:7]
    pb = PolicyActor(env, w, actor_inputs=(extra,), activation="tanh", seed=4, env_offset=16, log_std=torch.zeros(NA))
    assert pb.actor_net.struct.activation == 1 and pb.actor_net.struct.bias[1] is None and pb.actor_net.struct.block_ld[0] == 9
    assert pb.value is None and pb.act()["value"] is None and (pb.seed, pb.env_offset) == (4, 16)


def test_rejected_networks_and_inputs_raise_with_a_message():
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_actor import PolicyActor
    env, _ = actor_env()
    NA, NOBS = env.NA, env.NOBS
    good = mlp(NOBS, 8, NA)
    z = torch.zeros
    bad = [
        (dict(actor=mlp(NOBS, 8, 8, 8, 8, NA)), "actor: 1 .. 4 layers"),
        (dict(actor=torch.nn.Sequential()), "actor: 1 .. 4 layers"),
        (dict(actor=good, actor_inputs=("obs",) * 5), "actor_inputs: 1 .. 4 blocks"),
        (dict(actor=good, actor_inputs=()), "actor_inputs: 1 .. 4 blocks"),
        (dict(actor=mlp(NOBS, 513, NA)), "actor: layer 0 width 513"),
        (dict(actor=[(z(0, NOBS), None), (z(NA, 0), None)]), "actor: layer 0 width 0"),
        (dict(actor=mlp(600, NA), actor_inputs=(z(3, 600, dtype=torch.float64),)), "actor_inputs: the input row has 600 columns"),
        (dict(actor=mlp(NOBS, 8, NA + 1)), "actor: the last width must be NA"),
        (dict(actor=good, critic=mlp(NOBS, 8, 2)), "critic: the last width must be 1"),
        (dict(actor=[(None, None)]), "actor: layer 0 has no weight"),
        (dict(actor=mlp(NOBS + 1, NA)), r"actor: layer 0 weight must be \[width, %d\]" % NOBS),
        (dict(actor=mlp(NOBS, 8, NA).double()), "actor: layer 0 weight must be a contiguous float32"),
        (dict(actor=[(z(NOBS, NA).t(), None)]), "actor: layer 0 weight must be a contiguous float32"),
        (dict(actor=[(z(NA, NOBS), z(NA + 1))]), "actor: layer 0 bias"),
        (dict(actor=torch.nn.Sequential(torch.nn.Linear(NOBS, 8), torch.nn.Sigmoid(), torch.nn.Linear(8, NA))), "actor: activation Sigmoid"),
        (dict(actor=torch.nn.Sequential(torch.nn.Linear(NOBS, 8), torch.nn.ELU(alpha=0.5), torch.nn.Linear(8, NA))), "actor: ELU alpha"),
        (dict(actor=torch.nn.Sequential(torch.nn.Linear(NOBS, 8), torch.nn.ELU(), torch.nn.Linear(8, 8), torch.nn.Tanh(), torch.nn.Linear(8, NA))),
         "actor: one activation type"),
        (dict(actor=torch.nn.Sequential(torch.nn.Linear(NOBS, NA), torch.nn.Tanh())), "actor: the last layer must be a Linear"),
        (dict(actor=torch.nn.Sequential(torch.nn.Tanh(), torch.nn.Linear(NOBS, NA))), "actor: expected a Linear"),
        (dict(actor=[(z(NA, NOBS), None)], activation="gelu"), "actor: activation must be one of"),
        (dict(actor=torch.nn.Linear(NOBS, NA)), "actor must be a torch.nn.Sequential or a list"),
        (dict(actor=[z(NA, NOBS)]), r"actor: layer 0 must be a \(weight, bias\) pair"),
        (dict(actor=good, actor_inputs=("observation",)), "actor_inputs: unknown input 'observation'"),
        (dict(actor=good, actor_inputs=(z(3, NOBS),)), "actor_inputs: a block must be"),                            # float32 in a float64 env
        (dict(actor=good, actor_inputs=(z(4, NOBS, dtype=torch.float64),)), "actor_inputs: a block must be"),       # rows
        (dict(actor=good, actor_inputs=(z(NOBS, 3, dtype=torch.float64).t(),)), "actor_inputs: a block must be"),   # column stride
        (dict(actor=good, critic=mlp(NOBS, 1), critic_inputs=("priv",)), r"critic: layer 0 weight must be \[width, 4\]"),
        (dict(actor=good, critic_inputs=("obs",)), "critic_inputs without a critic"),
        (dict(actor=good, log_std=z(NA + 1)), "log_std must be"),
        (dict(actor=good, log_std=z(NA, dtype=torch.float64)), "log_std must be"),
        (dict(actor=good, seed=2 ** 32), "seed must be a whole number"),
        (dict(actor=good, seed=-1), "seed must be a whole number"),
        (dict(actor=good, env_offset=2 ** 31), "env_offset must be a whole number"),
        (dict(actor=good, env_offset=0.5), "env_offset must be a whole number"),
    ]
    for kw, msg in bad:
        with pytest.raises(_lib.TsidbError, match="PolicyActor: " + msg):
            PolicyActor(env, **kw)
    # an input the env was built without
    env.height_scan = None
    with pytest.raises(_lib.TsidbError, match="the env has no height_scan"):
        PolicyActor(env, mlp(NOBS + 77, NA), actor_inputs=("obs", "height_scan"))


def test_rollout_is_actor_step_copies_and_a_last_value():
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_actor import PolicyActor, RolloutStorage, rollout_written
    env, calls = actor_env()
    NA, NOBS = env.NA, env.NOBS
    pa = PolicyActor(env, mlp(NOBS, 8, NA), mlp(NOBS + 4, 8, 1), critic_inputs=("obs", "priv"))
    st = env.rollout(pa, 2)
    step = ["tsidb_policy_actor", "tsidb_policy_act", "tsidb_sim_ctrl", "tsidb_policy_reward", "tsidb_reset_done", "tsidb_policy_obs"]
    assert [c[0] for c in calls] == step * 2 + ["tsidb_policy_actor"]
    assert isinstance(st, RolloutStorage) and st.steps == 2
    assert st.actor_input.shape == (2, 3, NOBS) and st.critic_input.shape == (2, 3, NOBS + 4) and st.value.shape == (3, 3)
    assert st.action.shape == st.mean.shape == (2, 3, NA) and st.action.dtype == torch.float32 and st.logp.shape == (2, 3)
    assert st.reward.dtype == st.done.dtype == torch.float64 and st.timeout.dtype == torch.int32 and st.timeout.shape == (2, 3)
    # slot t through the output pointers: the env-dtype action goes to the actor's buffer, which the step reads
    actor_calls = [c[1] for c in calls if c[0] == "tsidb_policy_actor"]
    for t in range(2):
        out = C.cast(actor_calls[t][3], C.POINTER(_lib.PolicyActorOut)).contents
        assert (out.action, out.action32, out.mean, out.logp, out.value, out.actor_input, out.critic_input) == \
            (pa.action.data_ptr(), st.action[t].data_ptr(), st.mean[t].data_ptr(), st.logp[t].data_ptr(), st.value[t].data_ptr(),
             st.actor_input[t].data_ptr(), st.critic_input[t].data_ptr())
        assert actor_calls[t][7] == 1 and actor_calls[t][1] is not None and actor_calls[t][2] is not None
    last = actor_calls[2]
    out = C.cast(last[3], C.POINTER(_lib.PolicyActorOut)).contents
    assert last[1] is None and last[2] is not None and last[7] == 0             # the critic alone, no draw
    assert out.value == st.value[2].data_ptr() and out.action is None and out.mean is None and out.critic_input is None
    acts = [c[1] for c in calls if c[0] == "tsidb_policy_act"]
    assert all(a[1].value == pa.action.data_ptr() for a in acts)
    # reuse; the advantages are one launch
    del calls[:]
    assert env.rollout(pa, 2, st) is st
    adv, ret = st.gae(0.99, 0.95)
    assert calls[-1][0] == "tsidb_policy_gae" and adv.shape == ret.shape == (2, 3) and adv.dtype == torch.float32
    g = calls[-1][1]
    assert g[0] == 2 and [a.value for a in g[1:5]] == [t.data_ptr() for t in (st.reward, st.done, st.timeout, st.value)]
    assert abs(g[5].value - 0.99) < 1e-7 and abs(g[6].value - 0.95) < 1e-7 and [a.value for a in g[7:9]] == [adv.data_ptr(), ret.data_ptr()]
    ids = {id(t) for t in rollout_written(st)}
    assert {id(t) for t in (st.actor_input, st.critic_input, st.action, st.mean, st.logp, st.value, st.reward, st.done, st.timeout, adv, ret,
                            pa.action)} == ids
    # what rollout() rejects
    for args, msg in (((pa, 0), "steps"), ((pa, 2.0), "steps"), ((pa, 3, st), "storage"), ((object(), 2), "actor must be a PolicyActor")):
        with pytest.raises(_lib.TsidbError, match="PolicyEnv.rollout: .*" + msg):
            env.rollout(*args)
    other, _ = actor_env()
    with pytest.raises(_lib.TsidbError, match="built on this env"):
        other.rollout(pa, 2)
