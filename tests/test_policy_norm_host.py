"""The policy normaliser (tsidb_policy_norm_update / tsidb_policy_actor_norm, PolicyNormalizer), the parts that need no GPU: the
binding against the header, both libraries' exports, everything the host rejects, the launches act() and rollout() make with
and without a normaliser, and the state dict."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_norm_reference as R  # noqa: E402
from policy_testlib import HEADER, assert_prototypes, header_enums  # noqa: E402
from test_policy_actor_host import actor_env, mlp  # noqa: E402

NAMES = ("tsidb_policy_norm_workspace", "tsidb_policy_norm_update", "tsidb_policy_actor_norm")


def test_binding_matches_the_header():
    from tsid_control_amd import _lib
    assert _lib.POL_NORM_SEG_ROWS == header_enums("TSIDB_POL_NORM_")["TSIDB_POL_NORM_SEG_ROWS"] == R.SEG_ROWS
    assert _lib.POL_NORM_SEG_ROWS % 16 == 0
    m = re.search(r"typedef struct tsidb_policy_norm \{(.*?)\} tsidb_policy_norm;", HEADER, re.S)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f[0] for f in _lib.PolicyNorm._fields_]
    assert C.sizeof(_lib.PolicyNorm) == 8 + 8 + 8 + 8 + 8 + 8
    assert (_lib.PolicyNorm.clip.offset, _lib.PolicyNorm.stats.offset, _lib.PolicyNorm.until.offset) == (8, 16, 40)
    # the network struct is the one from before the normaliser: nothing was appended, the learner cannot see one
    assert C.sizeof(_lib.PolicyNet) == 160
    assert_prototypes(NAMES)


def build(n=3, has_critic=True, **kw):
    from tsid_control_amd import PolicyActor, PolicyNormalizer
    env, calls = actor_env(n)
    NA, NOBS = env.NA, env.NOBS
    nz = PolicyNormalizer(**kw)
    pa = PolicyActor(env, mlp(NOBS, 8, NA), mlp(NOBS + 4, 8, 1) if has_critic else None, critic_inputs=("obs", "priv") if has_critic else None,
                     normalizer=nz)
    return env, calls, pa, nz


def test_without_a_normaliser_nothing_changes():
    from tsid_control_amd import PolicyActor, _lib
    env, calls = actor_env()
    NA, NOBS = env.NA, env.NOBS
    actor, critic = mlp(NOBS, 8, NA), mlp(NOBS, 8, 1)
    pa, pb = PolicyActor(env, actor, critic), PolicyActor(env, actor, critic, normalizer=None)
    assert pa.normalizer is None and pb.normalizer is None
    assert bytes(pa.actor_net.struct) == bytes(pb.actor_net.struct) and bytes(pa.critic_net.struct) == bytes(pb.critic_net.struct)
    pb.act()
    env.rollout(pb, 1)
    names = [c[0] for c in calls]
    assert "tsidb_policy_actor_norm" not in names and "tsidb_policy_norm_update" not in names
    assert names[0] == "tsidb_policy_actor" and len(calls[0][1]) == 9
    assert len(pb.written()) == 7
    with pytest.raises(_lib.TsidbError, match="PolicyActor: normalizer must be a PolicyNormalizer"):
        PolicyActor(env, actor, critic, normalizer=dict(eps=1e-2))


def test_state_structs_and_launch_order():
    import tsid_control_amd
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_normalizer import PolicyNormalizer
    assert tsid_control_amd.PolicyNormalizer is PolicyNormalizer
    env, calls, pa, nz = build(eps=0.05, clip=4.0, until=1000)
    NA, NOBS = env.NA, env.NOBS
    assert pa.normalizer is nz and nz.training
    for st, K in ((nz.actor, NOBS), (nz.critic, NOBS + 4)):
        assert st.stats.shape == (2, K) and st.stats.dtype == torch.float64 and st.count.shape == (1,) and st.count.dtype == torch.int64
        assert st.affine.shape == (2, K) and st.affine.dtype == torch.float32
        assert (st.stats[0] == 0).all() and (st.stats[1] == 1).all() and st.count.item() == 0
        assert (st.affine[0] == 0).all() and (st.affine[1] == torch.tensor(1.0 / 1.05, dtype=torch.float64).float()).all()
        s = st.struct
        assert (s.affine, s.stats, s.count) == (st.affine.data_ptr(), st.stats.data_ptr(), st.count.data_ptr())
        assert (s.clip, s.eps, s.until) == (4.0, 0.05, 1000)
    assert nz.workspace.dtype == torch.float64 and nz.workspace.numel() == 2 * (NOBS + NOBS + 4)
    ids = [id(t) for t in nz.written()]
    assert ids == [id(t) for t in (nz.actor.stats, nz.actor.count, nz.actor.affine, nz.critic.stats, nz.critic.count, nz.critic.affine, nz.workspace)]
    assert [id(t) for t in pa.written()][7:] == ids
    # act() in training mode: the update, then the launch that normalises; in eval mode the launch alone
    pa.act()
    assert [c[0] for c in calls] == ["tsidb_policy_norm_update", "tsidb_policy_actor_norm"]
    up, act = calls[0][1], calls[1][1]
    assert len(up) == 7 and len(act) == 11          # (one more in the library: the handle)
    norm = lambda ref: C.cast(ref, C.POINTER(_lib.PolicyNorm)).contents
    assert norm(up[2]).stats == nz.actor.stats.data_ptr() and norm(up[3]).stats == nz.critic.stats.data_ptr()
    assert up[4].value == nz.workspace.data_ptr() and up[5].value == nz.workspace.numel() * 8
    assert norm(act[3]).affine == nz.actor.affine.data_ptr() and norm(act[4]).affine == nz.critic.affine.data_ptr() and act[9] == 1
    del calls[:]
    assert nz.eval() is nz and not nz.training
    pa.act(deterministic=True)
    assert [c[0] for c in calls] == ["tsidb_policy_actor_norm"] and calls[0][1][9] == 0
    assert nz.train() is nz and nz.training
    # rollout: per step update, launch, step; the closing value launch without an update and without the actor's norm
    del calls[:]
    st = env.rollout(pa, 2)
    step = ["tsidb_policy_norm_update", "tsidb_policy_actor_norm", "tsidb_policy_act", "tsidb_sim_ctrl", "tsidb_policy_reward", "tsidb_reset_done",
            "tsidb_policy_obs"]
    assert [c[0] for c in calls] == step * 2 + ["tsidb_policy_actor_norm"]
    last = calls[-1][1]
    assert last[1] is None and last[3] is None and norm(last[4]).affine == nz.critic.affine.data_ptr() and last[9] == 0
    from tsid_control_amd import rollout_written
    assert [id(t) for t in rollout_written(st)][-7:] == ids
    nz.eval()
    del calls[:]
    env.rollout(pa, 1, env.rollout(pa, 1))
    assert "tsidb_policy_norm_update" not in [c[0] for c in calls]
    # critic = False: the critic's rows stay raw, no state for it; no critic at all likewise
    for has_critic, kw in ((True, dict(critic=False)), (False, dict())):
        env, calls, pa, nz = build(has_critic=has_critic, **kw)
        assert nz.critic is None and len(nz.written()) == 4 and nz.workspace.numel() == 2 * NOBS
        pa.act()
        assert calls[0][1][1] is None and calls[0][1][3] is None and calls[1][1][4] is None


def test_rejected_settings_raise_with_a_message():
    from tsid_control_amd import PolicyActor, PolicyNormalizer, _lib
    bad = [(dict(eps=0), "eps must be > 0"), (dict(eps=-1e-2), "eps must be > 0"), (dict(eps="1e-2"), "eps must be a finite number"),
           (dict(eps=float("nan")), "eps must be a finite number"), (dict(eps=True), "eps must be a finite number"),
           (dict(clip=0), "clip must be > 0"), (dict(clip=-5.0), "clip must be > 0"), (dict(clip="5"), "clip must be a finite number"),
           (dict(clip=float("inf")), "clip must be a finite number"),
           (dict(until=0), "until must be a whole number >= 1"), (dict(until=-3), "until must be a whole number >= 1"),
           (dict(until=2.0), "until must be a whole number >= 1"), (dict(until=True), "until must be a whole number >= 1"),
           (dict(critic=1), "critic must be a bool")]
    for kw, msg in bad:
        with pytest.raises(_lib.TsidbError, match="PolicyNormalizer: " + msg):
            PolicyNormalizer(**kw)
    nz = PolicyNormalizer()
    assert (nz.eps, nz.clip, nz.until, nz.with_critic) == (1e-2, None, None, True)
    for call in (nz.update, nz.written, nz.state_dict, lambda: nz.load_state_dict({})):
        with pytest.raises(_lib.TsidbError, match="PolicyNormalizer: not attached"):
            call()
    with pytest.raises(_lib.TsidbError, match="PolicyNormalizer: mode must be a bool"):
        nz.train(1)
    env, calls = actor_env()
    PolicyActor(env, mlp(env.NOBS, 8, env.NA), normalizer=nz)
    with pytest.raises(_lib.TsidbError, match="PolicyNormalizer: this normaliser already belongs"):
        PolicyActor(env, mlp(env.NOBS, 8, env.NA), normalizer=nz)


def test_state_dict_round_trip_and_its_shape_checks():
    from tsid_control_amd import _lib
    env, calls, pa, nz = build(eps=0.02)
    NOBS = env.NOBS
    g = torch.Generator().manual_seed(5)
    for st in (nz.actor, nz.critic):
        st.stats[0] = torch.randn(st.K, generator=g, dtype=torch.float64) * 3
        st.stats[1] = torch.rand(st.K, generator=g, dtype=torch.float64) + 0.01
        st.count.fill_(12345)
        st.fill_affine()
    sd = nz.state_dict()
    assert sorted(sd) == ["critic_obs_normalizer", "obs_normalizer"]
    for key, st in (("obs_normalizer", nz.actor), ("critic_obs_normalizer", nz.critic)):
        d = sd[key]
        assert sorted(d) == ["_mean", "_std", "_var", "count"]
        assert d["_mean"].shape == d["_var"].shape == d["_std"].shape == (1, st.K) and d["count"].shape == () and d["count"].dtype == torch.int64
        assert torch.equal(d["_std"], torch.sqrt(d["_var"])) and d["_mean"].data_ptr() != st.stats.data_ptr()
    env2, calls2, pb, nz2 = build(eps=0.02)
    nz2.load_state_dict(sd)
    assert calls2 == []                                      # torch ops only
    for a, b in zip(nz.written()[:-1], nz2.written()[:-1]):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
    want = R.affine32(nz.actor.stats[0].numpy(), nz.actor.stats[1].numpy(), 0.02)
    assert (nz2.actor.affine.numpy() == want).all()
    # rsl_rl's own buffers are float32 with an int64 scalar count: they load too
    f32 = {k: {n: (t.float() if t.is_floating_point() else t) for n, t in d.items()} for k, d in sd.items()}
    nz2.load_state_dict(f32)
    assert torch.equal(nz2.actor.stats[0], sd["obs_normalizer"]["_mean"][0].float().double()) and nz2.critic.count.item() == 12345
    # shapes that do not match K, missing pieces
    def changed(key, name, value):
        out = {k: dict(d) for k, d in sd.items()}
        if name is None:
            del out[key]
        else:
            out[key][name] = value
        return out
    z = torch.zeros
    bad = [(changed("obs_normalizer", "_mean", z(1, NOBS + 1, dtype=torch.float64)), r"obs_normalizer: _mean must be a \[1, %d\]" % NOBS),
           (changed("obs_normalizer", "_var", z(NOBS, dtype=torch.float64)), r"obs_normalizer: _var must be a \[1, %d\]" % NOBS),
           (changed("critic_obs_normalizer", "_mean", z(1, NOBS, dtype=torch.float64)), r"critic_obs_normalizer: _mean must be a \[1, %d\]" % (NOBS + 4)),
           (changed("critic_obs_normalizer", "_std", z(1, NOBS, dtype=torch.float64)), "critic_obs_normalizer: _std must be"),
           (changed("obs_normalizer", "_mean", z(1, NOBS, dtype=torch.int64)), "obs_normalizer: _mean must be"),
           (changed("obs_normalizer", "count", z(2, dtype=torch.int64)), "obs_normalizer: count must be"),
           (changed("obs_normalizer", "count", torch.tensor(3.0)), "obs_normalizer: count must be"),
           (changed("critic_obs_normalizer", None, None), "state has no 'critic_obs_normalizer'"),
           ([], "state must be a dict")]
    before = [t.clone() for t in nz2.written()]
    for state, msg in bad:
        with pytest.raises(_lib.TsidbError, match="PolicyNormalizer: " + msg):
            nz2.load_state_dict(state)
    for a, b in zip(nz2.written(), before):
        assert torch.equal(a, b)                             # a rejected dict changes nothing, the actor's half included
