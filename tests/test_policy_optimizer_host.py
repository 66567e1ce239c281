"""The policy optimiser (tsidb_policy_opt_step, PolicyOptimizer), the parts that need no GPU: the binding against the header, both
libraries' exports, the call step() makes with its pointers, what update() calls with and without a PolicyOptimizer, the
checkpoint's layout, and what the host rejects."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_testlib import HEADER, assert_prototypes, header_enums  # noqa: E402
from test_policy_learner_host import learner_setup  # noqa: E402

NAMES = ("tsidb_policy_opt_workspace", "tsidb_policy_opt_step")
ROOT_CSRC = Path(__file__).resolve().parent.parent / "tsid_control_amd" / "csrc"


def test_binding_matches_the_header():
    from tsid_control_amd import _lib
    import policy_optimizer_reference as R
    en = header_enums("TSIDB_POL_OPT_")
    assert _lib.POL_OPT_CHUNK == en["TSIDB_POL_OPT_CHUNK"] == R.CHUNK == 1024
    assert _lib.POL_OPT_LANES == en["TSIDB_POL_OPT_LANES"] == R.LANES and R.CHUNK == 4 * R.LANES and R.SEG_ROWS == 2 * R.LANES == _lib.POL_LEARN_SEG_ROWS
    assert len(_lib.POL_OPT_STATS) == en["TSIDB_POL_OPT_NSTATS"] == 8 and _lib.POL_OPT_STATS == R.STATS
    for cname, struct in (("tsidb_policy_opt_cfg", _lib.PolicyOptCfg), ("tsidb_policy_opt_state", _lib.PolicyOptState),
                          ("tsidb_policy_opt_kl", _lib.PolicyOptKl)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), HEADER, re.S)
        fields = re.findall(r"\b(\w+)(?:\[4\])?;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
        assert fields == [f[0] for f in struct._fields_], cname
    assert C.sizeof(_lib.PolicyOptCfg) == 5 * 8 + 3 * 4 + 4 and C.sizeof(_lib.PolicyOptState) == 40 and C.sizeof(_lib.PolicyOptKl) == 3 * 8 + 8
    # the structs of the learner and of the actor did not grow
    assert C.sizeof(_lib.PolicyLearnBatch) == 8 * 8 + 4 + 4 + 8 and C.sizeof(_lib.PolicyGrads) == 64 and C.sizeof(_lib.PolicyLearnCfg) == 16
    assert C.sizeof(_lib.PolicyNet) == 4 + 16 + 4 + 32 + 32 + 4 + 4 + 32 + 16 + 16
    assert_prototypes(NAMES)
    assert (ROOT_CSRC / "tsidb_optim.hpp").exists()
    assert "int tsidb_policy_opt_step(" in (ROOT_CSRC / "tsidb_api.hip").read_text()


def test_step_is_a_workspace_query_and_one_call_with_the_learners_last_minibatch_behind_it():
    import tsid_control_amd
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_optimizer import PolicyOptimizer
    assert tsid_control_amd.PolicyOptimizer is PolicyOptimizer
    env, calls, pa, st, pl = learner_setup()
    opt = PolicyOptimizer(pl, lr=3e-3, betas=(0.8, 0.99), eps=1e-6, max_grad_norm=0.5, desired_kl=0.02, lr_min=1e-4, lr_max=5e-3)
    params = pl.parameters()
    assert opt.P == sum(p.numel() for p in params) and opt.moments.shape == (2, opt.P) and opt.moments.dtype == torch.float32
    assert opt.lr.dtype == torch.float32 and opt.lr.shape == (1,) and float(opt.lr) == float(torch.tensor(3e-3, dtype=torch.float32))
    assert opt.step_count.dtype == torch.int64 and opt.step_count.shape == (1,) and int(opt.step_count) == 0
    assert opt.stats.shape == (8,) and opt.log_std_old.shape == (env.NA,) and opt.log_std_old is not pa.log_std and opt.log is None
    with pytest.raises(_lib.TsidbError, match="PolicyOptimizer: no backward\\(\\) has run"):
        opt.step()
    assert not calls
    index = torch.tensor([4, 0, 5, 5], dtype=torch.int32)
    pl.backward(st, index)
    del calls[:]
    stats = opt.step()
    assert stats is opt.stats
    assert [c[0] for c in calls] == ["tsidb_policy_opt_workspace", "tsidb_policy_opt_step"]
    q = calls[0][1]
    assert len(q) == 4 and q[2] == 4 and q[0]._obj is pa.actor_net.struct and q[1]._obj is pa.critic_net.struct
    a = calls[1][1]
    assert len(a) == 12                                             # (+ the handle: the header's 13)
    assert a[0]._obj is pa.actor_net.struct and a[1]._obj is pa.critic_net.struct
    for arg, net in ((a[2], pa.actor_net), (a[3], pa.critic_net)):
        g = C.cast(arg, C.POINTER(_lib.PolicyGrads)).contents
        for l, (w, b) in enumerate(net.layers):
            assert (g.weight[l], g.bias[l]) == (w.grad.data_ptr(), b.grad.data_ptr())
            assert (net.struct.weight[l], net.struct.bias[l]) == (w.data_ptr(), b.data_ptr())
        assert g.weight[2] is None and g.bias[2] is None
    assert (a[4].value, a[5].value) == (pa.log_std.data_ptr(), pa.log_std.grad.data_ptr())
    cfg = C.cast(a[6], C.POINTER(_lib.PolicyOptCfg)).contents
    assert (cfg.b1, cfg.b2, cfg.eps, cfg.max_norm, cfg.desired_kl, cfg.skip_nonfinite) == (0.8, 0.99, 1e-6, 0.5, 0.02, 1)
    assert (cfg.lr_min, cfg.lr_max) == (C.c_float(1e-4).value, C.c_float(5e-3).value)
    state = C.cast(a[7], C.POINTER(_lib.PolicyOptState)).contents
    assert (state.moments, state.lr, state.step, state.log_std_old, state.stats) == \
        tuple(t.data_ptr() for t in (opt.moments, opt.lr, opt.step_count, opt.log_std_old, opt.stats))
    kl = C.cast(a[8], C.POINTER(_lib.PolicyOptKl)).contents
    assert (kl.mu, kl.mean, kl.index, kl.rows, kl.M) == (pl.workspace.data_ptr(), st.mean.data_ptr(), index.data_ptr(), 2 * 3, 4)
    assert a[9].value == opt.workspace.data_ptr() and a[10].value == opt.workspace.numel() * 8
    # the moments' views, in the order of parameters()
    off = 0
    for p in params:
        for which, view in ((0, opt.exp_avg(p)), (1, opt.exp_avg_sq(p))):
            assert view.shape == p.shape and view.data_ptr() == opt.moments[which, off:].data_ptr()
        off += p.numel()
    with pytest.raises(_lib.TsidbError, match="PolicyOptimizer: not a parameter"):
        opt.exp_avg(torch.zeros(3))
    ptrs = [t.data_ptr() for t in opt.written()]
    assert ptrs == [t.data_ptr() for t in params + [opt.moments, opt.lr, opt.step_count, opt.stats, opt.workspace]]
    assert not any(t.requires_grad for t in opt.written()) and any(p.requires_grad for p in params)
    # a smaller minibatch reuses the workspace, a larger one asks again; the log takes the rows of the next steps, then stats again
    del calls[:]
    opt.log = torch.zeros(2, 8)
    pl.backward(st, index[:2])
    r0 = opt.step()
    pl.backward(st, torch.zeros(5, dtype=torch.int32))
    r1 = opt.step()
    r2 = opt.step()
    assert [c[0] for c in calls if "opt" in c[0]] == ["tsidb_policy_opt_step", "tsidb_policy_opt_workspace", "tsidb_policy_opt_step", "tsidb_policy_opt_step"]
    steps = [c[1] for c in calls if c[0] == "tsidb_policy_opt_step"]
    assert [C.cast(s[7], C.POINTER(_lib.PolicyOptState)).contents.stats for s in steps] == [opt.log[0].data_ptr(), opt.log[1].data_ptr(), opt.stats.data_ptr()]
    assert r0.data_ptr() == opt.log[0].data_ptr() and r1.data_ptr() == opt.log[1].data_ptr() and r2 is opt.stats
    assert [C.cast(s[8], C.POINTER(_lib.PolicyOptKl)).contents.M for s in steps] == [2, 5, 5] and opt.written()[-1] is opt.log
    # without the schedule and the clip, without a critic: no KL inputs, no workspace rows
    env, calls, pa, st, pl = learner_setup(critic=False)
    opt = PolicyOptimizer(pl, max_grad_norm=None, desired_kl=None, skip_nonfinite=False)
    pl.backward(st, index)
    del calls[:]
    opt.step()
    assert calls[0][0] == "tsidb_policy_opt_workspace" and calls[0][1][1] is None and calls[0][1][2] == 0
    a = calls[1][1]
    assert a[1] is None and a[3] is None and a[8] is None
    cfg = C.cast(a[6], C.POINTER(_lib.PolicyOptCfg)).contents
    assert (cfg.b1, cfg.b2, cfg.eps, cfg.max_norm, cfg.desired_kl, cfg.skip_nonfinite) == (0.9, 0.999, 1e-8, 0.0, 0.0, 0)


def test_update_with_a_policy_optimizer_is_a_snapshot_and_a_learn_and_a_step_per_slice():
    from tsid_control_amd.policy_optimizer import PolicyOptimizer
    env, calls, pa, st, pl = learner_setup(T=3)
    opt = PolicyOptimizer(pl, desired_kl=0.01)
    with torch.no_grad():
        pa.log_std.fill_(-0.3)
    assert float(opt.log_std_old.abs().max()) == 0
    inner = opt.snapshot

    def snapshot():
        calls.append(("snapshot", ()))
        inner()
    opt.snapshot = snapshot
    pl.update(st, opt, epochs=2, minibatches=4, generator=torch.Generator().manual_seed(3))
    names = [c[0] for c in calls if not c[0].endswith("_workspace")]
    assert names == ["snapshot"] + ["tsidb_policy_learn", "tsidb_policy_opt_step"] * 8
    assert torch.equal(opt.log_std_old, pa.log_std) and opt.log_std_old is not pa.log_std
    # each step reads the minibatch of the backward() before it
    from tsid_control_amd import _lib
    learn = [c[1] for c in calls if c[0] == "tsidb_policy_learn"]
    steps = [c[1] for c in calls if c[0] == "tsidb_policy_opt_step"]
    for l, s in zip(learn, steps):
        batch = C.cast(l[2], C.POINTER(_lib.PolicyLearnBatch)).contents
        kl = C.cast(s[8], C.POINTER(_lib.PolicyOptKl)).contents
        assert (kl.index, kl.M, kl.rows, kl.mean, kl.mu) == (batch.index, batch.M, batch.rows, st.mean.data_ptr(), l[8].value)


def test_update_with_a_step_only_optimizer_makes_exactly_the_calls_it_made():
    env, calls, pa, st, pl = learner_setup(T=3)

    class Steps:
        n = 0

        def step(self):
            self.n += 1
    opt = Steps()
    pl.update(st, opt, epochs=2, minibatches=4, generator=torch.Generator().manual_seed(3))
    # Ms = 2, 2, 2, 3: the workspace is asked for at the first slice and again at the first larger one
    assert [c[0] for c in calls] == ["tsidb_policy_learn_workspace"] + ["tsidb_policy_learn"] * 3 + ["tsidb_policy_learn_workspace"] + \
        ["tsidb_policy_learn"] * 5 and opt.n == 8
    assert pl.parameters()[-1] is pa.log_std and len(pl.parameters()) == 9
    assert {id(t) for t in pl.written()} == {id(p.grad) for p in pl.parameters()} | {id(pl.stats), id(pl.adv_stats), id(pl.workspace)}
    # a torch optimiser has no snapshot(): update() asks before it calls
    assert not hasattr(torch.optim.Adam(pl.parameters()), "snapshot")


def test_state_dict_has_torch_adams_layout_and_moves_both_ways():
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_optimizer import PolicyOptimizer
    env, calls, pa, st, pl = learner_setup()
    params = pl.parameters()
    opt = PolicyOptimizer(pl, lr=2e-3, betas=(0.8, 0.99), eps=1e-6)
    sd = opt.state_dict()
    assert sd["state"] == {} and len(sd["param_groups"]) == 1
    twin = torch.optim.Adam(params, lr=1.0)
    assert set(sd["param_groups"][0]) == set(twin.state_dict()["param_groups"][0])
    g = sd["param_groups"][0]
    assert g["params"] == list(range(len(params))) and g["betas"] == (0.8, 0.99) and g["eps"] == 1e-6 and g["weight_decay"] == 0 and not g["amsgrad"]
    assert g["lr"] == float(torch.tensor(2e-3, dtype=torch.float32))
    # stepped: the state of every parameter
    gen = torch.Generator().manual_seed(0)
    opt.moments.copy_(torch.rand(opt.moments.shape, generator=gen))
    opt.step_count.fill_(7)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(len(params)))
    for i, p in enumerate(params):
        s = sd["state"][i]
        assert sorted(s) == ["exp_avg", "exp_avg_sq", "step"] and float(s["step"]) == 7 and s["step"].dtype == torch.float32 and s["step"].dim() == 0
        assert torch.equal(s["exp_avg"], opt.exp_avg(p)) and torch.equal(s["exp_avg_sq"], opt.exp_avg_sq(p)) and s["exp_avg"].shape == p.shape
        assert s["exp_avg"].data_ptr() != opt.exp_avg(p).data_ptr()
    # into torch.optim.Adam
    twin.load_state_dict(sd)
    assert twin.param_groups[0]["lr"] == g["lr"] and twin.param_groups[0]["betas"] == (0.8, 0.99)
    for p in params:
        assert torch.equal(twin.state[p]["exp_avg"], opt.exp_avg(p)) and float(twin.state[p]["step"]) == 7
    # and back, from torch's own dict, into a fresh optimiser
    for p in params:
        twin.state[p]["exp_avg_sq"].mul_(2.0)
        twin.state[p]["step"] += 1
    twin.param_groups[0]["lr"] = 5e-4
    other = PolicyOptimizer(pl)
    other.load_state_dict(twin.state_dict())
    assert int(other.step_count) == 8 and float(other.lr) == float(torch.tensor(5e-4, dtype=torch.float32)) and other.betas == (0.8, 0.99) and other.eps == 1e-6
    assert torch.equal(other.moments[0], opt.moments[0]) and torch.equal(other.moments[1], opt.moments[1] * 2.0)
    assert (other._cfg.b1, other._cfg.b2, other._cfg.eps) == (0.8, 0.99, 1e-6)
    fresh = PolicyOptimizer(pl)
    fresh.moments.fill_(1.0)
    fresh.load_state_dict(torch.optim.Adam(params, lr=1e-3).state_dict())
    assert int(fresh.step_count) == 0 and float(fresh.moments.abs().max()) == 0
    for sd_bad, msg in ((dict(state={}, param_groups=[]), "one param group"), (dict(twin.state_dict(), param_groups=[dict(g, params=[0, 1])]), "2 parameters"),
                        (dict(state={}, param_groups=[dict(g, weight_decay=0.1)]), "weight_decay, amsgrad and maximize are not built"),
                        (dict(state={}, param_groups=[dict(g, amsgrad=True)]), "not built")):
        with pytest.raises(_lib.TsidbError, match="PolicyOptimizer: .*" + msg):
            other.load_state_dict(sd_bad)


def test_rejected_arguments_raise_with_a_message():
    from tsid_control_amd import _lib
    from tsid_control_amd.policy_optimizer import PolicyOptimizer
    env, calls, pa, st, pl = learner_setup()
    inf, nan = float("inf"), float("nan")
    for kw, msg in ((dict(lr=0), "lr must be > 0"), (dict(lr=-1e-3), "lr must be > 0"), (dict(lr="a"), "lr must be a finite number"), (dict(lr=nan), "lr must be a finite number"),
                    (dict(betas=0.9), "betas must be a pair"), (dict(betas=(0.9,)), "betas must be a pair"), (dict(betas=(1.0, 0.999)), "betas\\[0\\] must be < 1"),
                    (dict(betas=(0.9, -0.1)), "betas\\[1\\] must be >= 0"), (dict(betas=(0.9, inf)), "betas\\[1\\] must be a finite number"),
                    (dict(eps=0), "eps must be > 0"), (dict(eps=-1e-8), "eps must be > 0"), (dict(max_grad_norm=-1), "max_grad_norm must be >= 0"),
                    (dict(max_grad_norm=inf), "max_grad_norm must be a finite number"), (dict(desired_kl=0), "desired_kl must be > 0"),
                    (dict(desired_kl=-0.01), "desired_kl must be > 0"), (dict(desired_kl=True), "desired_kl must be a finite number"),
                    (dict(lr_min=0), "lr_min must be > 0"), (dict(lr_max=nan), "lr_max must be a finite number"),
                    (dict(lr_min=1e-2, lr_max=1e-3), "lr_min must be <= lr_max"), (dict(skip_nonfinite=1), "skip_nonfinite must be a bool")):
        with pytest.raises(_lib.TsidbError, match="PolicyOptimizer: " + msg):
            PolicyOptimizer(pl, **kw)
    with pytest.raises(_lib.TsidbError, match="PolicyOptimizer: learner must be a PolicyLearner"):
        PolicyOptimizer(pa)
    opt = PolicyOptimizer(pl)
    for log in (torch.zeros(8), torch.zeros(2, 7), torch.zeros(2, 8, dtype=torch.float64), torch.zeros(2, 16)[:, ::2], [0.0] * 8):
        with pytest.raises(_lib.TsidbError, match="PolicyOptimizer: log must be"):
            opt.log = log
    pl.backward(st, torch.zeros(4, dtype=torch.int32))
    pa.actor_net.layers[0][0].grad = torch.zeros(env.NOBS, 8).t()
    with pytest.raises(_lib.TsidbError, match="PolicyLearner: a .grad must be a contiguous float32"):
        opt.step()
    assert not [c for c in calls if c[0] == "tsidb_policy_opt_step"]
