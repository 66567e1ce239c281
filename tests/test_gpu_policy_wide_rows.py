"""Rows wider than 480 columns need more than the default 64 KB of dynamic LDS, and the library raises the limit once per handle
and KERNEL: the actor's launch with and without a normaliser, and the learner's rows kernel in its plain, imitation and symmetry
variants - five kernels.  A handle that took one kernel's raised limit for another's would have the second wide launch refused
(an invalid-value error from the launch, no fault), so two handles run all five in different orders and must agree bit for bit:
which kernel's limit was raised first changes no arithmetic."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from policy_testlib import make_env, same  # noqa: E402

pytestmark = pytest.mark.gpu

N, FRAMES, T = 17, 7, 2


def run(flip):
    """every wide launch on a fresh handle; flip: the normalised actor before the plain one, the three learners in reverse.
    Returns {name: tensor} of everything the calls wrote."""
    from tsid_control_amd import PolicyActor, PolicyLearner, PolicyNormalizer, PolicyObsHistory, PolicySymmetry
    env = make_env(N, "f64", obs_history=PolicyObsHistory(FRAMES, ("obs",)))
    K = FRAMES * env.NOBS
    assert K == 497 and env.obs_history.shape == (N, K)              # (more than 480: every rows / actor kernel is past 64 KB)
    torch.manual_seed(11)
    mlp = lambda out: torch.nn.Sequential(torch.nn.Linear(K, 16), torch.nn.ELU(), torch.nn.Linear(16, out)).to("cuda:0")
    actor, critic = mlp(env.NA), mlp(1)
    kw = dict(actor_inputs=("obs_history",), seed=5)
    pa = PolicyActor(env, actor, critic, **kw)
    pn = PolicyActor(env, actor, critic, normalizer=PolicyNormalizer(), **kw)
    out = {}

    def act(name, p):
        o = p.act()
        out.update({f"{name}.{k}": o[k].clone() for k in ("action", "logp", "value")})
    for name, p in (("normed", pn), ("plain", pa)) if flip else (("plain", pa), ("normed", pn)):
        act(name, p)
    st = env.rollout(pa, T)
    st.gae()
    index = torch.arange(T * N, dtype=torch.int32, device="cuda:0")
    learners = [("plain", lambda: PolicyLearner(pa)), ("imit", lambda: PolicyLearner(pa, surrogate_coef=0.5)),
                ("sym", lambda: PolicyLearner(pa, symmetry=PolicySymmetry(env, pa)))]
    for name, make in learners[::-1] if flip else learners:
        pl = make()
        out[f"{name}.stats"] = pl.backward(st, index).clone()
        out.update({f"{name}.grad{i}": p.grad.clone() for i, p in enumerate(pl.parameters())})
        if name == "imit":
            out["imit.imit_stats"] = pl.imit_stats.clone()
        if name == "sym":
            out["sym.sym_stats"] = pl.sym_stats.clone()
    torch.cuda.synchronize()
    return out


def test_five_wide_kernels_on_one_handle_in_either_order_agree_bit_for_bit():
    a, b = run(False), run(True)
    assert sorted(a) == sorted(b) and len(a) == 6 + 3 * (1 + 9) + 2
    for k in a:
        assert same(a[k], b[k]), k
    assert all(bool(torch.isfinite(a[f"{v}.stats"]).all()) for v in ("plain", "imit", "sym"))
    assert float(a["plain.grad0"].abs().max()) > 0 and not same(a["plain.grad0"], a["imit.grad0"])     # (the variants did run)
