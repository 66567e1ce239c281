"""The numpy restatement of the policy learner (tests/policy_learner_reference.py) against torch's CPU autograd of the loss
expression in float64, on every case the GPU test uses; e32(case), the error of torch's float32 autograd that is the GPU test's
yardstick; and the cases' distance from the loss's kinks.  No GPU, no library."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_learner_reference as R  # noqa: E402

ACT = {"elu": torch.nn.functional.elu, "tanh": torch.tanh, "relu": torch.relu}
LN_2PI = float(np.log(2.0 * np.pi))


def torch_grads(case, dtype):
    """(loss, [(name, gradient)] in grad_list's order) of the loss expression by torch.autograd on the CPU, everything in dtype"""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    idx = np.asarray(case["index"]).astype(np.int64)
    j = torch.from_numpy(idx[(idx >= 0) & (idx < case["rows"])])
    M, c = len(idx), case["clip"]
    params = {}

    def net(which, x):
        layers, act = case[which]
        for l, (w, b) in enumerate(layers):
            W = params[f"{which}.{l}.weight"] = t(w).requires_grad_()
            x = x @ W.T
            if b is not None:
                B = params[f"{which}.{l}.bias"] = t(b).requires_grad_()
                x = x + B
            if l + 1 < len(layers):
                x = ACT[act](x)
        return x
    mu = net("actor", t(case["actor_input"])[j])
    v = net("critic", t(case["critic_input"])[j])[:, 0] if case["critic"] is not None else None
    ls = params["log_std"] = t(case["log_std"]).requires_grad_()
    z = (t(case["action"])[j] - mu) / torch.exp(ls)
    logp = -(z * z / 2 + ls).sum(1) - case["na"] * LN_2PI / 2
    r = torch.exp(logp - t(case["logp"])[j])
    adv = t(case["advantage"])[j]
    if case["adv_stats"] is not None:
        st = t(case["adv_stats"])
        adv = (adv - st[0]) * st[1]
    l_pi = torch.max(-adv * r, -adv * torch.clamp(r, 1 - c, 1 + c)).sum() / M
    l_v = torch.zeros((), dtype=dtype)
    if v is not None:
        old, ret = t(case["value"])[j], t(case["returns"])[j]
        l_v = (v - ret) ** 2
        if case["value_clip"]:
            l_v = torch.max(l_v, (old + torch.clamp(v - old, -c, c) - ret) ** 2)
        l_v = l_v.sum() / M
    entropy = (ls + (1 + LN_2PI) / 2).sum()
    loss = l_pi + case["value_coef"] * l_v - case["entropy_coef"] * entropy
    loss.backward()
    return float(loss.detach()), [(k, p.grad.numpy().astype(np.float64)) for k, p in params.items()], \
        np.array([float(l_pi.detach()), float(l_v.detach()), float(entropy.detach())])


def e32(case):
    """(E, stats error): the largest max|g32 - g64| / max|g64| over the parameter tensors of torch's CPU float32 autograd against
    its float64 autograd - what an honest float32 implementation of this case loses"""
    _, g64, _ = torch_grads(case, torch.float64)
    _, g32, _ = torch_grads(case, torch.float32)
    worst = 0.0
    for (k, a), (k2, b) in zip(g64, g32):
        assert k == k2
        scale = float(np.abs(a).max())
        if scale > 0:
            worst = max(worst, float(np.abs(a - b).max()) / scale)
    return worst


@pytest.fixture(scope="module")
def evaluated():
    return {name: (case, R.evaluate(case)) for name, case in ((n, R.make_case(n)) for n in R.CASES)}


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_is_torch_float64_autograd(name, evaluated):
    case, ev = evaluated[name]
    loss, grads, parts = torch_grads(case, torch.float64)
    assert abs(ev["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(ev["stats"][:3] - parts).max() <= 1e-12 * max(1.0, np.abs(parts).max())
    mine = dict(R.grad_list(ev))
    assert sorted(mine) == sorted(k for k, _ in grads)
    for k, g in grads:
        scale = np.abs(g).max()
        assert mine[k].shape == g.shape and np.abs(mine[k] - g).max() <= 1e-12 * max(scale, 1e-300), (k, np.abs(mine[k] - g).max() / scale)
    if name == "all_ties":
        assert (ev["l1"] == ev["l2"]).all() and np.abs(ev["r"] - 1).max() < 1e-5


def test_bad_indices_are_left_out_and_counted():
    case = R.make_case("tanh_relu_17")
    bad = dict(case, index=np.concatenate([case["index"][:5], [-1], case["index"][5:], [case["rows"]]]).astype(np.int32))
    a, b = R.evaluate(case), R.evaluate(bad)
    assert list(b["stats"][6:]) == [17, 2] and list(a["stats"][6:]) == [17, 0]
    for (k, ga), (_, gb) in zip(R.grad_list(a)[:-1], R.grad_list(b)[:-1]):
        assert np.abs(ga * 17 / 19 - gb).max() <= 1e-13 * np.abs(gb).max(), k
    loss, grads, _ = torch_grads(bad, torch.float64)
    assert abs(b["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_cases_stay_away_from_the_kinks(name, evaluated):
    """in the float64 reference: every ratio 1e-3 from 1 +- c, every |v - value| 1e-3 from c, l1 and l2 1e-6 apart or equal, every
    ReLU pre-activation 1e-4 from 0; and in the cases of 16 rows or more that are no ties, between a quarter and all but one of
    the rows outside the clip range (a single row cannot be on both sides)"""
    case, ev = evaluated[name]
    d = R.conditions(case, ev)
    print(name, d, "e32", e32(case))
    assert d["ratio"] >= 1e-3
    assert d.get("value", 1.0) >= 1e-3 and d.get("l1_l2", 1.0) >= 1e-6 and d.get("relu", 1.0) >= 1e-4
    if name != "all_ties" and case["M"] >= 16:
        assert 0.25 <= d["clipped"] < 1.0
    assert len(set(case["index"].tolist())) < case["M"] or case["M"] < 4      # repeats
