"""The numpy restatement of the learner's mirror symmetry (tests/policy_symmetry_reference.py) against torch's CPU autograd in
float64 of the same loss written the rsl_rl way - the minibatch and its mirror image concatenated into one batch, the mirror
loss an MSE against the detached, mirrored mean of the original half - on every case the GPU test uses; e32(case), the error of
torch's float32 autograd that is the GPU test's yardstick; and the cases' distance from the loss's kinks.  No GPU, no library."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_symmetry_reference as S  # noqa: E402
from test_policy_learner_reference import ACT, LN_2PI  # noqa: E402


def _mirror(x, table):
    perm, sign = torch.from_numpy(np.asarray(table[0]).astype(np.int64)), torch.from_numpy(np.asarray(table[1])).to(x.dtype)
    ok = (perm >= 0) & (perm < x.shape[1])                  # (a perm entry outside the row: a zero column)
    return x[:, torch.where(ok, perm, torch.zeros_like(perm))] * sign * ok.to(x.dtype)


def torch_grads(case, dtype):
    """(loss, [(name, gradient)] in grad_list's order, (L_pi, L_v, entropy, L_sym)) by torch.autograd on the CPU, all in dtype"""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    idx = np.asarray(case["index"]).astype(np.int64)
    j = torch.from_numpy(idx[(idx >= 0) & (idx < case["rows"])])
    M, c, m, aug = len(idx), case["clip"], len(j), case["augment"]
    params = {}

    def net(which, x):
        layers, act = case[which]
        for l, (w, b) in enumerate(layers):
            W = params.get(f"{which}.{l}.weight")
            if W is None:
                W = params[f"{which}.{l}.weight"] = t(w).requires_grad_()
            x = x @ W.T
            if b is not None:
                B = params.get(f"{which}.{l}.bias")
                if B is None:
                    B = params[f"{which}.{l}.bias"] = t(b).requires_grad_()
                x = x + B
            if l + 1 < len(layers):
                x = ACT[act](x)
        return x
    two = lambda x: torch.cat([x, x])
    x = t(case["actor_input"])[j]
    mu_all = net("actor", torch.cat([x, _mirror(x, case["actor_table"])]))          # the concatenated batch
    a = t(case["action"])[j]
    a_all = torch.cat([a, _mirror(a, case["action_table"])])
    n = 2 * m if aug else m                                                           # the rows of the surrogate and the value loss
    denom = 2 * M if aug else M
    v = None
    if case["critic"] is not None:
        xc = t(case["critic_input"])[j]
        v = net("critic", torch.cat([xc, _mirror(xc, case["critic_table"])])[:n])[:, 0]
    ls = params["log_std"] = t(case["log_std"]).requires_grad_()
    z = (a_all[:n] - mu_all[:n]) / torch.exp(ls)
    logp = -(z * z / 2 + ls).sum(1) - case["na"] * LN_2PI / 2
    rep = two if aug else (lambda y: y)
    r = torch.exp(logp - rep(t(case["logp"])[j]))
    adv = rep(t(case["advantage"])[j])
    if case["adv_stats"] is not None:
        st = t(case["adv_stats"])
        adv = (adv - st[0]) * st[1]
    l_pi = torch.max(-adv * r, -adv * torch.clamp(r, 1 - c, 1 + c)).sum() / denom
    l_v = torch.zeros((), dtype=dtype)
    if v is not None:
        old, ret = rep(t(case["value"])[j]), rep(t(case["returns"])[j])
        l_v = (v - ret) ** 2
        if case["value_clip"]:
            l_v = torch.max(l_v, (old + torch.clamp(v - old, -c, c) - ret) ** 2)
        l_v = l_v.sum() / denom
    entropy = (ls + (1 + LN_2PI) / 2).sum()
    target = _mirror(mu_all[:m].detach(), case["action_table"])
    l_sym = ((mu_all[m:] - target) ** 2).sum() / (M * case["na"])
    loss = l_pi + case["value_coef"] * l_v - case["entropy_coef"] * entropy
    if case["mirror_coef"] > 0:
        loss = loss + case["mirror_coef"] * l_sym
    loss.backward()
    order = [k for k in params if k != "log_std"] + ["log_std"]
    return float(loss.detach()), [(k, params[k].grad.numpy().astype(np.float64)) for k in order], \
        np.array([float(l_pi.detach()), float(l_v.detach()), float(entropy.detach()), float(l_sym.detach())])


def e32(case):
    """the largest max|g32 - g64| / max|g64| over the parameter tensors of torch's CPU float32 autograd against its float64
    autograd - what an honest float32 implementation of this case loses"""
    _, g64, _ = torch_grads(case, torch.float64)
    _, g32, _ = torch_grads(case, torch.float32)
    worst = 0.0
    for (k, a), (k2, b) in zip(g64, g32):
        assert k == k2
        scale = float(np.abs(a).max())
        if scale > 0:
            worst = max(worst, float(np.abs(a - b).max()) / scale)
    return worst


VARIANTS = [(name, {}) for name in sorted(S.CASES)] + \
    [("aug_17", dict(augment=a, mirror_coef=c)) for a in (False, True) for c in (0.0, 0.5)]


@pytest.mark.parametrize("name,over", VARIANTS, ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()) or "case")
def test_restatement_is_torch_float64_autograd(name, over):
    case = S.make_case(name, **over)
    ev = S.evaluate(case)
    loss, grads, parts = torch_grads(case, torch.float64)
    assert abs(ev["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    mine_parts = np.array([ev["stats"][0], ev["stats"][1], ev["stats"][2], ev["mirror_loss"]])
    assert np.abs(mine_parts - parts).max() <= 1e-12 * max(1.0, np.abs(parts).max())
    mine = dict(S.grad_list(ev))
    assert sorted(mine) == sorted(k for k, _ in grads)
    for k, g in grads:
        scale = np.abs(g).max()
        assert mine[k].shape == g.shape and np.abs(mine[k] - g).max() <= 1e-12 * max(scale, 1e-300), (k, np.abs(mine[k] - g).max() / scale)
    j, M = S.R.rows_of(case)
    assert list(ev["stats"][6:]) == [(2 if case["augment"] else 1) * len(j), M - len(j)] and list(ev["sym_stats"][1:]) == [len(j)]
    assert ev["mirror_loss"] > 1e-3                # (random networks are not symmetric: the term is alive)


def test_the_tables_are_involutions_and_the_term_vanishes_for_an_identity():
    for name in S.CASES:
        case = S.make_case(name)
        for k in ("actor_table", "critic_table", "action_table"):
            if case[k] is None:
                continue
            perm, sign = case[k]
            assert np.array_equal(perm[perm], np.arange(len(perm))) and np.array_equal(sign[perm], sign) and set(np.abs(sign)) == {1.0}
            x = np.random.default_rng(1).normal(0, 1, (3, len(perm))).astype(np.float32)
            assert np.array_equal(S.mirror(S.mirror(x, case[k]), case[k]), x)
        assert (case["actor_table"][0] != np.arange(len(case["actor_table"][0]))).any() and (case["actor_table"][1] < 0).any()
    case = S.make_case("aug_17")
    ident = lambda k: (np.arange(k, dtype=np.int32), np.ones(k, dtype=np.float32))
    same = dict(case, actor_table=ident(case["actor_input"].shape[1]), action_table=ident(case["na"]))
    assert S.evaluate(same)["mirror_loss"] <= 1e-28     # (0 but for the matrix product's blocking of two memory layouts)
    # a perm entry outside the row is a zero column
    x = np.arange(6, dtype=np.float32).reshape(2, 3) + 1
    assert np.array_equal(S.mirror(x, ([2, -1, 3], [1.0, 1.0, -1.0])), np.array([[3, 0, 0], [6, 0, 0]], dtype=np.float32))


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_cases_stay_away_from_the_kinks(name):
    """in the float64 reference, over the virtual rows (the mirrored ones with augment): every ratio 1e-3 from 1 +- c, every
    |v - value| 1e-3 from c, l1 and l2 1e-6 apart or equal, every ReLU pre-activation 1e-4 from 0"""
    case = S.make_case(name)
    ev = S.evaluate(case)
    d = S.conditions(case, ev)
    print(name, d, "e32", e32(case))
    assert d["ratio"] >= 1e-3
    assert d.get("value", 1.0) >= 1e-3 and d.get("l1_l2", 1.0) >= 1e-6 and d.get("relu", 1.0) >= 1e-4
    if case["M"] >= 16:
        assert 0.25 <= d["clipped"] <= 1.0
