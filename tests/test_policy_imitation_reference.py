"""The numpy restatement of the imitation slice (tests/policy_imitation_reference.py) against torch's CPU float64 autograd of the
extended loss - F.mse_loss / F.huber_loss per element with per-row weights, the surrogate masked on the executed rows and scaled
by surrogate_coef, every mean over M - at 1e-12, the bound the learner's restatement is held to; e32(case), the error of torch's
float32 autograd that is the GPU test's yardstick; the cases' distance from the Huber kink; and the mix kernel's restatement
against its description.  No GPU, no library."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_dr_reference as DR  # noqa: E402
import policy_imitation_reference as RI  # noqa: E402
import policy_learner_reference as R  # noqa: E402
from test_policy_learner_reference import ACT, LN_2PI  # noqa: E402


def torch_grads(case, dtype):
    """(loss, [(name, gradient)] in grad_list's order, (L_pi, L_v, entropy, L_im)) by torch.autograd on the CPU, everything in dtype"""
    F = torch.nn.functional
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    idx = np.asarray(case["index"]).astype(np.int64)
    j = torch.from_numpy(idx[(idx >= 0) & (idx < case["rows"])])
    M, c, na = len(idx), case["clip"], case["na"]
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
    logp = -(z * z / 2 + ls).sum(1) - na * LN_2PI / 2
    r = torch.exp(logp - t(case["logp"])[j])
    adv = t(case["advantage"])[j]
    if case["adv_stats"] is not None:
        st = t(case["adv_stats"])
        adv = (adv - st[0]) * st[1]
    keep = torch.ones(len(j), dtype=torch.bool) if case["skip"] is None else torch.from_numpy(np.asarray(case["skip"]))[j] == 0
    l_pi = torch.max(-adv * r, -adv * torch.clamp(r, 1 - c, 1 + c))[keep].sum() / M
    l_v = torch.zeros((), dtype=dtype)
    if v is not None:
        old, ret = t(case["value"])[j], t(case["returns"])[j]
        l_v = (v - ret) ** 2
        if case["value_clip"]:
            l_v = torch.max(l_v, (old + torch.clamp(v - old, -c, c) - ret) ** 2)
        l_v = l_v.sum() / M
    entropy = (ls + (1 + LN_2PI) / 2).sum()
    w = torch.ones(len(j), dtype=dtype) if case["weight"] is None else t(case["weight"])[j]
    use = w != 0
    target = t(case["target"])[j][use]
    assert bool(torch.isfinite(target).all())
    fn = F.mse_loss if case["imit_loss"] == "mse" else F.huber_loss         # (delta = 1, the default)
    l_im = (w[use] * fn(mu[use], target, reduction="none").mean(1)).sum() / M
    loss = case["surrogate_coef"] * l_pi + case["value_coef"] * l_v - case["entropy_coef"] * entropy + case["imitation_coef"] * l_im
    loss.backward()
    zero = lambda p: p.grad if p.grad is not None else torch.zeros_like(p)
    return float(loss.detach()), [(k, zero(p).numpy().astype(np.float64)) for k, p in params.items()], \
        np.array([float(x.detach()) for x in (l_pi, l_v, entropy, l_im)])


def e32(case):
    """the largest max|g32 - g64| / max|g64| over the parameter tensors of torch's CPU float32 autograd against its float64
    autograd of the extended loss: what an honest float32 implementation of this case loses"""
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
    return {name: (case, RI.evaluate(case)) for name, case in ((n, RI.make_case(n)) for n in RI.CASES)}


@pytest.mark.parametrize("name", sorted(RI.CASES))
def test_restatement_is_torch_float64_autograd(name, evaluated):
    case, ev = evaluated[name]
    loss, grads, parts = torch_grads(case, torch.float64)
    assert abs(ev["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    mine_parts = np.array([ev["stats"][0], ev["stats"][1], ev["stats"][2], ev["imit_stats"][0]])
    assert np.abs(mine_parts - parts).max() <= 1e-12 * max(1.0, np.abs(parts).max())
    assert ev["stats"][5] == ev["loss"]
    mine = dict(RI.grad_list(ev))
    assert sorted(mine) == sorted(k for k, _ in grads)
    for k, g in grads:
        scale = np.abs(g).max()
        assert mine[k].shape == g.shape
        assert np.abs(mine[k] - g).max() <= 1e-12 * max(scale, 1e-300), (k, np.abs(mine[k] - g).max() / max(scale, 1e-300))
    # pure distillation: nothing for the critic and log_std, something for the actor
    if case["surrogate_coef"] == 0 and case["value_coef"] == 0 and case["entropy_coef"] == 0:
        assert not np.abs(mine["log_std"]).max() and all(not np.abs(g).max() for k, g in mine.items() if k.startswith("critic"))
        assert np.abs(mine["actor.0.weight"]).max() > 0


@pytest.mark.parametrize("name", sorted(RI.CASES))
def test_cases_cover_both_branches_weights_and_executed_rows(name, evaluated):
    """every used |mu - target| at least 0.04 from the Huber kink at 1 and from 0, both branches present where the case has more
    than one row; weights 0 (behind NaN labels), 1 and fractional, and executed rows, among the rows the index names; the counts"""
    case, ev = evaluated[name]
    m = RI.margins(case, ev)
    print(name, m, "e32", e32(case))
    assert m["kink"] >= 0.04 and m["zero"] >= 0.04
    j, M = R.rows_of(case)
    if len(j) > 1:
        assert m["quadratic"] > 0.3 and m["linear"] > 0.2
    if case["weight"] is not None and len(j) >= 3:
        w, s = case["weight"][j], case["skip"][j]
        assert (w == 0).any() and (w == 1).any() and ((w > 0) & (w < 1)).any() and (s != 0).any() and (s == 0).any()
        assert np.isnan(case["target"][case["weight"] == 0]).all() and np.isfinite(case["target"][case["weight"] != 0]).all()
        assert list(ev["imit_stats"][1:]) == [float(w.astype(np.float64).sum()), float((w > 0).sum()), float((s != 0).sum())]
    else:
        assert list(ev["imit_stats"][1:]) == [len(j), len(j), 0]
    assert list(ev["stats"][6:]) == [len(j), M - len(j)]
    if name == "huber_segments_bad":
        assert M - len(j) == 2 and M == R.SEG_ROWS + 19


def test_term_off_is_the_learners_restatement():
    """imitation_coef = 0, surrogate_coef = 1, no skipped row: policy_learner_reference.evaluate, exactly - whatever the labels hold"""
    case = RI.make_case("mse_17")
    off = dict(case, imitation_coef=0.0, surrogate_coef=1.0, skip=None, target=np.full_like(case["target"], np.nan), weight=None)
    a, b = R.evaluate(case), RI.evaluate(dict(off, target=None))
    assert a["loss"] == b["loss"] and np.array_equal(a["stats"], b["stats"])
    for (k, ga), (_, gb) in zip(R.grad_list(a), RI.grad_list(b)):
        assert np.array_equal(ga, gb), k
    # an executed row leaves the surrogate and its statistics, not the value loss
    one = np.zeros(case["rows"], dtype=np.int32)
    one[case["index"][3]] = 1
    c = RI.evaluate(dict(off, target=None, skip=one))
    assert c["imit_stats"][3] == 1 and c["stats"][1] == a["stats"][1] and c["stats"][0] != a["stats"][0] and c["stats"][6] == a["stats"][6]


def test_mix_restatement():
    """labels are the float32 cast; weight and executed need ep_len > 0; beta 0 executes nothing, beta 1 every live env; the draw
    is stream 23, column 0, counter episode * 2^32, env index env_offset + e: a split batch draws what the whole one draws, an
    episode keeps its draw whatever ep_len, the next episode draws anew"""
    rng = np.random.default_rng(3)
    n, na = 64, 20
    ta, act = rng.normal(0, 1, (n, na)), rng.normal(0, 1, (n, na))
    ep_len, episode = rng.integers(0, 3, n), rng.integers(1, 5, n)
    label, weight, executed, out = RI.mix(ta, act, ep_len, episode, 0.5, seed=11)
    assert label.dtype == np.float32 and np.array_equal(label, ta.astype(np.float32))
    assert np.array_equal(weight, (ep_len > 0).astype(np.float32)) and weight.dtype == np.float32 and executed.dtype == np.int32
    u = DR.draw(11, 23, 0, np.arange(n, dtype=np.uint64), episode.astype(np.uint64) << np.uint64(32))
    assert np.array_equal(executed, ((u < 0.5) & (ep_len > 0)).astype(np.int32)) and 0 < executed.sum() < (ep_len > 0).sum()
    assert np.array_equal(out[executed == 1], ta[executed == 1]) and np.array_equal(out[executed == 0], act[executed == 0])
    assert not RI.mix(ta, act, ep_len, episode, 0.0, 11)[2].any() and not RI.mix(ta, act, ep_len, episode, None, 11)[2].any()
    assert np.array_equal(RI.mix(ta, act, ep_len, episode, 1.0, 11)[2], (ep_len > 0).astype(np.int32))
    lo, hi = RI.mix(ta[:32], act[:32], ep_len[:32], episode[:32], 0.5, 11), RI.mix(ta[32:], act[32:], ep_len[32:], episode[32:], 0.5, 11, env_offset=32)
    assert np.array_equal(np.concatenate([lo[2], hi[2]]), executed)
    live = np.maximum(ep_len, 1)
    assert np.array_equal(RI.mix(ta, act, live, episode, 0.5, 11)[2], RI.mix(ta, act, live + 7, episode, 0.5, 11)[2])
    assert not np.array_equal(RI.mix(ta, act, live, episode, 0.5, 11)[2], RI.mix(ta, act, live, episode + 1, 0.5, 11)[2])
    assert not np.array_equal(RI.mix(ta, act, live, episode, 0.5, 11)[2], RI.mix(ta, act, live, episode, 0.5, 12)[2])
