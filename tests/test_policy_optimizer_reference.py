"""The float64 restatement of the policy optimiser (tests/policy_optimizer_reference.py) against torch on the CPU in float64, at
1e-12 relative, on every case the device is run on and over its 5 consecutive steps: the norm and the clip factor against
torch.nn.utils.clip_grad_norm_, parameters and moments against torch.optim.Adam behind it, the KL against
torch.distributions.kl_divergence of two Normals.  And the cases' distance from the kinks of the rules they exercise: that is
how they were built, here it is asserted.  Also e32(): what torch's CPU float32 pipeline loses on a case - the yardstick of
tests/test_gpu_policy_optimizer.py."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_optimizer_reference as R  # noqa: E402


@functools.lru_cache(maxsize=None)
def case_of(name):
    """(case, [(state, stats)] of the restatement's STEPS steps), computed once per process and left unchanged"""
    case = R.make_case(name)
    return case, R.run(case)


def torch_run(case, dtype, lrs, steps=R.STEPS):
    """clip_grad_norm_ and torch.optim.Adam on the CPU in `dtype`, with lr set to lrs[k] before step k.  Per step:
    dict(norm, clipped = the gradients behind the clip, params, exp_avg, exp_avg_sq), lists in the order of the parameters"""
    o = case["opt"]
    cfg = o["cfg"]
    params = [torch.tensor(np.asarray(a), dtype=dtype) for _, a in R.param_list(case)]
    opt = torch.optim.Adam(params, lr=float(lrs[0]), betas=(cfg["b1"], cfg["b2"]), eps=cfg["eps"])
    out = []
    for k in range(steps):
        for p, g in zip(params, o["grads"][k]):
            p.grad = torch.tensor(g, dtype=dtype).reshape(p.shape)
        norm = torch.nn.utils.clip_grad_norm_(params, cfg["max_norm"] if cfg["max_norm"] > 0 else float("inf"))
        opt.param_groups[0]["lr"] = float(lrs[k])
        clipped = [p.grad.double().numpy().copy() for p in params]
        opt.step()
        f = lambda t: t.detach().double().numpy().copy()
        out.append(dict(norm=float(norm), clipped=clipped, params=[f(p) for p in params], exp_avg=[f(opt.state[p]["exp_avg"]) for p in params],
                        exp_avg_sq=[f(opt.state[p]["exp_avg_sq"]) for p in params]))
    return out


def e32(name):
    """{step: E}: the largest max|x32 - x64| / max|x64| over the parameters and both moments of torch's CPU float32
    clip_grad_norm_ + Adam against the restatement, after 1 .. STEPS steps of the case"""
    case, ref = case_of(name)
    t32 = torch_run(case, torch.float32, [st["lr"] for st, _ in ref])
    out = {}
    for k, ((state, _), got) in enumerate(zip(ref, t32)):
        worst = 0.0
        for key in ("params", "exp_avg", "exp_avg_sq"):
            for a, b in zip(state[key], got[key]):
                worst = max(worst, float(np.abs(a - b).max() / np.abs(a).max()))
        out[k + 1] = worst
    return out


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_is_torch_float64_clip_and_adam(name):
    case, ref = case_of(name)
    pure = R.run(case, cast_coef=False)                        # (torch keeps the clip factor in float64)
    t64 = torch_run(case, torch.float64, [st["lr"] for st, _ in ref])
    for k, ((state, stats), got) in enumerate(zip(pure, t64)):
        assert abs(stats[0] - got["norm"]) <= 1e-12 * got["norm"], k
        for g, c in zip(case["opt"]["grads"][k], got["clipped"]):
            assert np.abs(stats[1] * g.astype(np.float64).reshape(c.shape) - c).max() <= 1e-12 * np.abs(c).max(), k
        for key in ("params", "exp_avg", "exp_avg_sq"):
            for (pname, _), a, b in zip(R.param_list(case), state[key], got[key]):
                assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (k, key, pname, np.abs(a - b).max() / np.abs(b).max())
        # the float32 cast of the clip factor is all that separates the device's contract from torch's float64 pipeline
        cast = ref[k][1]
        assert cast[0] == stats[0] and cast[1] == stats[1] and abs(float(np.float32(cast[1])) - cast[1]) <= 2.0 ** -24 * cast[1]
        assert stats[4] == k + 1 and stats[5] == 0


@pytest.mark.parametrize("name", sorted(n for n in R.CASES if R.CASES[n][2]))
def test_kl_is_torch_kl_divergence_of_two_normals(name):
    from torch.distributions import Normal, kl_divergence
    case, ref = case_of(name)
    o = case["opt"]
    idx = case["index"].astype(np.int64)
    ok = (idx >= 0) & (idx < case["rows"])
    d = lambda a: torch.tensor(np.asarray(a, dtype=np.float32)).double()
    state = R.new_state([a for _, a in R.param_list(case)], o["lr"])
    for k in range(R.STEPS):
        ls = state["params"][-1].astype(np.float32)
        old = Normal(d(o["mean"][idx[ok]]), torch.exp(d(o["log_std_old"])))
        new = Normal(d(o["mu"][k][ok]), torch.exp(d(ls)))
        want = float(kl_divergence(old, new).sum(-1).sum() / len(idx))
        state, stats = ref[k]
        assert abs(stats[2] - want) <= 1e-12 * max(1.0, abs(want)), (k, stats[2], want)
        assert stats[6] == ok.sum()
    assert (not ok.all()) == (name == "segments_bad")


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_cases_stay_off_the_kinks_and_move_lr_as_designed(name):
    """every step's kl at least 1e-3 relative from 2 desired_kl and desired_kl / 2, its norm from max_norm; clipping active in
    some steps and inactive in others; lr goes up, is held by lr_max, stays, goes down, is held by lr_min"""
    case, ref = case_of(name)
    cfg = case["opt"]["cfg"]
    lrs, dirs = [np.float32(R.LR)], []
    for k, (state, stats) in enumerate(ref):
        if cfg["max_norm"] > 0:
            assert abs(stats[0] - cfg["max_norm"]) >= 1e-3 * cfg["max_norm"], k
            assert (stats[1] < 1.0) == (R.NORMS[k] > 1.0), k
        else:
            assert stats[1] == 1.0 and stats[0] > 0
        if cfg["desired_kl"]:
            for kink in (2.0 * cfg["desired_kl"], cfg["desired_kl"] / 2.0):
                assert abs(stats[2] - kink) >= 1e-3 * kink, (k, stats[2])
            assert abs(stats[2] - R.KLS[k] * cfg["desired_kl"]) <= 1e-4 * cfg["desired_kl"], (k, stats[2])
        else:
            assert stats[2] == 0 and stats[6] == 0 and stats[7] == 0 and state["lr"] == np.float32(R.LR)
        lrs.append(state["lr"])
        dirs.append(int(stats[7]))
        assert stats[3] == state["lr"] and state["lr"].dtype == np.float32
    if cfg["desired_kl"]:
        f = np.float32
        assert R.LR_MOVES == ("up", "pinned at lr_max", "unchanged", "down", "pinned at lr_min")
        assert lrs[1] == f(f(R.LR) * f(1.5)) and lrs[2] == f(R.LR_MAX) < f(lrs[1] * f(1.5)) and lrs[3] == lrs[2]
        assert lrs[4] == f(lrs[3] / f(1.5)) and lrs[5] == f(R.LR_MIN) > f(lrs[4] / f(1.5))
        assert dirs == [1, 1, 0, -1, -1]
        # held by a bound with nowhere to go: the direction is 0
        assert R.lr_rule(R.LR_MIN, 1.0, cfg["desired_kl"], R.LR_MIN, R.LR_MAX) == (f(R.LR_MIN), 0)
        assert R.lr_rule(R.LR_MAX, cfg["desired_kl"] / 4, cfg["desired_kl"], R.LR_MIN, R.LR_MAX) == (f(R.LR_MAX), 0)


def test_lr_rule_is_float32_arithmetic():
    for lr in (1e-2, 1.5e-2, 3e-4, 1e-3):
        t = torch.tensor(lr, dtype=torch.float32)
        assert float(R.lr_rule(lr, 1.0, 0.01, 1e-9, 1.0)[0]) == float(t / 1.5)
        assert float(R.lr_rule(lr, 1e-3, 0.01, 1e-9, 1.0)[0]) == float(t * 1.5)
        assert R.lr_rule(lr, 0.01, 0.01, 1e-9, 1.0) == (np.float32(lr), 0) and R.lr_rule(lr, 0.0, 0.01, 1e-9, 1.0)[1] == 0


def test_a_chunk_sum_has_the_headers_order_and_the_norm_is_the_plain_one():
    rng = np.random.default_rng(0)
    g = rng.normal(0, 1, 2 * R.CHUNK + 5).astype(np.float32)
    sums = R.chunk_sums(g)
    assert sums.shape == (3,)
    x = np.zeros(R.CHUNK)
    x[:5] = g[2 * R.CHUNK:].astype(np.float64) ** 2
    slots = [((x[4 * t] + x[4 * t + 1]) + x[4 * t + 2]) + x[4 * t + 3] for t in range(R.LANES)]
    s = R.LANES // 2
    while s >= 1:
        slots = [slots[t] + slots[t + s] for t in range(s)]
        s //= 2
    assert sums[2] == slots[0]
    assert abs(R.grad_norm([g[:7], g[7:]]) - np.linalg.norm(g.astype(np.float64))) <= 1e-13 * np.linalg.norm(g.astype(np.float64))


def test_skip_keeps_the_state_and_without_it_the_step_poisons_as_torchs_does():
    case, _ = case_of("tanh_relu_17")
    o = case["opt"]
    state = R.new_state([a for _, a in R.param_list(case)], o["lr"])
    grads = [g.copy() for g in o["grads"][0]]
    grads[0].reshape(-1)[3] = np.inf
    after, stats = R.step(state, grads, o["cfg"], R.kl_input(case, 0))
    assert after is state and stats[5] == 1 and stats[4] == 0 and stats[3] == state["lr"] and stats[7] == 0 and np.isinf(stats[0])
    after, stats = R.step(state, grads, dict(o["cfg"], skip_nonfinite=False), R.kl_input(case, 0))
    assert stats[5] == 0 and after["step"] == 1 and np.isnan(after["params"][0].reshape(-1)[3])
    # torch: the clip factor is 0, 0 * inf = NaN in that element, every other gradient becomes 0
    bad = dict(case, opt=dict(o, grads=[grads]))
    got = torch_run(bad, torch.float64, [after["lr"]], steps=1)[0]
    for a, b in zip(after["params"], got["params"]):
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b))
