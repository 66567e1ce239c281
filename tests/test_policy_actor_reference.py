"""tests/policy_actor_reference.py pinned by its properties: float32 evaluations (numpy, torch.nn.Sequential on the CPU) stay
inside its forward error bound against its float64 values, the float64 values are torch's, the Box-Muller draw has the moments
of a standard normal, and the advantage recursion equals the direct double sum."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_actor_reference as R  # noqa: E402
from policy_dr_reference import draw  # noqa: E402

ACT = {"elu": torch.nn.ELU, "tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}


def sequential(layers, act, dtype):
    mods = []
    for i, (w, b) in enumerate(layers):
        lin = torch.nn.Linear(w.shape[1], w.shape[0]).to(dtype)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w).to(dtype))
            lin.bias.copy_(torch.from_numpy(b).to(dtype))
        mods.append(lin)
        if i + 1 < len(layers):
            mods.append(ACT[act]())
    return torch.nn.Sequential(*mods)


@pytest.mark.parametrize("na", [20, 18])
@pytest.mark.parametrize("name", ["tanh3", "elu_wide", "single", "relu_critic"])
def test_float32_evaluations_stay_inside_the_bound(na, name):
    blocks, widths, act = R.network_cases(na)[name]
    rng = np.random.default_rng(100 * na + sorted(R.network_cases(na)).index(name))
    k = sum(c for _, c in blocks)
    layers = R.make_layers(rng, k, widths)
    for n in (1, 17, 33):
        x = R.assemble([rng.normal(0, 1.5, (n, c)) for _, c in blocks])
        y, bnd = R.forward_bound(x, layers, act)
        assert y.shape == (n, widths[-1]) and (bnd > 0).all() and bnd.max() < 1e-2      # (worst case, yet far below the O(1) outputs)
        y32 = R.forward(x, layers, act, np.float32)
        assert y32.dtype == np.float32
        with torch.no_grad():
            t32 = sequential(layers, act, torch.float32)(torch.from_numpy(x.astype(np.float32))).numpy()
            t64 = sequential(layers, act, torch.float64)(torch.from_numpy(x)).numpy()
        for got in (y32, t32):
            ratio = np.abs(got.astype(np.float64) - y) / bnd
            assert ratio.max() < 1.0, (name, n, ratio.max())
        assert np.abs(t64 - y).max() < 1e-13


def test_sample_and_logp_in_float32_stay_inside_the_bound():
    rng = np.random.default_rng(3)
    na, n = 20, 33
    mean = rng.normal(0, 1, (n, na))
    b_mean = 1e-6 * np.abs(mean)
    ls = rng.uniform(-2, 0.5, na).astype(np.float32)
    e64 = R.eps(7, np.arange(n) + 5, np.full(n, 2), np.arange(n), na)
    s = R.sample(mean, b_mean, ls, e64)
    m32, e32 = mean.astype(np.float32), e64.astype(np.float32)
    a32 = m32 + np.exp(ls) * e32
    assert (np.abs(a32 - s["action"]) <= s["b_action"] + np.abs(m32 - mean)).all()
    lp32 = np.float32(0)
    for a in range(na):
        lp32 = lp32 + (np.float32(0.5) * e32[:, a] * e32[:, a] + ls[a])
    lp32 = -lp32 - np.float32(0.5 * na * R.LN_2PI)
    assert lp32.dtype == np.float32 and (np.abs(lp32 - s["logp"]) <= s["b_logp"]).all()
    # the density: logp is that of a normal with mean, sigma at the action
    sig = np.exp(ls.astype(np.float64))
    want = (-0.5 * ((s["action"] - mean) / sig) ** 2 - np.log(sig) - 0.5 * R.LN_2PI).sum(1)
    assert np.abs(want - s["logp"]).max() < 1e-9
    d = R.sample(mean, b_mean, ls, None)
    assert (d["action"] == mean).all() and (d["b_action"] == b_mean).all() and (d["eps32"] == 0).all()
    assert np.abs(d["logp"] - (-ls.astype(np.float64).sum() - 0.5 * na * R.LN_2PI)).max() < 1e-12


def test_eps_is_a_standard_normal_and_finite():
    n = 2 ** 16 // 16
    e = R.eps(11, np.arange(n), np.ones(n, dtype=np.int64), np.zeros(n, dtype=np.int64), 16).reshape(-1)
    assert e.size == 2 ** 16 and np.isfinite(e).all()
    assert abs(e.mean()) < 0.02 and abs(e.var() - 1) < 0.03
    # U1 = 0 (the smallest draw) maps to ln 1 = 0: eps = 0, not a non-finite value
    assert np.sqrt(-2.0 * np.log(1.0 - 0.0)) * np.cos(0.3) == 0.0
    assert np.isfinite(np.sqrt(-2.0 * np.log(1.0 - (1.0 - 2.0 ** -53))))
    # the two uniforms are different streams, and a column, an env, a step each change the draw
    base = R.eps(11, [3], [1], [4], 2)
    assert base[0, 0] != base[0, 1]
    for other in (R.eps(12, [3], [1], [4], 2), R.eps(11, [4], [1], [4], 2), R.eps(11, [3], [2], [4], 2), R.eps(11, [3], [1], [5], 2)):
        assert (other != base).all()
    assert (R.eps(11, [3], [1], [4], 2) == base).all()
    u1 = draw(11, R.S_U1, 0, np.array([3]), np.array([(1 << 32) | 4], dtype=np.uint64))
    u2 = draw(11, R.S_U2, 0, np.array([3]), np.array([(1 << 32) | 4], dtype=np.uint64))
    assert base[0, 0] == np.sqrt(-2.0 * np.log(1.0 - u1[0])) * np.cos(2.0 * np.pi * u2[0])


def gae_direct(reward, done, timeout, value, gamma, lam):
    """A_t = sum_{s >= t} (gamma lam)^(s - t) prod_{t <= j < s} (1 - done_j) delta_s, term by term"""
    T, n = reward.shape
    delta = reward + gamma * value[:-1] * timeout + gamma * value[1:] * (1 - done) - value[:-1]
    adv = np.zeros((T, n))
    for t in range(T):
        for s in range(t, T):
            alive = np.prod(1 - done[t:s], axis=0) if s > t else 1.0
            adv[t] += (gamma * lam) ** (s - t) * alive * delta[s]
    return adv, adv + value[:-1]


def test_gae_equals_the_direct_sum():
    rng = np.random.default_rng(5)
    T, n = 9, 6
    reward, value = rng.normal(0, 1, (T, n)), rng.normal(0, 2, (T + 1, n))
    done, timeout = np.zeros((T, n)), np.zeros((T, n), dtype=np.int32)
    done[3, 0] = done[4, 1] = done[T - 1, 2] = done[T - 1, 3] = done[2, 4] = done[3, 4] = 1
    timeout[4, 1] = timeout[T - 1, 3] = timeout[3, 4] = 1       # a timeout in the middle and at the last step
    for gamma, lam in ((0.99, 0.95), (0.99, 0.0), (0.0, 0.95)):
        adv, ret = R.gae(reward, done, timeout, value, gamma, lam)
        want_adv, want_ret = gae_direct(reward, done, timeout.astype(np.float64), value, gamma, lam)
        assert np.abs(adv - want_adv).max() < 1e-12 and np.abs(ret - want_ret).max() < 1e-12
    # lam = 0: A = delta; a done cuts the bootstrap, a timeout adds gamma V_t back
    adv, _ = R.gae(reward, done, timeout, value, 0.99, 0.0)
    assert adv[3, 0] == reward[3, 0] - value[3, 0]
    assert adv[4, 1] == reward[4, 1] + 0.99 * value[4, 1] - value[4, 1]
    a32, r32 = R.gae(reward, done, timeout, value, 0.99, 0.95, np.float32)
    assert a32.dtype == np.float32 and np.abs(a32 - R.gae(reward, done, timeout, value, 0.99, 0.95)[0]).max() < 1e-4
