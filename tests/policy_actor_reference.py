"""Numpy restatement of the policy actor (tsidb_policy_actor / tsidb_policy_gae), written from their description in
include/tsidb.h: the input row from its column blocks, the dense layers in a chosen dtype, the three activations, the
Box-Muller draw on streams 21 / 22 of the randomisation's key layout, action, log-probability and value, and the advantage
recursion.  No torch, no library.

Beside the float64 values it carries a worst-case FORWARD ERROR BOUND for a float32 implementation, computed in float64
(u = 2^-24, the unit roundoff of float32):
    input cast            b = u |x|
    layer, fan-in K       b_out = (K + 2) u (|W| |x| + |b|) + |W| b_in        (K products and sums, the bias, one to spare)
    activation            b <- b + 4 u |y|                                       (ELU, tanh, ReLU are 1-Lipschitz; 4 ulp: expm1f / tanhf)
    sample                b_action = b_mean + 4 u (|mean| + |sigma eps|)         (expf, the product, the sum, eps itself)
    log-probability       b_logp = (NA + 2) u (sum_a (eps_a^2 / 2 + |log_std_a|) + NA ln(2 pi) / 2)
tests/test_policy_actor_reference.py shows that honest float32 implementations stay inside it."""
import numpy as np

from policy_dr_reference import counter_hi_lo, draw

U32 = 2.0 ** -24
S_U1, S_U2 = 21, 22
ACTIVATIONS = ("elu", "tanh", "relu")
LN_2PI = float(np.log(2.0 * np.pi))


def assemble(blocks, dtype=np.float64):
    """the input rows [n, K] from the column blocks [n, k_i], cast to dtype"""
    return np.concatenate([np.asarray(b) for b in blocks], axis=1).astype(dtype)


def activation(name, x):
    if name == "elu":
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    if name == "tanh":
        return np.tanh(x)
    if name == "relu":
        return np.maximum(x, 0)
    raise ValueError(name)


def forward(x, layers, act, dtype=np.float64):
    """the network on the rows x [n, K] with everything in dtype: layers = [(weight [out, in], bias [out] or None)], the hidden
    activation after every layer but the last"""
    y = np.asarray(x).astype(dtype)
    for i, (w, b) in enumerate(layers):
        y = y @ np.asarray(w).astype(dtype).T
        if b is not None:
            y = y + np.asarray(b).astype(dtype)
        if i + 1 < len(layers):
            y = activation(act, y).astype(dtype)
    return y.astype(dtype)


def forward_bound(x, layers, act):
    """(y, bound) in float64: the network on the rows x (the env's values, before the cast to float32) and the forward error
    bound of a float32 evaluation, element by element"""
    y = np.asarray(x, dtype=np.float64)
    bnd = U32 * np.abs(y)
    for i, (w, b) in enumerate(layers):
        w = np.asarray(w, dtype=np.float64)
        k = w.shape[1]
        mag = np.abs(y) @ np.abs(w).T
        bnd = bnd @ np.abs(w).T
        y = y @ w.T
        if b is not None:
            b = np.asarray(b, dtype=np.float64)
            y = y + b
            mag = mag + np.abs(b)
        bnd = (k + 2) * U32 * mag + bnd
        if i + 1 < len(layers):
            y = activation(act, y)
            bnd = bnd + 4 * U32 * np.abs(y)
    return y, bnd


def eps(seed, env, episode, ep_len, na):
    """[n, na] float64: sqrt(-2 ln(1 - U1)) cos(2 pi U2), U1 / U2 = streams 21 / 22, column = actuator, env = the GLOBAL env
    indices (env_offset added), counter = episode * 2^32 + ep_len"""
    env = np.atleast_1d(np.asarray(env)).astype(np.int64)
    ctr = counter_hi_lo(episode, ep_len)
    out = np.empty((len(env), na))
    for a in range(na):
        u1, u2 = draw(seed, S_U1, a, env, ctr), draw(seed, S_U2, a, env, ctr)
        out[:, a] = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)
    return out


def sample(mean, b_mean, log_std, eps64=None):
    """dict(action, b_action, logp, b_logp, eps32) in float64 from the mean [n, na] and its bound; eps64 None = deterministic
    (action = mean, eps = 0).  eps is cast to float32 once, as the device casts it; log_std is the float32 parameter"""
    mean, b_mean = np.asarray(mean, dtype=np.float64), np.asarray(b_mean, dtype=np.float64)
    ls = np.asarray(log_std, dtype=np.float32).astype(np.float64)
    na = mean.shape[1]
    e = np.zeros_like(mean) if eps64 is None else np.asarray(eps64).astype(np.float32).astype(np.float64)
    if eps64 is None:
        action, b_action = mean.copy(), b_mean.copy()
    else:
        se = np.exp(ls) * e
        action = mean + se
        b_action = b_mean + 4 * U32 * (np.abs(mean) + np.abs(se))
    logp = -(0.5 * e * e + ls).sum(1) - 0.5 * na * LN_2PI
    b_logp = (na + 2) * U32 * ((0.5 * e * e + np.abs(ls)).sum(1) + 0.5 * na * LN_2PI)
    return dict(action=action, b_action=b_action, logp=logp, b_logp=b_logp, eps32=e)


def gae(reward, done, timeout, value, gamma, lam, dtype=np.float64):
    """(advantage, returns) [T, n] in dtype: reward, done, timeout [T, n], value [T + 1, n]
        r'_t = r_t + gamma V_t timeout_t;  delta_t = r'_t + gamma V_{t+1} (1 - done_t) - V_t
        A_t = delta_t + gamma lam (1 - done_t) A_{t+1}, A_T = 0;  returns_t = A_t + V_t"""
    r, d, to, v = (np.asarray(x).astype(dtype) for x in (reward, done, timeout, value))
    g, l, one = dtype(gamma), dtype(lam), dtype(1)
    T = r.shape[0]
    adv, ret = np.zeros_like(r), np.zeros_like(r)
    nxt = np.zeros(r.shape[1], dtype=dtype)
    for t in range(T - 1, -1, -1):
        nd = one - d[t]
        rp = r[t] + g * v[t] * to[t]
        delta = rp + g * v[t + 1] * nd - v[t]
        nxt = delta + g * l * nd * nxt
        adv[t] = nxt
        ret[t] = nxt + v[t]
    return adv, ret


# ---------------------------------------------------------------------------- the networks the tests share
def network_cases(na):
    """{name: (input blocks [(name, columns)], widths, activation)} for a robot with na actuators: widths that are no tile
    multiples, the widest layer with three blocks and more than 128 inputs, a single layer, and a critic"""
    nobs = 11 + 3 * na
    return {
        "tanh3": ([("obs", nobs)], [24, 40, na], "tanh"),
        "elu_wide": ([("obs", nobs), ("height_scan", 77), ("teacher_obs", 14 + na)], [512, na], "elu"),
        "single": ([("obs", nobs)], [na], "elu"),
        "relu_critic": ([("obs", nobs), ("priv", 4)], [33, 1], "relu"),
    }


def make_layers(rng, fan_in, widths):
    """[(weight, bias)] float32, uniform in +-1 / sqrt(fan-in)"""
    layers = []
    for w in widths:
        a = 1.0 / np.sqrt(fan_in)
        layers.append((rng.uniform(-a, a, (w, fan_in)).astype(np.float32), rng.uniform(-a, a, w).astype(np.float32)))
        fan_in = w
    return layers
