"""Numpy float64 restatement of the policy learner (tsidb_policy_learn), written from its description in include/tsidb.h: the
forward pass with every layer kept, rsl_rl's PPO loss on a minibatch of stored rows, and the gradient by the chain rule with
torch.autograd's tie rules spelled out (a max of two equal terms gives each half; clamp passes the gradient on its bounds).
No torch, no library.  Also the cases the tests share: tests/test_policy_learner_reference.py checks the restatement against
torch's float64 autograd and the cases' distance from the loss's kinks, tests/test_gpu_policy_learner.py runs them on the device.
"""
import numpy as np

from policy_actor_reference import LN_2PI, activation, make_layers

SEG_ROWS = 512          # TSIDB_POL_LEARN_SEG_ROWS
STATS = ("policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "loss", "rows", "bad_indices")


def act_prime(name, y):
    """the activation's derivative from its output"""
    if name == "elu":
        return np.where(y > 0, 1.0, y + 1.0)
    if name == "tanh":
        return 1.0 - y * y
    if name == "relu":
        return (y > 0).astype(np.float64)
    raise ValueError(name)


def forward_all(x, layers, act):
    """(H, pre): the rows after each layer (activated but for the last) and each layer's pre-activations, float64"""
    H, pre, y = [], [], np.asarray(x, dtype=np.float64)
    for i, (w, b) in enumerate(layers):
        y = y @ np.asarray(w, dtype=np.float64).T
        if b is not None:
            y = y + np.asarray(b, dtype=np.float64)
        pre.append(y)
        if i + 1 < len(layers):
            y = activation(act, y)
        H.append(y)
    return H, pre


def backward_net(x, layers, act, H, g_last):
    """[(dW, db)] of the layers from the gradient of the loss with respect to the network's output rows"""
    out, g = [None] * len(layers), g_last
    for l in range(len(layers) - 1, -1, -1):
        w, b = layers[l]
        h_prev = H[l - 1] if l else np.asarray(x, dtype=np.float64)
        out[l] = (g.T @ h_prev, g.sum(0) if b is not None else None)
        if l:
            g = (g @ np.asarray(w, dtype=np.float64)) * act_prime(act, H[l - 1])
    return out


def rows_of(case):
    """(j, M): the stored rows of the usable minibatch entries, and the length of index - the M of the means"""
    idx = np.asarray(case["index"]).astype(np.int64)
    return idx[(idx >= 0) & (idx < case["rows"])], len(idx)


def evaluate(case):
    """dict(loss, stats [8], actor [(dW, db)], critic [(dW, db)] or None, log_std [na], and the per-row r, v, v_old, l1, l2, mu,
    logp, pre (hidden pre-activations of both networks) the case conditions look at), all float64"""
    f = lambda k: np.asarray(case[k], dtype=np.float64)
    j, M = rows_of(case)
    c, vc, ec, na = case["clip"], case["value_coef"], case["entropy_coef"], case["na"]
    ls = f("log_std")
    sigma = np.exp(ls)
    layers, act = case["actor"]
    xa = f("actor_input")[j]
    H, pre_a = forward_all(xa, layers, act)
    mu = H[-1]
    z = (f("action")[j] - mu) / sigma
    logp = -(0.5 * z * z + ls).sum(1) - 0.5 * na * LN_2PI
    old = f("logp")[j]
    r = np.exp(logp - old)
    adv = f("advantage")[j]
    if case["adv_stats"] is not None:
        st = f("adv_stats")
        adv = (adv - st[0]) * st[1]
    t1, t2 = -adv * r, -adv * np.clip(r, 1 - c, 1 + c)
    inside = (r >= 1 - c) & (r <= 1 + c)
    l_pi = np.maximum(t1, t2).sum() / M
    dr = np.where(inside | (t1 > t2), -adv / M, 0.0)
    dlogp = r * dr
    g_mu = dlogp[:, None] * z / sigma
    entropy = (ls + 0.5 * (1 + LN_2PI)).sum()
    out = dict(actor=backward_net(xa, layers, act, H, g_mu), critic=None, log_std=(dlogp[:, None] * (z * z - 1)).sum(0) - ec, r=r, mu=mu,
               logp=logp, pre=pre_a[:-1], v=None)
    l_v = 0.0
    if case["critic"] is not None:
        layers, act = case["critic"]
        xc = f("critic_input")[j]
        H, pre_c = forward_all(xc, layers, act)
        v, v_old, ret = H[-1][:, 0], f("value")[j], f("returns")[j]
        l1 = (v - ret) ** 2
        raw, row = 2 * (v - ret), l1
        l2 = l1
        if case["value_clip"]:
            d = v - v_old
            v_clip = v_old + np.clip(d, -c, c)
            ins = (np.abs(d) <= c).astype(np.float64)
            l2 = (v_clip - ret) ** 2
            raw = np.where(l1 > l2, 2 * (v - ret), np.where(l1 < l2, 2 * (v_clip - ret) * ins, (v - ret) + (v_clip - ret) * ins))
            row = np.maximum(l1, l2)
        l_v = row.sum() / M
        out.update(critic=backward_net(xc, layers, act, H, (raw * vc / M)[:, None]), v=v, v_old=v_old, l1=l1, l2=l2, pre=pre_a[:-1] + pre_c[:-1])
    loss = l_pi + vc * l_v - ec * entropy
    out["loss"] = loss
    out["stats"] = np.array([l_pi, l_v, entropy, (old - logp).sum() / M, (~inside).sum() / M, loss, len(j), M - len(j)])
    return out


def grad_list(ev):
    """[(name, array)] of every gradient of evaluate()'s result, in a fixed order"""
    out = []
    for net in ("actor", "critic"):
        for l, (dw, db) in enumerate(ev[net] or []):
            out.append((f"{net}.{l}.weight", dw))
            if db is not None:
                out.append((f"{net}.{l}.bias", db))
    return out + [("log_std", ev["log_std"])]


# ---------------------------------------------------------------------------- the cases the tests share
def _spec(v0):
    na = 18 if v0 else 20
    return na, 11 + 3 * na


# name: (v0, M, rows, actor (K or None = the observation's, widths without NA, activation), critic or None, value_clip, options)
CASES = {
    "tanh_relu_17": (False, 17, 66, (None, [24], "tanh"), (75, [24], "relu"), True, {}),
    "elu3_nobias_33": (False, 33, 99, (75, [40, 24], "elu"), (75, [24], "elu"), False, dict(no_bias=1)),
    "segments": (False, SEG_ROWS + 17, 660, (None, [24], "tanh"), (75, [24], "tanh"), True, {}),
    "wide_no_critic": (False, 33, 99, (30, [512, 512], "elu"), None, True, {}),
    "v0_single_row": (True, 1, 33, (None, [24], "tanh"), (69, [24], "relu"), True, {}),
    "v0_elu3_17": (True, 17, 66, (69, [40, 24], "elu"), (69, [24], "tanh"), True, {}),
    "all_ties": (False, 33, 99, (None, [24], "tanh"), (75, [24], "tanh"), True, dict(ties=True)),
}
SEEDS = dict({name: 0 for name in CASES}, tanh_relu_17=2)      # chosen so that the conditions hold with no row excluded


def make_case(name, seed=None):
    """The case `name` as float32 / int32 numpy arrays, the way a RolloutStorage holds them: networks, the stored rows, a
    shuffled index with repeats, returns = v + N(0, 1), and - so that no row of however many sits on a kink of the loss -
    logp_old = the recomputed logp - ln r with r uniform in [0.55, 0.78], [0.83, 1.17] or [1.22, 1.6] (a fifth, three fifths, a
    fifth of the rows), value = v - d with |d| uniform in [0, 0.18] (three fifths) or [0.22, 0.5].
    ties: logp_old = logp, and a critic whose last layer is the constant 0.5 = value, so that v = value = v_clip exactly in
    every precision.  The float64 evaluation of a case reads these float32 values, as the device does."""
    v0, M, rows, (ka, wa, aa), critic, value_clip, opt = CASES[name]
    na, nobs = _spec(v0)
    rng = np.random.default_rng([SEEDS[name] if seed is None else seed, sorted(CASES).index(name)])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    ka = nobs if ka is None else ka
    case = dict(name=name, v0=v0, na=na, M=M, rows=rows, clip=0.2, value_coef=0.7, entropy_coef=0.01, value_clip=value_clip, critic=None)
    layers = make_layers(rng, ka, wa + [na])
    if "no_bias" in opt:
        layers[opt["no_bias"]] = (layers[opt["no_bias"]][0], None)
    case["actor"] = (layers, aa)
    case["actor_input"] = f32(rng.normal(0, 1, (rows, ka)))
    case["log_std"] = f32(rng.uniform(-1.0, 0.0, na))
    mu = forward_all(case["actor_input"], layers, aa)[0][-1]
    sigma = np.exp(case["log_std"].astype(np.float64))
    case["action"] = f32(mu + sigma * rng.normal(0, 1, (rows, na)))
    case["advantage"] = f32(rng.normal(0.3, 1.5, rows))
    case["adv_stats"] = f32([case["advantage"].mean(), 1.0 / (case["advantage"].std(ddof=1) + 1e-8)])
    z = (case["action"].astype(np.float64) - mu) / sigma
    logp = -(0.5 * z * z + case["log_std"].astype(np.float64)).sum(1) - 0.5 * na * LN_2PI
    ties = bool(opt.get("ties"))
    pick = rng.random(rows)
    ratio = np.where(pick < 0.2, rng.uniform(0.55, 0.78, rows), np.where(pick < 0.8, rng.uniform(0.83, 1.17, rows), rng.uniform(1.22, 1.6, rows)))
    case["logp"] = f32(logp if ties else logp - np.log(ratio))
    case["critic_input"] = case["value"] = case["returns"] = None
    if critic is not None:
        kc, wc, ac = critic
        cl = make_layers(rng, kc, wc + [1])
        if ties:
            cl[-1] = (np.zeros_like(cl[-1][0]), np.full(1, 0.5, dtype=np.float32))
        case["critic"] = (cl, ac)
        case["critic_input"] = f32(rng.normal(0, 1, (rows, kc)))
        v = forward_all(case["critic_input"], cl, ac)[0][-1][:, 0]
        d = np.where(rng.random(rows) < 0.6, rng.uniform(0, 0.18, rows), rng.uniform(0.22, 0.5, rows)) * rng.choice([-1.0, 1.0], rows)
        case["value"] = f32(v if ties else v - d)
        case["returns"] = f32(v + rng.normal(0, 1, rows))
    # a shuffled index with repeats: the first entries twice when the storage allows, then rows at random
    idx = rng.permutation(rows)[:M] if M <= rows else rng.integers(0, rows, M)
    if M >= 4:
        idx[-2:] = idx[:2]
    case["index"] = np.ascontiguousarray(idx, dtype=np.int32)
    return case


def conditions(case, ev):
    """{name: smallest distance} of the float64 evaluation from the loss's kinks (the tests assert the thresholds), and the
    fraction of rows outside the clip range"""
    c = case["clip"]
    out = dict(ratio=float(np.minimum(np.abs(ev["r"] - (1 - c)), np.abs(ev["r"] - (1 + c))).min()),
               clipped=float(((ev["r"] < 1 - c) | (ev["r"] > 1 + c)).mean()))
    if ev["v"] is not None and case["value_clip"]:
        d = np.abs(ev["v"] - ev["v_old"])
        gap = np.abs(ev["l1"] - ev["l2"])[d > c]      # (inside the range v_clip is v by construction: tied but for its rounding)
        out["value"] = float(np.abs(d - c).min())
        out["l1_l2"] = float(gap[gap != 0].min()) if (gap != 0).any() else float("inf")
    relu = [p for (net, p) in _relu_pre(case, ev)]
    if relu:
        out["relu"] = float(min(np.abs(p).min() for p in relu))
    return out


def _relu_pre(case, ev):
    """the hidden pre-activations of the networks whose activation is ReLU"""
    pre, k, out = ev["pre"], 0, []
    for net in ("actor", "critic"):
        if case[net] is None:
            continue
        layers, act = case[net]
        for _ in range(len(layers) - 1):
            if act == "relu":
                out.append((net, pre[k]))
            k += 1
    return out
