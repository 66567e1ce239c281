"""Numpy float64 restatement of the policy optimiser (tsidb_policy_opt_step), written from its description in include/tsidb.h:
the gradient norm in the header's order of sums, the clip factor, the Gaussian KL of a minibatch in its order, rsl_rl's step
size rule in IEEE float32, torch.optim.Adam's step, and the skip.  No torch, no library.  Also the cases the tests share:
tests/test_policy_optimizer_reference.py holds the restatement to torch's float64 clip_grad_norm_ / Adam / kl_divergence and the
cases to their distance from the rule's kinks, tests/test_gpu_policy_optimizer.py runs them on the device.

A case is a learner case (policy_learner_reference.make_case: the networks, the storage, the index) plus case["opt"]: the
settings, STEPS lists of float32 gradients in the order of PolicyLearner.parameters(), the rollout's stored means, the
rollout's log_std, and per step the mu the KL reads from the learner's workspace.
"""
import numpy as np

import policy_learner_reference as RL

CHUNK, LANES = 1024, 256        # TSIDB_POL_OPT_CHUNK, TSIDB_POL_OPT_LANES
SEG_ROWS = RL.SEG_ROWS          # TSIDB_POL_LEARN_SEG_ROWS
STATS = ("grad_norm", "clip_coef", "kl", "lr", "step", "skipped", "kl_rows", "lr_direction")
STEPS = 5
F32 = np.float32


# ---------------------------------------------------------------------------- the sums
def halve(slots):
    """slot[t] += slot[t + s] for s = LANES / 2 .. 1 along axis -1 of [.., LANES]; the [..] slot 0"""
    s = np.asarray(slots, dtype=np.float64)
    h = LANES // 2
    while h >= 1:
        s = s[..., :h] + s[..., h:2 * h]
        h //= 2
    return s[..., 0]


def chunk_sums(g):
    """the float64 sums of squares of the chunks of one piece, each in the header's order"""
    flat = np.asarray(g, dtype=np.float64).reshape(-1)
    n = -(-len(flat) // CHUNK)
    x = np.zeros(n * CHUNK)
    x[:len(flat)] = flat
    x = (x * x).reshape(n, LANES, 4)
    return halve(((x[..., 0] + x[..., 1]) + x[..., 2]) + x[..., 3])


def in_order(values):
    total = 0.0
    for v in values:
        total = total + float(v)
    return total


def grad_norm(grads):
    """sqrt of the chunk sums of every piece, added in chunk order, piece after piece"""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sqrt(in_order(s for g in grads for s in chunk_sums(g))))


def clip_coef(norm, max_norm):
    """float64; max_norm = 0: no clipping; a NaN stays a NaN"""
    if max_norm <= 0:
        return 1.0
    with np.errstate(invalid="ignore"):
        x = max_norm / (norm + 1e-6)
    return 1.0 if x > 1.0 else float(x)


def kl_rows(mu, mu_old, log_std, log_std_old):
    """kl_m of each row, the actuators added in rising order"""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    mu, mu_old, s, so = f(mu), f(mu_old), f(log_std), f(log_std_old)
    out = np.zeros(len(mu))
    e_old, den = np.exp(2.0 * so), 2.0 * np.exp(2.0 * s)
    for a in range(mu.shape[1]):
        d = mu_old[:, a] - mu[:, a]
        out = out + (((s[a] - so[a]) + (e_old[a] + d * d) / den[a]) - 0.5)
    return out


def kl_of(mu, mean, index, rows, log_std, log_std_old):
    """(kl, rows used): the mean over M = len(index) of kl_m, the segments' slots in the header's order; an index outside
    [0, rows) contributes nothing"""
    idx = np.asarray(index).astype(np.int64)
    M = len(idx)
    ok = (idx >= 0) & (idx < rows)
    per = np.zeros(M)
    if ok.any():
        per[ok] = kl_rows(np.asarray(mu)[:M][ok], np.asarray(mean).reshape(rows, -1)[idx[ok]], log_std, log_std_old)
    nseg = -(-M // SEG_ROWS)
    x = np.zeros(nseg * SEG_ROWS)
    x[:M] = per
    x = x.reshape(nseg, 2, LANES)
    return in_order(halve(x[:, 0] + x[:, 1])) / M, int(ok.sum())


def lr_rule(lr, kl, desired_kl, lr_min, lr_max):
    """rsl_rl's adaptive rule in IEEE float32: (lr, direction)"""
    lr0 = lr = F32(lr)
    if kl > 2.0 * desired_kl:
        lr = max(F32(lr_min), F32(lr0 / F32(1.5)))
    elif 0.0 < kl < desired_kl / 2.0:
        lr = min(F32(lr_max), F32(lr0 * F32(1.5)))
    return F32(lr), int(lr > lr0) - int(lr < lr0)


# ---------------------------------------------------------------------------- one step
def new_state(params, lr):
    """float64 copies of the parameters, zero moments, the float32 lr, step 0"""
    p = [np.asarray(x, dtype=np.float64).copy() for x in params]
    return dict(params=p, exp_avg=[np.zeros_like(x) for x in p], exp_avg_sq=[np.zeros_like(x) for x in p], lr=F32(lr), step=0)


def step(state, grads, cfg, kl_in=None, cast_coef=True):
    """(state after the call, stats [8] float64).  cfg: dict(b1, b2, eps, max_norm, desired_kl (None / 0 = off), lr_min, lr_max,
    skip_nonfinite).  kl_in: dict(mu, mean, index, rows, log_std_old) with the schedule; log_std is the state's last parameter
    as float32, as the device reads it.  cast_coef False: coef stays float64 (the comparison with torch's float64 pipeline)."""
    b1, b2, eps = cfg["b1"], cfg["b2"], cfg["eps"]
    sched = bool(cfg.get("desired_kl"))
    norm = grad_norm(grads)
    coef = clip_coef(norm, cfg["max_norm"])
    kl, used = 0.0, 0
    if sched:
        with np.errstate(over="ignore", invalid="ignore"):
            kl, used = kl_of(kl_in["mu"], kl_in["mean"], kl_in["index"], kl_in["rows"], state["params"][-1].astype(np.float32), kl_in["log_std_old"])
    skip = bool(cfg["skip_nonfinite"]) and (not np.isfinite(norm) or (sched and not np.isfinite(kl)))
    if skip:
        return state, np.array([norm, coef, kl, state["lr"], state["step"], 1.0, used, 0.0])
    lr, direction = lr_rule(state["lr"], kl, cfg["desired_kl"], cfg["lr_min"], cfg["lr_max"]) if sched else (state["lr"], 0)
    t = state["step"] + 1
    c = float(F32(coef)) if cast_coef else coef
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    out = dict(params=[], exp_avg=[], exp_avg_sq=[], lr=lr, step=t)
    with np.errstate(over="ignore", invalid="ignore"):
        for p, m, v, grad in zip(state["params"], state["exp_avg"], state["exp_avg_sq"], grads):
            g = c * np.asarray(grad, dtype=np.float64).reshape(p.shape)
            m = m + (g - m) * (1.0 - b1)
            v = b2 * v + (1.0 - b2) * g * g
            out["params"].append(p - (float(lr) / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps)))
            out["exp_avg"].append(m)
            out["exp_avg_sq"].append(v)
    return out, np.array([norm, coef, kl, lr, t, 0.0, used, direction], dtype=np.float64)


def run(case, steps=STEPS, cast_coef=True):
    """the case's steps from its initial parameters: [(state, stats)] after each"""
    o = case["opt"]
    state = new_state([a for _, a in param_list(case)], o["lr"])
    out = []
    for k in range(steps):
        state, stats = step(state, o["grads"][k], o["cfg"], kl_input(case, k), cast_coef)
        out.append((state, stats))
    return out


def kl_input(case, k):
    o = case["opt"]
    if not o["cfg"]["desired_kl"]:
        return None
    return dict(mu=o["mu"][k], mean=o["mean"], index=case["index"], rows=case["rows"], log_std_old=o["log_std_old"])


# ---------------------------------------------------------------------------- the cases the tests share
def param_list(case):
    """[(name, float32 array)] in the order of PolicyLearner.parameters()"""
    out = []
    for net in ("actor", "critic"):
        if case[net] is None:
            continue
        for l, (w, b) in enumerate(case[net][0]):
            out.append((f"{net}.{l}.weight", w))
            if b is not None:
                out.append((f"{net}.{l}.bias", b))
    return out + [("log_std", case["log_std"])]


# name: (the learner's case, bad indices appended, desired_kl or None, max_norm)
CASES = {
    "tanh_relu_17": ("tanh_relu_17", 0, 0.05, 1.0),
    "wide_no_critic": ("wide_no_critic", 0, 0.05, 1.0),
    "segments": ("segments", 0, 0.05, 1.0),
    "segments_bad": ("segments", 2, 0.05, 1.0),
    "v0_single_row": ("v0_single_row", 0, 0.05, 1.0),
    "elu3_nobias_33": ("elu3_nobias_33", 0, 0.05, 1.0),
    "no_schedule_no_clip": ("tanh_relu_17", 0, None, 0.0),
}
LR, LR_MIN, LR_MAX = 1e-2, 1e-2, 2e-2
# per step: the gradient norm over max_norm (clipping inactive below 1, active above), the KL over desired_kl (below 1/2: lr up;
# above 2: lr down), and what lr does from LR inside [LR_MIN, LR_MAX]: up, held by lr_max, unchanged, down, held by lr_min
NORMS = (0.5, 3.0, 0.8, 5.0, 2.0)
KLS = (0.25, 0.25, 1.0, 4.0, 4.0)
LR_MOVES = ("up", "pinned at lr_max", "unchanged", "down", "pinned at lr_min")


def make_case(name):
    """The learner's case with case["opt"].  The gradients of step k are one random direction per parameter set, scaled so
    that their norm is NORMS[k] (times max_norm, or 1); the stored means are random, and the mu of step k is the mean minus a
    random shift scaled so that the KL is KLS[k] * desired_kl with the log_std the float64 restatement holds at that step -
    log_std moves with every step, and its own share of the KL is left to it."""
    base, n_bad, desired_kl, max_norm = CASES[name]
    case = RL.make_case(base)
    rng = np.random.default_rng([7, sorted(CASES).index(name)])
    case["name"] = name
    rows, na = case["rows"], case["na"]
    if n_bad:
        case["index"] = np.ascontiguousarray(np.concatenate([case["index"], [-1, rows][:n_bad]]), dtype=np.int32)
        case["M"] = len(case["index"])
    idx = case["index"].astype(np.int64)
    ok = (idx >= 0) & (idx < rows)
    cfg = dict(b1=0.9, b2=0.999, eps=1e-8, max_norm=max_norm, desired_kl=desired_kl, lr_min=LR_MIN, lr_max=LR_MAX, skip_nonfinite=True)
    params = param_list(case)
    direction = [rng.normal(0, 1, a.shape) for _, a in params]
    unit = np.sqrt(sum(float((d * d).sum()) for d in direction))
    grads = [[np.ascontiguousarray(d * (NORMS[k] * (max_norm or 1.0) / unit), dtype=np.float32) for d in direction] for k in range(STEPS)]
    mean = np.full((rows, na), np.nan, dtype=np.float32)          # (rows outside the index are never read)
    stored = np.unique(idx[ok])
    mean[stored] = rng.normal(0, 0.5, (len(stored), na)).astype(np.float32)
    opt = dict(cfg=cfg, lr=LR, grads=grads, mean=mean, log_std_old=case["log_std"].copy(), mu=[None] * STEPS)
    case["opt"] = opt
    if desired_kl:
        shift = rng.normal(0, 1, (case["M"], na))
        state = new_state([a for _, a in params], LR)
        rows_mean = np.zeros((case["M"], na))
        rows_mean[ok] = mean[idx[ok]]
        for k in range(STEPS):
            ls = state["params"][-1].astype(np.float32)
            # kl(delta) = kl(0) + delta^2 * mean_m sum_a shift^2 / (2 exp(2 log_std_a)), over the usable rows
            at0 = kl_of(rows_mean, mean, idx, rows, ls, opt["log_std_old"])[0]
            gain = float((shift[ok] ** 2 / (2.0 * np.exp(2.0 * ls.astype(np.float64)))).sum() / case["M"])
            target = KLS[k] * desired_kl
            assert target > at0 >= 0.0, (name, k, target, at0)
            opt["mu"][k] = np.ascontiguousarray(rows_mean - np.sqrt((target - at0) / gain) * shift, dtype=np.float32)
            state, _ = step(state, grads[k], cfg, kl_input(case, k))
    return case
