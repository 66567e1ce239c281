"""Numpy float64 restatement of the imitation slice, written from include/tsidb.h: tsidb_policy_learn_imit's loss and gradient (on
top of tests/policy_learner_reference.py, whose critic part it takes as it is) and tsidb_policy_teacher_mix's labels, weights,
executed flags and executed actions (the draw: tests/policy_dr_reference.py, stream 23).  No torch, no library.  Also the cases
the tests share: tests/test_policy_imitation_reference.py holds the restatement to torch's float64 autograd,
tests/test_gpu_policy_imitation.py runs the cases on the device.
"""
import numpy as np

import policy_dr_reference as DR
import policy_learner_reference as R

STREAM = 23             # the teacher / student draw of an episode
LOSSES = ("mse", "huber")
IMIT_STATS = ("imitation_loss", "weight_sum", "weighted_rows", "skipped_rows")


# ---------------------------------------------------------------------------- tsidb_policy_teacher_mix
def mix(teacher_action, action, ep_len, episode, beta, seed, env_offset=0):
    """(label float32 [N, NA], weight float32 [N], executed int32 [N], action as the env executes it) of one launch; teacher_action
    and action in the path's dtype, beta a float32 value or None (= 0)"""
    teacher_action, action = np.asarray(teacher_action), np.asarray(action)
    ep_len, episode = np.asarray(ep_len).astype(np.int64), np.asarray(episode).astype(np.int64)
    n = len(ep_len)
    u = DR.draw(seed, STREAM, 0, np.uint64(env_offset) + np.arange(n, dtype=np.uint64), DR.counter_hi_lo(episode, np.zeros(n, dtype=np.int64)))
    live = ep_len > 0
    executed = live & (u < (0.0 if beta is None else float(np.float32(beta))))
    out = action.copy()
    out[executed] = teacher_action[executed]
    return teacher_action.astype(np.float32), live.astype(np.float32), executed.astype(np.int32), out


# ---------------------------------------------------------------------------- tsidb_policy_learn_imit
def evaluate(case):
    """policy_learner_reference.evaluate's dict for the extended loss: loss, stats [8] (stats[5] the full loss), imit_stats [4],
    actor / critic / log_std gradients.  case: a learner case plus target [rows, NA] or None, weight [rows] or None (= 1), skip
    [rows] or None, imitation_coef, surrogate_coef, imit_loss"""
    base = R.evaluate(case)                      # the critic's part, and the actor's forward pass, as they are
    f = lambda k: np.asarray(case[k], dtype=np.float64)
    j, M = R.rows_of(case)
    c, vc, ec, na = case["clip"], case["value_coef"], case["entropy_coef"], case["na"]
    ic, sc = case["imitation_coef"], case["surrogate_coef"]
    ls = f("log_std")
    sigma = np.exp(ls)
    layers, act = case["actor"]
    xa = f("actor_input")[j]
    H, _ = R.forward_all(xa, layers, act)
    mu = H[-1]
    z = (f("action")[j] - mu) / sigma
    logp, old, r = base["logp"], f("logp")[j], base["r"]
    adv = f("advantage")[j]
    if case["adv_stats"] is not None:
        st = f("adv_stats")
        adv = (adv - st[0]) * st[1]
    skip = np.zeros(len(j), dtype=bool) if case["skip"] is None else np.asarray(case["skip"])[j] != 0
    t1, t2 = -adv * r, -adv * np.clip(r, 1 - c, 1 + c)
    inside = (r >= 1 - c) & (r <= 1 + c)
    l_pi = np.where(skip, 0.0, np.maximum(t1, t2)).sum() / M
    dlogp = np.where(skip, 0.0, sc * r * np.where(inside | (t1 > t2), -adv / M, 0.0))
    g_mu = dlogp[:, None] * z / sigma
    # the label's term: a row whose weight is exactly 0 is left out by a select, its label is not looked at
    w = np.ones(len(j)) if case["weight"] is None else f("weight")[j]
    l_im = 0.0
    if case["target"] is not None:
        use = w != 0
        d = np.where(use[:, None], mu - np.where(use[:, None], f("target")[j], 0.0), 0.0)
        if case["imit_loss"] == "mse":
            rows, dd = (d * d).sum(1) / na, 2 * d
        else:
            rows, dd = np.where(np.abs(d) <= 1, d * d / 2, np.abs(d) - 0.5).sum(1) / na, np.clip(d, -1, 1)
        l_im = np.where(use, w * rows, 0.0).sum() / M
        if ic > 0:
            g_mu = g_mu + np.where(use[:, None], (ic * w / (M * na))[:, None] * dd, 0.0)
    elif ic > 0:
        raise ValueError("imitation_coef > 0 needs target")
    entropy, l_v = base["stats"][2], base["stats"][1]
    loss = sc * l_pi + vc * l_v - ec * entropy + (ic * l_im if ic > 0 else 0.0)
    out = dict(base, actor=R.backward_net(xa, layers, act, H, g_mu), log_std=(dlogp[:, None] * (z * z - 1)).sum(0) - ec, loss=loss, mu=mu)
    out["stats"] = np.array([l_pi, l_v, entropy, np.where(skip, 0.0, old - logp).sum() / M, (~inside & ~skip).sum() / M, loss, len(j), M - len(j)])
    out["imit_stats"] = np.array([l_im, w.sum(), (w > 0).sum(), skip.sum()], dtype=np.float64)
    return out


grad_list = R.grad_list

PPO_BC = dict(imitation_coef=0.5, surrogate_coef=1.0)
DISTILL = dict(imitation_coef=1.0, surrogate_coef=0.0, value_coef=0.0, entropy_coef=0.0)
# name: (the learner's case, loss, coefficients, options) - both robots' NA; 1, 17, 33 and 512 + 17 rows; both losses; weights 0, 1
# and fractional with NaN labels behind the zeros; executed rows; bad indices; no critic; pure distillation; NULL weight and skip
CASES = {
    "mse_17": ("tanh_relu_17", "mse", PPO_BC, {}),
    "huber_33_nobias": ("elu3_nobias_33", "huber", PPO_BC, {}),
    "huber_segments_bad": ("segments", "huber", dict(imitation_coef=2.0, surrogate_coef=0.5), dict(bad=True)),
    "mse_no_critic_distill": ("wide_no_critic", "mse", DISTILL, {}),
    "v0_huber_single_row": ("v0_single_row", "huber", PPO_BC, {}),
    "v0_mse_17_distill": ("v0_elu3_17", "mse", DISTILL, {}),
    "huber_17_plain": ("tanh_relu_17", "huber", dict(imitation_coef=0.25, surrogate_coef=1.0), dict(plain=True)),
}


def make_case(name):
    """The imitation case `name`: policy_learner_reference.make_case's arrays and, float32 / int32 as a teacher storage holds them,
    target = mu + delta with |delta| uniform in [0.05, 0.8] (three fifths of the elements) or [1.2, 2.5] - both branches of the
    Huber loss and of its clamp, none within 0.05 of |d| = 1 or 0 -, weight 0 (a quarter of the rows, their labels NaN), 1 (half) or
    uniform in [0.1, 0.9], skip 1 for three rows in ten.  The rows index names keep at least one weight of each kind where there
    are three rows or more; a single row has weight 1.  plain: weight and skip None.  bad: index gains a -1 and a rows + 5."""
    base, loss, coefs, opt = CASES[name]
    case = dict(R.make_case(base))
    case.update(name=name, imit_loss=loss, **coefs)
    rows, na = case["rows"], case["na"]
    rng = np.random.default_rng([7, sorted(CASES).index(name)])
    mu = R.forward_all(case["actor_input"], *case["actor"])[0][-1]
    mag = np.where(rng.random((rows, na)) < 0.6, rng.uniform(0.05, 0.8, (rows, na)), rng.uniform(1.2, 2.5, (rows, na)))
    target = (mu + mag * rng.choice([-1.0, 1.0], (rows, na))).astype(np.float32)
    pick = rng.random(rows)
    weight = np.where(pick < 0.25, 0.0, np.where(pick < 0.75, 1.0, rng.uniform(0.1, 0.9, rows))).astype(np.float32)
    used = np.unique(case["index"])
    if len(used) >= 3:
        weight[used[0]], weight[used[1]], weight[used[2]] = 0.0, 1.0, 0.5
    else:
        weight[used] = 1.0
    full = target.copy()
    target[weight == 0] = np.nan
    skip = (rng.random(rows) < 0.3).astype(np.int32)
    if len(used) >= 3:
        skip[used[1]], skip[used[2]] = 1, 0
    else:
        skip[used] = 0                           # (a single row keeps its surrogate)
    case.update(target=target, weight=None if opt.get("plain") else weight, skip=None if opt.get("plain") else skip)
    if opt.get("plain"):
        case["target"] = full                    # (every row is used: every label is one)
    if opt.get("bad"):
        idx = case["index"]
        case["index"] = np.concatenate([idx[:5], [-1], idx[5:], [rows + 5]]).astype(np.int32)
        case["M"] = len(case["index"])
    return case


def margins(case, ev):
    """the smallest distance of |d| = |mu - target| from 1 and from 0 over the rows the term uses, and the fractions of the used
    elements on the quadratic and on the linear branch"""
    j, _ = R.rows_of(case)
    w = np.ones(len(j)) if case["weight"] is None else np.asarray(case["weight"], dtype=np.float64)[j]
    d = np.abs(ev["mu"] - np.asarray(case["target"], dtype=np.float64)[j])[w != 0]
    return dict(kink=float(np.abs(d - 1).min()), zero=float(d.min()), quadratic=float((d < 1).mean()), linear=float((d > 1).mean()))
