"""Numpy float64 restatement of the learner's mirror symmetry (tsidb_policy_learn_sym), written from its description in
include/tsidb.h and built on tests/policy_learner_reference.py: the augmented surrogate and value loss are the plain learner's on
a storage of twice the rows whose second half holds the mirrored rows, and the mirror term L_sym = 1 / (M NA) sum_m
|mu(S_o x_m) - S_a mu(x_m)|^2 with its constant target is added by the chain rule.  No torch, no library.  Also the cases the
tests share: tests/test_policy_symmetry_reference.py checks the restatement against torch's float64 autograd and the cases'
distance from the loss's kinks, tests/test_gpu_policy_symmetry.py runs them on the device.
"""
import importlib.util
from pathlib import Path

import numpy as np

import policy_learner_reference as R

SYM_STATS = ("mirror_loss", "mirrored_rows")

# the actuator tables of the two robots (PolicySymmetry derives them from the model blobs; tests/test_policy_symmetry_host.py)
ACTUATORS = {
    False: ([6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5, 15, 16, 17, 12, 13, 14, 18, 19], [-1.0] * 19 + [1.0]),
    True: ([3, 4, 5, 0, 1, 2, 6, 7, 13, 14, 15, 16, 17, 8, 9, 10, 11, 12], [1.0] * 6 + [-1.0, 1.0] + [-1.0] * 10),
}


def mirror(x, table):
    """sign[c] * x[..., perm[c]]; a perm entry outside the row makes the column 0"""
    perm, sign = np.asarray(table[0]).astype(np.int64), np.asarray(table[1])
    x = np.asarray(x)
    ok = (perm >= 0) & (perm < x.shape[-1])
    return np.where(ok, x[..., np.where(ok, perm, 0)] * sign.astype(x.dtype), np.zeros((), dtype=x.dtype))


def random_involution(rng, k):
    """a signed involution of k columns: about a third fixed (half of them flipped), the rest swapped in pairs of one sign"""
    perm, sign = np.arange(k), np.ones(k)
    cols = rng.permutation(k)
    fixed = k // 3 + ((k - k // 3) % 2)
    for c in cols[:fixed]:
        sign[c] = rng.choice([-1.0, 1.0])
    rest = cols[fixed:]
    for a, b in zip(rest[0::2], rest[1::2]):
        perm[a], perm[b] = b, a
        sign[a] = sign[b] = rng.choice([-1.0, 1.0])
    return perm.astype(np.int32), sign.astype(np.float32)


def doubled(case):
    """the plain learner's case on a storage of twice the rows, the second half the mirror image of the first:
    index2 = (index, index + rows), a bad index bad in both halves"""
    rows = case["rows"]
    idx = np.asarray(case["index"]).astype(np.int64)
    ok = (idx >= 0) & (idx < rows)
    big = dict(case, rows=2 * rows, M=2 * len(idx), index=np.concatenate([np.where(ok, idx, -1), np.where(ok, idx + rows, -1)]).astype(np.int32))
    for k, table in (("actor_input", "actor_table"), ("critic_input", "critic_table"), ("action", "action_table")):
        if case[k] is not None:
            big[k] = np.concatenate([case[k], mirror(case[k], case[table])])
    for k in ("logp", "value", "advantage", "returns"):
        if case[k] is not None:
            big[k] = np.concatenate([case[k], case[k]])
    return big


def evaluate(case):
    """R.evaluate's dict for the case's augment and mirror_coef, with sym_stats [2], mirror_loss, and ev["virtual"]: the
    evaluation whose per-row values (r, v, pre) the kink conditions look at - the doubled case's with augment"""
    j, M = R.rows_of(case)
    na, coef = case["na"], case["mirror_coef"]
    ev = R.evaluate(doubled(case) if case["augment"] else case)
    out = dict(ev, virtual=ev, actor=[(dw.copy(), None if db is None else db.copy()) for dw, db in ev["actor"]])
    stats = ev["stats"].copy()
    if case["augment"]:
        stats[7] = M - len(j)                      # (each bad index once)
        out["mu"] = ev["mu"][:len(j)]
    layers, act = case["actor"]
    x = np.asarray(case["actor_input"], dtype=np.float64)[j]
    xm = mirror(x, case["actor_table"])
    mu = R.forward_all(x, layers, act)[0][-1]
    H, pre_m = R.forward_all(xm, layers, act)
    d = H[-1] - mirror(mu, case["action_table"])
    l_sym = (d * d).sum() / (M * na)
    if coef > 0:
        for l, (dw, db) in enumerate(R.backward_net(xm, layers, act, H, coef * 2.0 * d / (M * na))):
            out["actor"][l] = (out["actor"][l][0] + dw, None if db is None else out["actor"][l][1] + db)
        stats[5] = stats[5] + coef * l_sym
    out.update(stats=stats, loss=stats[5], mirror_loss=l_sym, sym_stats=np.array([l_sym, len(j)]), mirror_pre=pre_m[:-1], mirror_d=d)
    return out


grad_list = R.grad_list


# ---------------------------------------------------------------------------- the cases the tests share
def _private_learner_reference(cases, seeds):
    """a second instance of policy_learner_reference whose CASES are these: its make_case draws a case as the learner's tests do"""
    spec = importlib.util.spec_from_file_location("_policy_learner_reference_for_symmetry", Path(R.__file__))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.CASES, mod.SEEDS = cases, seeds
    return mod


# name: ((v0, M, rows, actor, critic, value_clip, options) as policy_learner_reference.CASES, augment, mirror_coef, bad indices)
CASES = {
    "aug_17": ((False, 17, 66, (None, [24], "tanh"), (75, [24], "relu"), True, {}), True, 0.0, False),
    "aug_mirror_33_nobias": ((False, 33, 99, (75, [40, 24], "elu"), (75, [24], "elu"), False, dict(no_bias=1)), True, 0.5, False),
    "mirror_17": ((False, 17, 66, (None, [24], "tanh"), (75, [24], "relu"), True, {}), False, 0.5, False),
    "off_33": ((False, 33, 99, (None, [24], "elu"), (75, [24], "tanh"), True, {}), False, 0.0, False),
    "aug_mirror_272": ((False, 272, 297, (None, [24], "tanh"), (75, [24], "tanh"), True, {}), True, 0.5, False),
    "wide_no_critic": ((False, 33, 99, (30, [512, 512], "elu"), None, True, {}), True, 0.5, False),
    "v0_single_row": ((True, 1, 33, (None, [24], "tanh"), (69, [24], "relu"), True, {}), True, 0.5, False),
    "v0_mirror_17": ((True, 17, 66, (69, [40, 24], "elu"), (69, [24], "tanh"), True, {}), False, 0.5, False),
    "bad_indices_33": ((False, 33, 99, (None, [24], "tanh"), (75, [24], "relu"), True, {}), True, 0.5, True),
}
SEEDS = {name: 0 for name in CASES}       # chosen so that the conditions hold with no row excluded, the mirrored rows included
_P = _private_learner_reference({k: v[0] for k, v in CASES.items()}, SEEDS)


def make_case(name, seed=None, **over):
    """policy_learner_reference.make_case's case with the three tables (the robot's actuator table for the action, random signed
    involutions for the two input rows), augment and mirror_coef; bad indices: a -1 and a `rows` inside the index.  over:
    augment= / mirror_coef= of the same draw."""
    _, augment, coef, bad = CASES[name]
    case = _P.make_case(name, seed)
    rng = np.random.default_rng([SEEDS[name] if seed is None else seed, sorted(CASES).index(name), 7])
    perm, sign = ACTUATORS[case["v0"]]
    case["action_table"] = (np.asarray(perm, dtype=np.int32), np.asarray(sign, dtype=np.float32))
    case["actor_table"] = random_involution(rng, case["actor_input"].shape[1])
    case["critic_table"] = random_involution(rng, case["critic_input"].shape[1]) if case["critic"] is not None else None
    if bad:
        idx = case["index"]
        case["index"] = np.concatenate([idx[:5], [-1], idx[5:-2], [case["rows"]]]).astype(np.int32)
    case.update(augment=augment, mirror_coef=coef)
    case.update(over)
    return case


def conditions(case, ev):
    """policy_learner_reference.conditions over the virtual rows - with augment the mirrored rows count - and, for a ReLU actor
    with the mirror term, the mirrored rows' pre-activations"""
    virt = doubled(case) if case["augment"] else case
    out = R.conditions(virt, ev["virtual"])
    if case["actor"][1] == "relu" and ev["mirror_pre"]:
        out["relu"] = min(out.get("relu", np.inf), float(min(np.abs(p).min() for p in ev["mirror_pre"])))
    return out
