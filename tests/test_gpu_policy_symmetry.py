"""The learner's mirror symmetry on the device (tsidb_policy_learn_sym, PolicyLearner(symmetry=...)) against the float64
restatement tests/policy_symmetry_reference.py.  The yardstick is the learner's own: torch's CPU float32 autograd of the same
case, E = e32(case) - every gradient, stats 0 .. 5 and L_sym stay within 8 max(E, 2^-22) max|ref| - and for the same reason: the
device sums the batch as one k-ordered chain per segment where torch's CPU kernels sum in blocks, and expf differs by an ulp or
two.  Then the bits: augmentation against the plain learner on a hand-mirrored storage of twice the rows, and the term switched off
against the plain learner.  Synthetic storages as in tests/test_gpu_policy_learner.py: 33 envs, every tensor a view inside a
NaN-filled allocation."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_symmetry_reference as S  # noqa: E402
from policy_testlib import capture, host, make_env  # noqa: E402
from test_gpu_policy_learner import build, grads_of, run  # noqa: E402
from test_policy_symmetry_reference import e32  # noqa: E402

pytestmark = pytest.mark.gpu


def build_sym(case, **over):
    """(PolicyActor, RolloutStorage, PolicyLearner with the case's symmetry, index, PolicySymmetry) on the device; the input
    blocks are raw tensors, so the case's tables go in as blocks=, the action's is derived from the model and must be the case's"""
    from tsid_control_amd import PolicyLearner, PolicySymmetry
    pa, st, plain, index = build(case)
    blocks = {("actor", 0): case["actor_table"]}
    if case["critic"] is not None:
        blocks["critic", 0] = case["critic_table"]
    sy = PolicySymmetry(pa.env, pa, blocks=blocks)
    assert np.array_equal(host(sy.action_perm), case["action_table"][0]) and np.array_equal(host(sy.action_sign), case["action_table"][1])
    kw = dict(symmetry_augment=case["augment"], mirror_coef=case["mirror_coef"])
    kw.update(over)
    pl = PolicyLearner(pa, clip=case["clip"], value_coef=case["value_coef"], entropy_coef=case["entropy_coef"], value_clip=case["value_clip"],
                       normalize_advantage=case["adv_stats"] is not None, symmetry=sy, **kw)
    pl.adv_stats.copy_(plain.adv_stats)
    return pa, st, pl, index, sy


def gate_ratio(case, got, stats, sym_stats, ev=None, E=None):
    """the largest error / gate over the parameter tensors, stats 0 .. 5 and L_sym, each printed"""
    ev = S.evaluate(case) if ev is None else ev
    E = max(e32(case) if E is None else E, 2.0 ** -22)
    worst = 0.0
    want = dict(S.grad_list(ev))
    assert sorted(want) == sorted(got)
    for k, g64 in want.items():
        assert got[k].shape == g64.shape and np.isfinite(got[k]).all(), k
        ratio = float(np.abs(got[k] - g64).max() / (8 * E * np.abs(g64).max()))
        print(f"{case['name']} {k}: error / gate {ratio:.3f}")
        worst = max(worst, ratio)
    for i in range(6):
        ratio = float(abs(stats[i] - ev["stats"][i]) / (8 * E * max(1.0, abs(ev["stats"][i]))))
        print(f"{case['name']} stats[{i}] {S.R.STATS[i]}: error / gate {ratio:.3f}")
        worst = max(worst, ratio)
    ratio = float(abs(sym_stats[0] - ev["mirror_loss"]) / (8 * E * max(1.0, abs(ev["mirror_loss"]))))
    print(f"{case['name']} sym_stats[0] mirror_loss: error / gate {ratio:.3f}")
    worst = max(worst, ratio)
    print(f"{case['name']}: augment {case['augment']}, mirror_coef {case['mirror_coef']}, E = {E:.2e}, largest error / gate {worst:.3f}")
    return worst, ev


VARIANTS = [(name, {}) for name in sorted(S.CASES)] + [("aug_17", dict(augment=a, mirror_coef=c)) for a, c in ((False, 0.0), (False, 0.5), (True, 0.5))]


# ---------------------------------------------------------------------------- (1) the gate
@pytest.mark.parametrize("name,over", VARIANTS, ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()) or "case")
def test_gradients_stats_and_mirror_loss_match_the_float64_reference(name, over):
    """every case of policy_symmetry_reference.CASES - both robots; M = 1, 17 (a partial tile), 33 and 272 (2 M > 512: two
    segments); tanh, ELU and ReLU; no critic with the 512-wide networks; a layer without bias; bad indices, skipped and counted
    once - and augment on / off crossed with mirror_coef 0 / 0.5 on one draw.  stats 6, 7 and sym_stats[1] exact.
    Measured (MI355X), E and the largest error / gate: aug_17 3.49e-7, 0.127; aug_mirror_272 9.83e-7, 0.178; aug_mirror_33_nobias
    6.88e-7, 0.296; bad_indices_33 9.58e-7, 0.187; mirror_17 1.29e-6, 0.096; off_33 1.40e-6, 0.139; v0_mirror_17 9.86e-7, 0.118;
    v0_single_row 2.66e-7, 0.164; wide_no_critic 5.17e-7, 0.546; aug_17 with (off, 0) 0.143, (off, 0.5) 0.130, (on, 0.5) 0.153."""
    case = S.make_case(name, **over)
    pa, st, pl, index, sy = build_sym(case)
    got, stats = run(pl, st, index)
    sym_stats = host(pl.sym_stats)
    worst, ev = gate_ratio(case, got, stats, sym_stats)
    assert worst <= 1.0
    assert list(stats[6:]) == list(ev["stats"][6:]) and sym_stats[1] == ev["sym_stats"][1]
    if name == "bad_indices_33":
        assert list(stats[6:]) == [62, 2] and sym_stats[1] == 31
    mu, v = pl.outputs(case["M"])
    j, M = S.R.rows_of(case)
    if len(j) == M:
        assert np.abs(host(mu) - ev["mu"]).max() <= 1e-4 * max(1.0, np.abs(ev["mu"]).max())
    assert (v is None) == (case["critic"] is None)


# ---------------------------------------------------------------------------- (2) the bit twin of the augmentation
@pytest.mark.parametrize("name,M", [("aug_17", 16), ("aug_mirror_272", 272)])
def test_augmentation_is_the_plain_learner_on_a_hand_mirrored_storage_bit_for_bit(name, M):
    """augment, mirror_coef = 0, M a multiple of 16 (one tile; two segments): a storage of twice the rows whose second half holds
    mirror_obs / mirror_action of the first and copies of logp, value, advantage and returns, index2 = (index, index + rows), the
    same explicit adv_stats - every .grad and stats 0 .. 6 are torch.equal"""
    case = S.make_case(name, augment=True, mirror_coef=0.0)
    case["index"] = np.ascontiguousarray(case["index"][:M])
    case["M"] = M
    pa, st, pl, index, sy = build_sym(case)
    big = S.doubled(case)
    pa2, st2, pl2, index2 = build(big)
    rows = case["rows"]
    assert torch.equal(index2, torch.cat([index, index + rows]))
    # the hand-built half is what mirror_obs / mirror_action give
    flat = lambda t, r: t.reshape(r, -1)
    assert torch.equal(flat(st2.actor_input, 2 * rows)[rows:], sy.mirror_obs(flat(st.actor_input, rows)))
    assert torch.equal(flat(st2.critic_input, 2 * rows)[rows:], sy.mirror_obs(flat(st.critic_input, rows), "critic"))
    assert torch.equal(flat(st2.action, 2 * rows)[rows:], sy.mirror_action(flat(st.action, rows)))
    assert not torch.equal(flat(st2.actor_input, 2 * rows)[rows:], flat(st.actor_input, rows))
    got, stats = run(pl, st, index)
    want, wstats = run(pl2, st2, index2)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(stats[:7], wstats[:7]) and stats[6] == 2 * M
    assert np.abs(want["actor.0.weight"]).max() > 0 and np.abs(want["critic.0.weight"]).max() > 0
    # and the mirrored half matters: the plain learner on the M rows alone gives other gradients
    pa1, st1, pl1, index1 = build(case)
    alone, _ = run(pl1, st1, index1)
    assert not np.array_equal(alone["actor.0.weight"] * 0.5, got["actor.0.weight"])


# ---------------------------------------------------------------------------- (3) the bit twin with the term off
def test_without_augmentation_the_mirrored_rows_add_exact_zeros():
    """augment off, mirror_coef = 0: every .grad is the plain learner's bit for bit and L_sym is still formed; mirror_coef = 0.5:
    the critic's .grad still is, the actor's moves.  On the two-segment case and on a partial tile."""
    for name in ("aug_mirror_272", "aug_17"):
        case = S.make_case(name, augment=False, mirror_coef=0.0)
        pa0, st0, pl0, index0 = build(case)
        want, wstats = run(pl0, st0, index0)
        pa, st, pl, index, sy = build_sym(case)
        got, stats = run(pl, st, index)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(stats, wstats)
        ev = S.evaluate(case)
        E = max(e32(case), 2.0 ** -22)
        sym_stats = host(pl.sym_stats)
        assert abs(sym_stats[0] - ev["mirror_loss"]) <= 8 * E * max(1.0, ev["mirror_loss"]) and sym_stats[0] > 1e-3 and sym_stats[1] == case["M"]
        half = S.make_case(name, augment=False, mirror_coef=0.5)
        pa, st, pl, index, sy = build_sym(half)
        got, stats = run(pl, st, index)
        for k in want:
            assert np.array_equal(got[k], want[k]) == (k.startswith("critic") or k == "log_std"), k
        assert np.array_equal(stats[:5], wstats[:5]) and stats[5] > wstats[5]


# ---------------------------------------------------------------------------- (4) an identity, and perm entries outside the row
def test_an_identity_symmetry_has_no_mirror_loss_and_a_perm_entry_outside_the_row_is_a_zero_column():
    case = S.make_case("aug_mirror_33_nobias")
    pa, st, pl, index, sy = build_sym(case)
    for perm, sign in ((sy.actor_perm, sy.actor_sign), (sy.critic_perm, sy.critic_sign), (sy.action_perm, sy.action_sign)):
        perm.copy_(torch.arange(len(perm), dtype=torch.int32))
        sign.fill_(1.0)
    got, stats = run(pl, st, index)
    assert float(pl.sym_stats[0]) == 0.0 and float(pl.sym_stats[1]) == case["M"] and stats[6] == 2 * case["M"]
    # -1 and K in the actor's and the critic's perm, NA in the action's: zero columns, as the restatement's
    clean = S.make_case("aug_mirror_33_nobias")
    case = dict(clean)
    for key, cols in (("actor_table", (3, 40)), ("critic_table", (0, 74)), ("action_table", (5, 19))):
        perm = case[key][0].copy()
        perm[cols[0]], perm[cols[1]] = -1, len(perm)
        case[key] = (perm, case[key][1])
    pa, st, pl, index, sy = build_sym(clean)
    for t, key in ((sy.actor_perm, "actor_table"), (sy.critic_perm, "critic_table"), (sy.action_perm, "action_table")):
        t.copy_(torch.from_numpy(case[key][0]))      # (past PolicyLearner's validation: the library's own rule)
    got, stats = run(pl, st, index)
    worst, ev = gate_ratio(case, got, stats, host(pl.sym_stats))
    assert worst <= 1.0 and all(np.isfinite(g).all() for g in got.values())
    # nothing outside the views was touched: the allocations around them are NaN as they were
    for big in st._keep:
        assert bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[-1]).all())


# ---------------------------------------------------------------------------- (5) bits: two calls, a capture, rows outside index
def test_two_calls_a_captured_backward_and_nan_outside_the_index_give_the_same_bits():
    case = S.make_case("aug_mirror_272")
    pa, st, pl, index, sy = build_sym(case)
    g1, s1 = run(pl, st, index)
    y1 = host(pl.sym_stats)
    for p in pl.parameters():
        p.grad.fill_(7.0)
    pl.sym_stats.fill_(7.0)
    g2, s2 = run(pl, st, index)
    assert all(np.array_equal(g1[k], g2[k]) for k in g1) and np.array_equal(s1, s2) and np.array_equal(y1, host(pl.sym_stats))
    # captured
    buf = torch.zeros_like(index)
    pl.backward(st, buf, adv_stats=pl.adv_stats)
    g, rewind = capture(lambda: pl.backward(st, buf, adv_stats=pl.adv_stats), pl.written())
    buf.copy_(index)
    g.replay()
    torch.cuda.synchronize()
    g3, s3 = grads_of(pl), host(pl.stats)
    assert all(np.array_equal(g1[k], g3[k]) for k in g1) and np.array_equal(s1, s3) and np.array_equal(y1, host(pl.sym_stats))
    # every stored row outside index is NaN
    unused = torch.ones(case["rows"], dtype=torch.bool, device=index.device)
    unused[index.long()] = False
    assert int(unused.sum()) > 20
    for k in ("actor_input", "critic_input", "action", "logp", "advantage", "returns"):
        getattr(st, k).view(case["rows"], -1)[unused] = float("nan")
    st.value[:-1].view(-1)[unused] = float("nan")
    g4, s4 = run(pl, st, index)
    assert all(np.array_equal(g1[k], g4[k]) for k in g1) and np.array_equal(s1, s4) and np.array_equal(y1, host(pl.sym_stats))


# ---------------------------------------------------------------------------- (6) update(), and symmetry = None
def test_update_is_the_hand_driven_loop_and_no_symmetry_is_the_parents_path():
    from tsid_control_amd import PolicyLearner
    case = S.make_case("aug_17", mirror_coef=0.5)
    pa, st, pl, index, sy = build_sym(case)
    opt = torch.optim.SGD(pl.parameters(), lr=0.05)
    run(pl, st, index)
    start = [p.detach().clone() for p in pl.parameters()]
    gen = torch.Generator(device=index.device).manual_seed(11)
    stats = pl.update(st, opt, epochs=2, minibatches=3, generator=gen).clone()
    torch.cuda.synchronize()
    ended = [p.detach().clone() for p in pl.parameters()]
    with torch.no_grad():
        for p, s in zip(pl.parameters(), start):
            p.copy_(s)
    gen = torch.Generator(device=index.device).manual_seed(11)
    pl.fill_adv_stats(st)
    mine, rows = [], case["rows"]
    for ep in range(2):
        perm = torch.randperm(rows, generator=gen, dtype=torch.int32, device=index.device)
        for k in range(3):
            mine.append(pl.backward(st, perm[k * rows // 3:(k + 1) * rows // 3].contiguous(), adv_stats=pl.adv_stats).clone())
            opt.step()
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(mine), stats) and bool(torch.isfinite(stats).all()) and list(host(stats[:, 6])) == [44.0] * 6
    assert all(torch.equal(p, e) for p, e in zip(pl.parameters(), ended)) and any(not torch.equal(s, e) for s, e in zip(start, ended))
    assert pl._last_storage is st and pl._last_index.shape[0] == 22                  # (a PolicyOptimizer's KL: the original rows)
    # symmetry = None
    pa0, st0, pl0, index0 = build(case)
    want, wstats = run(pl0, st0, index0)
    none = PolicyLearner(pa0, clip=case["clip"], value_coef=case["value_coef"], entropy_coef=case["entropy_coef"], value_clip=case["value_clip"],
                         symmetry=None, symmetry_augment=True, mirror_coef=0.0)
    none.adv_stats.copy_(pl0.adv_stats)
    got, stats = run(none, st0, index0)
    assert all(np.array_equal(got[k], want[k]) for k in want) and np.array_equal(stats, wstats) and none.sym_stats is None


# ---------------------------------------------------------------------------- (7) a real rollout
def test_mirrored_rows_of_a_real_rollout_swap_the_contact_flags():
    """8 envs, 4 steps, position mode, no randomisation; the actor's mean is a constant hip-pitch action on one leg, with the knee
    and the ankle following so that the sole stays level - the leg retracts and its foot leaves the floor: where the two contact
    flags of a stored row differ, the mirrored row has them swapped"""
    from tsid_control_amd import PolicyActor, PolicySymmetry
    from tsid_control_amd.policy_symmetry import body_frames
    env = make_env(8, "f32", decimation=16)
    NA, nobs, dev = env.NA, env.NOBS, env.device
    w = torch.zeros(NA, nobs, dtype=torch.float32, device=dev)
    b = torch.zeros(NA, dtype=torch.float32, device=dev)
    # the pitch joints of the leg of actuator 0: the hinges along the mirror normal x, from the hip down (hip pitch, knee, ankle pitch)
    origin, axis, depth = body_frames(env.wc.model)
    body = np.asarray(env.wc.model["mj_act_dof"]).astype(np.int64) - 5
    pitch = sorted((a for a in range(6) if abs(axis[body[a], 0]) > 0.99), key=lambda a: depth[body[a]])
    assert len(pitch) == 3
    for a, turn in zip(pitch, (0.5, -1.0, 0.5)):                     # rotations about +x in radians; action_scale is 0.25
        b[a] = float(np.sign(axis[body[a], 0]) * turn / 0.25)
    pa = PolicyActor(env, [(w, b)], log_std=torch.full((NA,), -8.0, dtype=torch.float32, device=dev))
    sy = PolicySymmetry(env, pa)
    st = env.rollout(pa, 4)
    torch.cuda.synchronize()
    rows = st.actor_input.reshape(-1, nobs)
    m = sy.mirror_obs(rows)
    lf, rf = rows[:, nobs - 2], rows[:, nobs - 1]
    differ = lf != rf
    print("rows whose contact flags differ:", int(differ.sum()), "of", rows.shape[0])
    assert int(differ.sum()) > 0
    assert torch.equal(m[:, nobs - 2], rf) and torch.equal(m[:, nobs - 1], lf)
    assert bool((m[differ, nobs - 2] != rows[differ, nobs - 2]).all())
    assert torch.equal(sy.mirror_obs(m), rows) and torch.equal(sy.mirror_action(sy.mirror_action(st.action)), st.action)
    # the last action's columns are the mirrored action of the step before
    assert torch.equal(m[:, 9 + 2 * NA:9 + 3 * NA], sy.mirror_action(rows[:, 9 + 2 * NA:9 + 3 * NA]))
