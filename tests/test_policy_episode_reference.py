"""The numpy restatement of the episode statistics and the terrain curriculum (tests/policy_episode_reference.py) against an
independent formulation - a per-env Python loop over plain floats for the records, legged_gym's _update_terrain_curriculum as
vectorised torch float64 for the levels - the coverage its scenarios promise, and its stream against the randomisation's hash.
No GPU."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_dr_reference as dr  # noqa: E402
import policy_episode_reference as er  # noqa: E402

CASES = [(n, dtype, top, teacher) for n in (1, 17, 33) for dtype in (np.float64, np.float32) for top, teacher in ((True, True), (False, False))]


def loop_records(sc):
    """per call (last, sum, run, start_xy), the last two as the begin stage leaves them, from a loop over the envs in plain
    Python floats"""
    n = sc["n"]
    run = [[0.0] * er.NREC for _ in range(n)]
    last = [[0.0] * er.NREC for _ in range(n)]
    total = [[0.0] * er.NREC for _ in range(n)]
    start = [[float(v) for v in row] for row in sc["start_xy0"]]
    fin = lambda x: x if math.isfinite(x) else 0.0
    for call in sc["calls"]:
        for e in range(n):
            r = run[e]
            r[er.LENGTH] += 1.0
            r[er.RETURN] += fin(float(call["reward"][e]))
            for k in range(er.NT):
                r[er.TERMS + k] += fin(float(call["terms"][e, k]))
            if call["teacher_terms"] is not None:
                for k in range(er.TEACH_NT):
                    r[er.TEACH + k] += fin(float(call["teacher_terms"][e, k]))
            if call["done"][e] == 0:
                continue
            d = math.hypot(float(call["xy"][e, 0]) - start[e][0], float(call["xy"][e, 1]) - start[e][1])
            rec = list(r)
            rec[er.COUNT], rec[er.TIMEOUT], rec[er.LENGTH] = 1.0, float(call["timeout"][e] != 0), float(call["ep_len"][e])
            rec[er.DISPLACEMENT] = d
            last[e] = rec
            for k in range(er.NREC):
                total[e][k] += fin(rec[k]) if k in (er.RETURN, er.DISPLACEMENT) else rec[k]
            run[e] = [0.0] * er.NREC
            start[e] = [float(v) for v in call["begin_xy"][e]]
        yield np.array(last), np.array(total), np.array(run), np.array(start)


def legged_gym_levels(level, distance, command, fresh, episode, cur, L, n):
    """_update_terrain_curriculum of legged_gym on the envs `fresh`, torch float64; the random level of a graduate is the
    restatement's draw in place of torch.randint_like"""
    lvl = torch.as_tensor(np.asarray(level), dtype=torch.int64).clamp(0, L - 1)
    dist = torch.as_tensor(distance, dtype=torch.float64)
    cmd = torch.as_tensor(np.asarray(command, dtype=np.float64))
    move_up = dist > cur["up_distance"]
    move_down = (dist < torch.norm(cmd[:, :2], dim=1) * cur["t_episode"] * cur["down_fraction"]) * ~move_up
    new = lvl + 1 * move_up - 1 * move_down
    u = torch.as_tensor(dr.draw(cur["seed"], 24, 0, np.arange(n) + cur["env_offset"], np.asarray(episode, dtype=np.int64) + 1))
    rand = torch.clamp(torch.floor(u * L).long(), max=L - 1) if cur["random_top"] else torch.full((n,), L - 1)
    new = torch.where(new >= L, rand, torch.clip(new, 0))
    return torch.where(torch.as_tensor(fresh), new, torch.as_tensor(np.asarray(level), dtype=torch.int64)).numpy()


@pytest.mark.parametrize("n,dtype,top,teacher", CASES)
def test_restatement_matches_the_loop_and_legged_gyms_rule(n, dtype, top, teacher):
    sc = er.scenario(n, dtype, random_top=top, teacher=teacher)
    played, _ = er.play(sc)
    level, start = sc["level0"].copy(), sc["start_xy0"].astype(np.float64)
    worst, level_sum, last_level = 0.0, np.zeros(n), np.zeros(n)
    for rec, call, (last, total, run, start_next) in zip(played, sc["calls"], loop_records(sc)):
        fresh = call["done"] != 0
        # the LEVEL column is the rule's: the level the episode ran on, clamped
        level_sum = level_sum + np.where(fresh, np.clip(level, 0, sc["num_levels"] - 1), 0)
        total[:, er.LEVEL] = level_sum
        last[:, er.LEVEL] = last_level = np.where(fresh, np.clip(level, 0, sc["num_levels"] - 1), last_level)
        for a, b in ((rec["last"], last), (rec["sum"], total)):
            assert np.array_equal(np.isnan(a), np.isnan(b))
            worst = max(worst, float(np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(b)), initial=0.0)))
        for k in (er.COUNT, er.TIMEOUT, er.LENGTH, er.LEVEL):
            assert np.array_equal(rec["last"][:, k], last[:, k]) and np.array_equal(rec["sum"][:, k], total[:, k])
        d = np.hypot(*(call["xy"].astype(np.float64) - start).T)
        level = legged_gym_levels(level, d, call["command"], fresh, call["episode"], sc["curriculum"], sc["num_levels"], n)
        assert np.array_equal(rec["level"], level)
        assert np.array_equal(rec["start_xy"], start_next) and np.abs(rec["run"] - run).max() <= 1e-12
        start = start_next
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("n,dtype,top,teacher", CASES)
def test_scenarios_cover_every_branch(n, dtype, top, teacher):
    sc = er.scenario(n, dtype, random_top=top, teacher=teacher)
    _, count = er.play(sc)
    assert count["in_band"] == 0
    # one env lives through role 0 alone: up from the top (a graduation), a NaN reward step, a termination, then down by a timeout
    need = ["up", "down", "termination", "timeout", "finishes_twice", "nan_step", "graduate_random" if top else "graduate_top"]
    if n >= 11:
        need += ["neither", "level_below", "level_above", "nan_position", "never_finishes"]
    if not teacher:
        need.append("teacher_null")
    for k in need:
        assert count[k] >= 1, (k, count)
    assert count["graduate_top" if top else "graduate_random"] == 0 and (count["teacher_null"] == 0) == teacher
    # the NaN inputs reached a record without poisoning a sum
    played, _ = er.play(sc)
    assert np.isfinite(played[-1]["sum"]).all() and np.isfinite(played[-1]["run"]).all()
    if n >= 11:
        assert np.isnan(np.stack([p["last"] for p in played])[:, :, er.DISPLACEMENT]).any()
    # with the curriculum off the levels stay, with no level pointer the column is 0
    off, _ = er.play(sc, curriculum=False)
    assert all(np.array_equal(p["level"], sc["level0"]) for p in off)
    none, _ = er.play(sc, level=False)
    assert all(p["level"] is None and (p["last"][:, er.LEVEL] == 0).all() for p in none)
    rest = [k for k in range(er.NREC) if k != er.LEVEL]          # (the levels the episodes ran on differ, nothing else)
    for a, b in zip(off, played):
        for k in ("last", "sum", "run"):
            assert np.array_equal(a[k][:, rest], b[k][:, rest], equal_nan=True)
        assert np.array_equal(a["start_xy"], b["start_xy"])


def test_a_random_graduate_lands_on_every_level_and_follows_the_env_offset():
    n, L = 66, 3
    sc = er.scenario(n, random_top=True, num_levels=L)
    played, _ = er.play(sc)
    landed = set()
    lvl = sc["level0"].copy()
    for call, p in zip(sc["calls"], played):
        fresh = call["done"] != 0
        graduated = fresh & p["up"] & (np.clip(lvl, 0, L - 1) == L - 1)
        landed.update(p["level"][graduated].tolist())
        lvl = p["level"]
    assert landed == set(range(L))
    # a split batch: the rows of the whole one
    for sl in (slice(0, 33), slice(33, 66)):
        part, _ = er.play(er.rows_of(sc, sl))
        for a, b in zip(part, played):
            for k in ("last", "sum", "run", "start_xy", "level"):
                assert np.array_equal(a[k], b[k][sl], equal_nan=True), k


def test_stream_24_is_the_randomisations_hash():
    env, ep = np.arange(40), np.arange(40) % 7 + 1
    for seed, off in ((5, 0), (2 ** 32 - 1, 16), (0, 2 ** 31 - 41)):
        assert np.array_equal(er.graduate_draw(seed, off, env, ep), dr.draw(seed, 24, 0, env + off, ep))
    assert dr.key(5, 24) == 5 + ((24 * 256) << 32) and er.STREAM == 24
    u = er.graduate_draw(5, 0, np.arange(4096), np.ones(4096, dtype=np.int64))
    assert 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.02
    # another stream, another draw
    assert not np.array_equal(u, dr.draw(5, 23, 0, np.arange(4096), np.ones(4096, dtype=np.int64)))
