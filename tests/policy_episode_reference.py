"""Numpy float64 restatement of the episode statistics and the terrain curriculum (tsidb_policy_episode_end / _begin), written
from their description in include/tsidb.h, vectorised over the envs, and a generator of synthetic scenarios that make every
branch of the two kernels occur by construction.  Inputs are taken in the dtype the device holds them in (the path's type) and
cast to float64 first, as the kernels do; everything behind that is float64.  tests/test_policy_episode_reference.py pins this
module against an independent formulation."""
import numpy as np

from policy_reference import uniform

COUNT, TIMEOUT, LENGTH, RETURN, DISPLACEMENT, LEVEL, TERMS = range(7)
NT, TEACH_NT = 12, 4
TEACH = TERMS + NT
NREC = TEACH + TEACH_NT
STREAM = 24          # the graduate's level (the header's key table)
BAND = 1e-6          # no displacement of a scenario lies this close [m] to a threshold of the curriculum


def finite(x):
    """x where it is finite, else 0"""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isfinite(x), x, 0.0)


def graduate_draw(seed, env_offset, env, next_episode):
    """U of stream 24, column 0: key = seed + ((24 * 256 + 0) << 32), env index env_offset + env, counter = the episode about to
    start"""
    return uniform(int(seed) + ((STREAM * 256) << 32), np.asarray(env, dtype=np.int64) + int(env_offset), next_episode)


class PolicyEpisodeReference:
    """run, start_xy, last, sum of n envs and the two stages.  num_levels = 0: no terrain configured (levels are clamped to
    >= 0 only).  curriculum: None, or dict(up_distance, down_fraction, random_top, seed, env_offset, t_episode) with seed and
    env_offset the terrain's and t_episode = max_episode_steps * (decimation * dt)."""

    def __init__(self, n, num_levels=0, curriculum=None):
        self.n, self.num_levels, self.cur = n, int(num_levels), curriculum
        self.run, self.last, self.sum = np.zeros((n, NREC)), np.zeros((n, NREC)), np.zeros((n, NREC))
        self.start_xy = np.zeros((n, 2))
        self.moved = dict(up=np.zeros(n, bool), down=np.zeros(n, bool), graduated=np.zeros(n, bool))
        self.d = np.full(n, np.nan)
        self.down_threshold = np.full(n, np.nan)

    def clamp(self, level):
        lvl = np.maximum(np.asarray(level, dtype=np.int64), 0)
        return np.minimum(lvl, self.num_levels - 1) if self.num_levels > 0 else lvl

    def end(self, terms, teacher_terms, reward, done, timeout, ep_len, episode, command, xy, level):
        """after the reward, before the reset.  level [n] int (None: no pointer).  Returns the level array as the launch leaves
        it (None where none was given)"""
        n = self.n
        fresh = np.asarray(done) != 0
        self.run[:, LENGTH] += 1.0
        self.run[:, RETURN] += finite(reward)
        self.run[:, TERMS:TEACH] += finite(terms)
        if teacher_terms is not None:
            self.run[:, TEACH:] += finite(teacher_terms)
        delta = np.asarray(xy, dtype=np.float64)[:, :2] - self.start_xy
        d = np.sqrt(delta[:, 0] * delta[:, 0] + delta[:, 1] * delta[:, 1])
        lvl = self.clamp(level) if level is not None else np.zeros(n, dtype=np.int64)
        rec = self.run.copy()
        rec[:, COUNT], rec[:, TIMEOUT], rec[:, LENGTH] = 1.0, (np.asarray(timeout) != 0).astype(np.float64), np.asarray(ep_len, dtype=np.float64)
        rec[:, DISPLACEMENT], rec[:, LEVEL] = d, lvl.astype(np.float64)
        add = rec.copy()
        add[:, RETURN], add[:, DISPLACEMENT] = finite(rec[:, RETURN]), finite(rec[:, DISPLACEMENT])
        self.last = np.where(fresh[:, None], rec, self.last)
        self.sum = self.sum + np.where(fresh[:, None], add, 0.0)
        self.d = np.where(fresh, d, np.nan)
        for k in self.moved:
            self.moved[k] = np.zeros(n, bool)
        if level is None:
            return None
        out = np.asarray(level).copy()
        if self.cur is not None:
            c, L = self.cur, self.num_levels
            cmd = np.asarray(command, dtype=np.float64)
            thr = c["down_fraction"] * np.sqrt(cmd[:, 0] * cmd[:, 0] + cmd[:, 1] * cmd[:, 1]) * c["t_episode"]
            with np.errstate(invalid="ignore"):
                up = d > c["up_distance"]
                down = ~up & (d < thr)
            nxt = lvl + up.astype(np.int64) - down.astype(np.int64)
            u = graduate_draw(c["seed"], c["env_offset"], np.arange(n), np.asarray(episode, dtype=np.int64) + 1)
            top = np.minimum(L - 1, np.floor(u * L).astype(np.int64)) if c["random_top"] else np.full(n, L - 1, dtype=np.int64)
            graduated = nxt >= L
            nxt = np.where(nxt < 0, 0, np.where(graduated, top, nxt))
            out = np.where(fresh, nxt, out).astype(out.dtype)
            self.moved = dict(up=fresh & up, down=fresh & down, graduated=fresh & graduated)
            self.down_threshold = np.where(fresh, thr, np.nan)
        return out

    def begin(self, done, xy):
        """after the reset, its noise and the terrain's redraw"""
        fresh = np.asarray(done) != 0
        self.start_xy = np.where(fresh[:, None], np.asarray(xy, dtype=np.float64)[:, :2], self.start_xy)
        self.run = np.where(fresh[:, None], 0.0, self.run)

    def means(self):
        """what PolicyEnv.episode_stats() returns, from sum: (episodes, timeouts, the means of the other columns [NREC])"""
        s = self.sum.sum(0)
        return s[COUNT], s[TIMEOUT], s / max(s[COUNT], 1.0)


# ---------------------------------------------------------------------------- scenarios
# what the env of role r = env % 11 lives through: (call, kind, timeout, NaN position) of each episode end, its first level
ROLES = {
    0: dict(level="top", ends=[(2, "up", False, False), (5, "down", True, False)]),       # graduates from the top, finishes twice
    1: dict(level=2, ends=[]),                                                            # never finishes
    2: dict(level=0, ends=[(3, "neither", True, False)]),
    3: dict(level=-2, ends=[(4, "down", False, False)]),                                  # below 0 on the way in, down: stays 0
    4: dict(level="above", ends=[(4, "up", True, False)]),                                # above the top on the way in, graduates
    5: dict(level=1, ends=[(1, "up", False, True)]),                                      # NaN position: the level stays
    6: dict(level=0, ends=[(6, "up", True, False)]),                                      # a NaN term and an inf teacher term at call 3
    7: dict(level=1, ends=[(2, "down", False, False), (6, "up", False, False)]),
    8: dict(level=1, ends=[(7, "zero", True, False)]),                                    # command 0: no distance asked for, stays
    9: dict(level=1, ends=[(0, "up", False, False)]),                                     # done at the very first call
    10: dict(level="top", ends=[(3, "up", False, False)]),
}
FACTOR = dict(up=1.5, down=0.3, neither=0.8, zero=0.1)   # d / up_distance; the down threshold is 0.6 up_distance (0 for "zero")


def scenario(n, dtype=np.float64, *, random_top=True, teacher=True, num_levels=3, up_distance=0.5, down_fraction=0.5, t_episode=10.0,
             seed=5, env_offset=0, calls=8, rng_seed=0):
    """A dict: the configuration, the state before the first call (start_xy0, level0, episode 1 running for every env - one
    tsidb_policy_episode_begin with every flag set) and per call the inputs of one end / begin pair, every array in `dtype`
    where the device holds it in the path's type"""
    assert down_fraction > 0 and num_levels >= 3 and calls >= 8
    rng = np.random.default_rng(rng_seed)
    role = np.arange(n) % len(ROLES)
    lvl0 = {"top": num_levels - 1, "above": num_levels + 3}
    level0 = np.array([lvl0.get(ROLES[r]["level"], ROLES[r]["level"]) for r in role], dtype=np.int32)
    cmd_mag = 0.6 * up_distance / (down_fraction * t_episode)
    start = rng.uniform(-2.0, 2.0, (n, 2)).astype(dtype)
    sc = dict(n=n, dtype=dtype, num_levels=num_levels, teacher=teacher, level0=level0, start_xy0=start.copy(), calls=[],
              curriculum=dict(up_distance=up_distance, down_fraction=down_fraction, random_top=random_top, seed=seed, env_offset=env_offset,
                              t_episode=t_episode))
    ep_len, episode = np.zeros(n, dtype=np.int32), np.ones(n, dtype=np.int32)
    for c in range(calls):
        terms, reward = rng.uniform(-1.0, 1.0, (n, NT)).astype(dtype), rng.uniform(-2.0, 2.0, n).astype(dtype)
        tt = rng.uniform(0.0, 2.0, (n, TEACH_NT)).astype(dtype) if teacher else None
        az = rng.uniform(0.0, 2.0 * np.pi, n)
        command = np.stack([cmd_mag * np.cos(az), cmd_mag * np.sin(az), rng.uniform(-1.0, 1.0, n)], axis=1).astype(dtype)
        xy = rng.uniform(-2.0, 2.0, (n, 2)).astype(dtype)
        done, timeout = np.zeros(n, dtype=dtype), np.zeros(n, dtype=np.int32)
        if c == 1:
            reward[role == 0] = np.nan
        if c == 3:
            terms[role == 6, 2] = np.nan
            if teacher:
                tt[role == 6, 1] = np.inf
        ep_len = ep_len + 1
        for e in range(n):
            for call, kind, tmo, nan_pos in ROLES[role[e]]["ends"]:
                if call != c:
                    continue
                done[e], timeout[e] = 1, int(tmo)
                a = rng.uniform(0.0, 2.0 * np.pi)
                xy[e] = (start[e].astype(np.float64) + FACTOR[kind] * up_distance * np.array([np.cos(a), np.sin(a)])).astype(dtype)
                if kind == "zero":
                    command[e, :2] = 0
                if nan_pos:
                    xy[e, 0] = np.nan
        begin_xy = xy.copy()
        fresh = done != 0
        begin_xy[fresh] = rng.uniform(-2.0, 2.0, (int(fresh.sum()), 2)).astype(dtype)
        sc["calls"].append(dict(terms=terms, teacher_terms=tt, reward=reward, done=done, timeout=timeout, ep_len=ep_len.copy(),
                                episode=episode.copy(), command=command, xy=xy, begin_xy=begin_xy))
        start = np.where(fresh[:, None], begin_xy, start)
        ep_len, episode = np.where(fresh, 0, ep_len).astype(np.int32), (episode + fresh).astype(np.int32)
    return sc


def rows_of(sc, sl):
    """the scenario of the envs sl alone (a slice), env_offset moved by its start: what a rank of a split batch holds"""
    pick = lambda v: v[sl] if isinstance(v, np.ndarray) else v
    out = dict(sc, n=len(range(*sl.indices(sc["n"]))), level0=sc["level0"][sl], start_xy0=sc["start_xy0"][sl],
               curriculum=dict(sc["curriculum"], env_offset=sc["curriculum"]["env_offset"] + sl.start),
               calls=[{k: pick(v) for k, v in call.items()} for call in sc["calls"]])
    return out


def reference_of(sc, curriculum=True):
    """the restatement in the state before the scenario's first call"""
    ref = PolicyEpisodeReference(sc["n"], sc["num_levels"], sc["curriculum"] if curriculum else None)
    ref.begin(np.ones(sc["n"]), sc["start_xy0"])
    return ref


def play(sc, curriculum=True, level=True):
    """the restatement over the whole scenario: per call a dict of copies of run, start_xy, last, sum (after end: *_end; after
    begin: run, start_xy), the level after end, and what moved; plus the branch counts"""
    ref = reference_of(sc, curriculum)
    lvl = sc["level0"].copy() if level else None
    out, n = [], sc["n"]
    count = dict(up=0, down=0, neither=0, graduate_random=0, graduate_top=0, level_below=0, level_above=0, nan_position=0, nan_step=0,
                 timeout=0, termination=0, never_finishes=0, finishes_twice=0, teacher_null=0, in_band=0)
    finished = np.zeros(n, dtype=int)
    for call in sc["calls"]:
        fresh = call["done"] != 0
        if lvl is not None:
            count["level_below"] += int((fresh & (lvl < 0)).sum())
            count["level_above"] += int((fresh & (lvl > sc["num_levels"] - 1)).sum())
        lvl = ref.end(call["terms"], call["teacher_terms"], call["reward"], call["done"], call["timeout"], call["ep_len"], call["episode"],
                      call["command"], call["xy"], lvl)
        m = ref.moved
        rec = dict(run_end=ref.run.copy(), last=ref.last.copy(), sum=ref.sum.copy(), level=None if lvl is None else lvl.copy(),
                   up=m["up"].copy(), down=m["down"].copy(), d=ref.d.copy())
        ref.begin(call["done"], call["begin_xy"])
        rec.update(run=ref.run.copy(), start_xy=ref.start_xy.copy())
        out.append(rec)
        finished += fresh
        count["up"] += int(m["up"].sum())
        count["down"] += int(m["down"].sum())
        count["neither"] += int((fresh & ~m["up"] & ~m["down"] & np.isfinite(ref.d)).sum())
        count["graduate_random" if sc["curriculum"]["random_top"] else "graduate_top"] += int(m["graduated"].sum())
        count["nan_position"] += int((fresh & np.isnan(ref.d)).sum())
        count["nan_step"] += int((~np.isfinite(call["reward"].astype(np.float64))).sum() + (~np.isfinite(call["terms"].astype(np.float64))).any(1).sum())
        count["timeout"] += int((fresh & (call["timeout"] != 0)).sum())
        count["termination"] += int((fresh & (call["timeout"] == 0)).sum())
        count["teacher_null"] += int(call["teacher_terms"] is None)
        if curriculum:
            with np.errstate(invalid="ignore"):
                near = (np.abs(ref.d - sc["curriculum"]["up_distance"]) <= BAND) | (np.abs(ref.d - ref.down_threshold) <= BAND)
            count["in_band"] += int((fresh & near).sum())
    count["never_finishes"], count["finishes_twice"] = int((finished == 0).sum()), int((finished >= 2).sum())
    return out, count
