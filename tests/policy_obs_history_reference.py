"""numpy restatement of the observation history of the policy environment (include/tsidb.h tsidb_policy_obs_history;
PolicyEnv(obs_history=)): the resolution of `sources` into columns and the push / fill rule on given frames, done flags and
push.  Nothing is computed: the history holds copies, so every comparison against this file is bit for bit.  Not a test module:
imported by the tests."""
import numpy as np

SOURCES = ("obs", "priv", "command", "height_scan", "teacher_obs")
MAXSRC, MAXFRAMES, MAXCOLS = 4, 32, 4096


def resolve(sources, columns):
    """[(name, lo, hi)] of `sources` - names or (name, lo, hi) - with columns = {name: the width of the env's tensor}; a name
    alone is all of its columns"""
    if isinstance(sources, str):
        sources = (sources,)
    if not 1 <= len(sources) <= MAXSRC:
        raise ValueError(f"1 .. {MAXSRC} sources, got {len(sources)}")
    out = []
    for s in sources:
        name, lo, hi = (s, 0, None) if isinstance(s, str) else s
        if name not in SOURCES or name not in columns:
            raise ValueError(f"unknown source {name!r}")
        hi = columns[name] if hi is None else hi
        if not 0 <= lo < hi <= columns[name]:
            raise ValueError(f"range ({lo}, {hi}) outside {name} [0, {columns[name]})")
        out.append((name, int(lo), int(hi)))
    return out


def column_list(resolved):
    """the columns of a frame, in order: [(name, column of that tensor)], K entries"""
    return [(name, c) for name, lo, hi in resolved for c in range(lo, hi)]


def select(tensors, resolved):
    """x [N, K]: the current frame of every env, from tensors = {name: [N, columns] array}"""
    return np.concatenate([np.asarray(tensors[name])[:, lo:hi] for name, lo, hi in resolved], axis=1)


def update(history, x, done, push):
    """history [N, frames * K] after one launch: an env whose done flag is set (anything but 0, NaN included) holds `frames`
    copies of x[e]; any other env, with push, drops its oldest frame and gets x[e] as its newest; without push it is untouched"""
    x = np.asarray(x)
    n, K = x.shape
    frames = history.shape[1] // K
    assert history.shape == (n, frames * K) and 1 <= frames <= MAXFRAMES and frames * K <= MAXCOLS
    h = history.reshape(n, frames, K).copy()
    fill = ~(np.asarray(done) == 0)
    if push:
        keep = ~fill
        h[keep, :-1] = h[keep, 1:]
        h[keep, -1] = x[keep]
    h[fill] = x[fill][:, None, :]
    return h.reshape(n, frames * K)
