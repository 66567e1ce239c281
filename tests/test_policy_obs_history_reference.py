"""The numpy restatement of the observation history (tests/policy_obs_history_reference.py) against an independently written
model - one collections.deque(maxlen = frames) per env, cleared and refilled when the env is done - and the resolution of
sources into columns.  No GPU."""
import collections
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_obs_history_reference as hr  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a).tobytes()


class DequeModel:
    """one deque of frames per env"""

    def __init__(self, n, frames, K, dtype):
        self.frames = frames
        self.q = [collections.deque([np.zeros(K, dtype)] * frames, maxlen=frames) for _ in range(n)]

    def call(self, x, done, push):
        for e, q in enumerate(self.q):
            if done[e] != 0:
                q.clear()
                q.extend([x[e].copy()] * self.frames)
            elif push:
                q.append(x[e].copy())      # (maxlen: the oldest frame falls out)

    def rows(self):
        return np.stack([np.concatenate(list(q)) for q in self.q])


@pytest.mark.parametrize("frames", [1, 2, 7])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_update_is_a_deque_per_env(frames, dtype):
    n, K, calls = 9, 5, 40
    rng = np.random.default_rng(frames)
    model = DequeModel(n, frames, K, dtype)
    hist = np.zeros((n, frames * K), dtype)
    seen = dict(push=0, hold=0, some=0, every=0, none=0, nan=0)
    for t in range(calls):
        x = rng.normal(size=(n, K)).astype(dtype)
        x[rng.random((n, K)) < 0.05] = np.nan                         # (frames are copied whatever they hold)
        done = (rng.random(n) < (0.0, 0.3, 1.0)[t % 3]).astype(dtype)
        if t % 6 == 1:
            done[t % n] = np.nan                                      # (a NaN flag is a set flag: the kernel tests "not == 0")
            seen["nan"] += 1
        push = int(t % 4 != 3)
        before = hist.copy()
        hist = hr.update(hist, x, done, push)
        model.call(x, np.where(np.isnan(done), 1, done), push)
        assert bits(hist) == bits(model.rows()), t
        fresh = ~(done == 0)
        if not push:
            assert bits(hist[~fresh]) == bits(before[~fresh])         # push = 0 leaves the envs that are not done untouched
            seen["hold"] += int((~fresh).sum())
        else:
            seen["push"] += int((~fresh).sum())
        # the newest frame is the current selection of every env the call wrote, and a done env holds nothing else
        wrote = fresh | bool(push)
        assert bits(hist[wrote, -K:]) == bits(x[wrote])
        assert bits(hist[fresh]) == bits(np.tile(x[fresh], (1, frames)))
        seen["every" if fresh.all() else "some" if fresh.any() else "none"] += 1
    assert all(v >= 1 for v in seen.values()), seen


def test_update_shifts_by_one_frame():
    """written out once by hand: frames = 3, K = 2"""
    hist = np.arange(12.0).reshape(2, 6)
    x = np.array([[100.0, 101.0], [200.0, 201.0]])
    got = hr.update(hist, x, np.array([0.0, 1.0]), 1)
    assert got.tolist() == [[2, 3, 4, 5, 100, 101], [200, 201, 200, 201, 200, 201]]
    got = hr.update(hist, x, np.array([0.0, 1.0]), 0)
    assert got.tolist() == [[0, 1, 2, 3, 4, 5], [200, 201, 200, 201, 200, 201]]
    assert hist.tolist() == np.arange(12.0).reshape(2, 6).tolist()    # (the argument is not written)


def test_sources_resolve_to_columns():
    cols = dict(obs=71, priv=4, command=3, height_scan=6)
    assert hr.resolve("obs", cols) == hr.resolve(("obs",), cols) == [("obs", 0, 71)]
    r = hr.resolve((("obs", 0, 6), ("obs", 9, 71), "priv"), cols)
    assert r == [("obs", 0, 6), ("obs", 9, 71), ("priv", 0, 4)]
    cl = hr.column_list(r)
    assert len(cl) == 6 + 62 + 4 and cl[:7] == [("obs", c) for c in range(6)] + [("obs", 9)] and cl[-4:] == [("priv", c) for c in range(4)]
    assert ("obs", 6) not in cl and ("obs", 8) not in cl
    tensors = {k: np.arange(2 * n, dtype=np.float64).reshape(2, n) + 1000 * i for i, (k, n) in enumerate(cols.items())}
    x = hr.select(tensors, r)
    assert x.shape == (2, 72) and all(x[e, j] == tensors[k][e, c] for e in range(2) for j, (k, c) in enumerate(cl))
    for bad in ((), ("obs",) * 5, ("pose",), ("teacher_obs",), (("obs", 3, 3),), (("obs", -1, 3),), (("priv", 0, 5),)):
        with pytest.raises(ValueError):
            hr.resolve(bad, cols)
