"""The TSID tick's results, bit for bit, against tests/golden/tick_bits_more.npz - arrays recorded once, on a GPU, at the
commit named in the file (tests/golden/make_tick_bits_more.py, which also defines the runs).  What tests/golden/tick_bits.npz
leaves out: the second robot's build of the library (libtsidb_v0.so; 48 / 36 / 24 variables, envs past the fast equality
solve) and v1 walkers on the host-planned schedule with start delays, so that double- and single-support bodies run in one
launch and envs change their support foot between the snapshots, in float64 and float32.  Changes to k_tick that move
values between registers, lanes and LDS, or leave out products with structural zeros, must reproduce every array exactly:
np.array_equal on the raw bytes, no tolerance anywhere."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_tick_bits_more", Path(__file__).parent / "golden" / "make_tick_bits_more.py")
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    return np.load(gen.FIXTURE)


@pytest.mark.parametrize("case", gen.CASES)
def test_tick_bits_more(golden, case):
    snaps = gen.run(case)
    assert len(snaps) == gen.n_snapshots(case)
    for s, snap in enumerate(snaps):
        for k in gen.FIELDS:
            want = golden[f"{case}/{s}/{k}"]
            assert snap[k].dtype == want.dtype and snap[k].shape == want.shape, (case, s, k)
            assert np.array_equal(snap[k].view(np.uint8), want.view(np.uint8)), (case, s, k)
    assert not any((snap["status"] == 4).any() for snap in snaps)


def test_fixture_covers_what_it_is_for(golden):
    """the recorded runs contain what they were chosen for: v0 envs of every contact configuration with at least 8 past the
    fast equality solve, at least 12 walkers of each contact configuration with double- and single-support bodies in every
    recorded launch and a touch-down between the snapshots, no env skipped as non-finite (status 4)"""
    assert bytes(golden["parent_commit"]).decode() != "unknown"
    gen.check_conditions(lambda c, s, k: golden[f"{c}/{s}/{k}"])
