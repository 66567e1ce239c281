"""The TSID tick's results, bit for bit, against tests/golden/tick_bits.npz - arrays recorded once, on a GPU, at the commit
named in the file (tests/golden/make_tick_bits.py, which also defines the runs; DESIGN.md section 5 "Register
factorisations").  Changes to k_tick that move values between registers, lanes and LDS without touching the arithmetic
must reproduce every array exactly: all three contact configurations (50 / 38 / 26 variables), float64 and float32, the
fast equality solve and the QR / active-set path behind it.  No tolerance anywhere: np.array_equal on the raw bytes."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_tick_bits", Path(__file__).parent / "golden" / "make_tick_bits.py")
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    return np.load(gen.FIXTURE)


@pytest.mark.parametrize("dtype,run", [(d, r) for d in gen.DTYPES for r in gen.RUNS])
def test_tick_bits(golden, dtype, run):
    snaps = gen.run(dtype, run)
    assert len(snaps) == len(gen.SNAPSHOTS)
    for s, snap in enumerate(snaps):
        for k in gen.FIELDS:
            want = golden[f"{dtype}/{run}/{s}/{k}"]
            assert snap[k].dtype == want.dtype and snap[k].shape == want.shape, (dtype, run, s, k)
            assert np.array_equal(snap[k].view(np.uint8), want.view(np.uint8)), (dtype, run, s, k)
    if run == "tight":   # the same conditions on what this build computed
        assert int((snaps[0]["info"][:, 0] > 1).sum()) >= 8
    assert not any((snap["status"] == 4).any() for snap in snaps)


def test_fixture_covers_what_it_is_for(golden):
    """the recorded runs contain what they were chosen for: at least 12 envs of each contact configuration, at least 8 envs
    of the tight-bounds run past the fast equality solve (more than one active-set iteration), no env skipped as
    non-finite (status 4)"""
    assert bytes(golden["parent_commit"]).decode() != "unknown"
    gen.check_conditions(lambda dt, r, s, k: golden[f"{dt}/{r}/{s}/{k}"])
