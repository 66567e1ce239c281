"""The sim kernel's results, bit for bit, against tests/golden/sim_step_bits.npz - arrays recorded once, on a GPU, at the commit
named in the file (tests/golden/make_sim_step_bits.py, which also defines the runs; DESIGN.md section 5 "Fixed phases of
k_sim").  Changes to k_sim that reorder loads, drop passes or move work between lanes without touching the arithmetic must
reproduce every array exactly, in every shape of the kernel: the library's default, one and two wavefronts per env, one and
eight sim steps per launch.  No tolerance anywhere: np.array_equal on the raw bytes."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_sim_step_bits", Path(__file__).parent / "golden" / "make_sim_step_bits.py")
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    return np.load(gen.FIXTURE)


def _want(golden, case, variant, s, k):
    own = f"{case}@{variant}/{s}/{k}"   # (a shape that rounded differently at the recording commit has a copy of its own)
    return golden[own] if own in golden.files else golden[f"{case}/{s}/{k}"]


@pytest.mark.parametrize("case,variant", [(c, v) for c in gen.CASES for v in gen.variants_of(c)])
def test_sim_step_bits(golden, case, variant):
    snaps, cov = gen.run_case(case, variant)
    assert np.array_equal(cov, golden[f"{case}/cov"]), (case, variant, dict(zip(gen.COV_FIELDS, cov.tolist())))
    n_snap = len([f for f in golden.files if f.startswith(case + "/") and f.endswith("/qpos")])
    assert len(snaps) == n_snap > 0
    for s, snap in enumerate(snaps):
        for k in gen.FIELDS:
            want = _want(golden, case, variant, s, k)
            assert snap[k].dtype == want.dtype and snap[k].shape == want.shape, (case, variant, s, k)
            assert np.array_equal(snap[k].view(np.uint8), want.view(np.uint8)), (case, variant, s, k)


def test_fixture_covers_what_it_is_for(golden):
    """the recorded runs reached the paths they were chosen for (so that an exact match means something): surviving hull
    pairs, the contact cap and its flag, three and more contact groups, cross-branch contacts (the dense Newton factor),
    touch-down windows with several Newton iterations - and no step in them was skipped as non-finite (flag bit 4)"""
    assert bytes(golden["parent_commit"]).decode() != "unknown"
    cov = {c: dict(zip(gen.COV_FIELDS, golden[f"{c}/cov"].tolist())) for c in gen.CASES}
    for c in gen.CASES:
        assert not cov[c]["flags_or"] & 4 and np.isfinite(golden[f"{c}/0/qpos"]).all(), c
    for c in ("a_walk_f64", "d_walk_f32"):
        assert cov[c]["ncon_max"] >= 8 and cov[c]["newton_iters_max"] >= 3, c      # double support (2 x 4 sole corners), a touch-down
        assert int(golden[f"{c}/2/ncon"].min()) >= 1
    b = cov["b_selfcol"]
    assert b["ncon_max"] == 32 and b["flags_or"] & 8                                # the contact cap, flagged
    assert b["hull_pair_contacts"] > 0 and b["cross_branch_contacts"] > 0 and b["floor_contact_bodies_max"] >= 3
    assert cov["c_terrain"]["ncon_max"] >= 8
    e = cov["e_v0_selfcol"]
    assert e["hull_pair_contacts"] > 0 and e["cross_branch_contacts"] > 0 and e["floor_contact_bodies_max"] >= 3
