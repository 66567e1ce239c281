"""Direct actuator control (tsidb_set_ctrl / tsidb_sim_ctrl), the parts that need no GPU: the binding against the header, the
order helpers against the blobs of both robots, and how sim_steps() splits its steps over launches."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def header_enums():
    """every NAME = integer of include/tsidb.h's enums"""
    text = (ROOT / "include" / "tsidb.h").read_text()
    return {k: int(v) for k, v in re.findall(r"\b(TSIDB_[A-Z0-9_]+)\s*=\s*(-?\d+)\b", text)}


def test_binding_matches_the_header():
    from tsid_control_amd import _lib
    text = (ROOT / "include" / "tsidb.h").read_text()
    en = header_enums()
    assert (_lib.CTRL_OFF, _lib.CTRL_POSITION, _lib.CTRL_MOTOR, _lib.CTRL_RESIDUAL) == \
        (en["TSIDB_CTRL_OFF"], en["TSIDB_CTRL_POSITION"], en["TSIDB_CTRL_MOTOR"], en["TSIDB_CTRL_RESIDUAL"]) == (0, 1, 2, 3)
    assert _lib.CTRL_MODES == dict(position=en["TSIDB_CTRL_POSITION"], motor=en["TSIDB_CTRL_MOTOR"], residual=en["TSIDB_CTRL_RESIDUAL"])
    assert _lib.MAX_SIM_BATCH == en["TSIDB_MAX_SIM_BATCH"]
    # the prototypes: as many arguments as the header declares, and both libraries export them
    for name in ("tsidb_set_ctrl", "tsidb_sim_ctrl"):
        assert name in _lib.SYMBOLS
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert m, name
        nargs = len(m.group(1).split(","))
        for lib in sorted((ROOT / "tsid_control_amd").glob("libtsidb*.so")):
            fn = getattr(_lib.load(lib), name)
            assert len(fn.argtypes) == nargs and fn.restype is C.c_int, (name, lib.name)
    assert len(list((ROOT / "tsid_control_amd").glob("libtsidb*.so"))) >= 2


def bare_controller(blob_path=None):
    """a WalkController with its model and sizes but no device and no library handle"""
    from tsid_control_amd.model import ModelBlob
    from tsid_control_amd.walk_controller import WalkController
    wc = object.__new__(WalkController)
    wc.model = ModelBlob(blob_path)
    wc._ctrl_qidx = None
    wc._pipe = None
    d = [int(x) for x in wc.model["model_dims"]]
    wc.NQ, wc.NV, wc.NA = d[1], d[2], d[3]
    return wc


@pytest.mark.parametrize("v0", [False, True])
def test_order_helpers_agree_with_the_blob(v0):
    from tsid_control_amd import op3_v0_conf
    from tsid_control_amd.walk_controller import map_tsid_to_mujoco
    wc = bare_controller(op3_v0_conf().model_blob if v0 else None)
    qidx = np.asarray(wc.model["mj_ctrl_qidx"])
    assert len(qidx) == wc.NA and sorted(qidx.tolist()) == list(range(7, wc.NQ))         # a permutation of the joints
    q = torch.arange(2 * wc.NQ, dtype=torch.float64).reshape(2, wc.NQ)
    got = wc.ctrl_from_q(q)
    assert got.shape == (2, wc.NA)
    assert torch.equal(got, map_tsid_to_mujoco(q, wc.model)) and np.array_equal(got[0].numpy(), qidx.astype(np.float64))
    tau = torch.arange(2 * wc.NA, dtype=torch.float64).reshape(2, wc.NA)
    got = wc.ctrl_from_tau(tau)
    assert np.array_equal(got[0].numpy(), (qidx - 7).astype(np.float64)) and np.array_equal(got[1].numpy(), (qidx - 7 + wc.NA).astype(np.float64))
    # the two agree: the joints of q, as a torque-ordered vector, land in the same actuator slots
    assert torch.equal(wc.ctrl_from_tau(q[:, 7:]), wc.ctrl_from_q(q))
    assert torch.equal(wc.ctrl_from_q(q[0]), wc.ctrl_from_q(q)[0])                        # (any leading shape)


def test_sim_steps_splits_into_launches_of_at_most_eight():
    wc = bare_controller()
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt)
    wc.qpos, wc.qvel, wc.qacc_warmstart = z(2, wc.NQ), z(2, wc.NV), z(2, wc.NV)
    wc.ncon, wc.con_pairs, wc.info = z(2, dt=torch.int32), z(2, 32, dt=torch.int32), z(2, 4, dt=torch.int32)
    calls = []
    wc._call = lambda name, *args: calls.append((name, args))
    wc._stream = lambda: C.c_void_p(0)
    for n, want in ((11, [8, 3]), (8, [8]), (1, [1]), (16, [8, 8]), (17, [8, 8, 1]), (0, [])):
        calls.clear()
        out = wc.sim_steps(n)
        assert [c[0] for c in calls] == ["tsidb_sim_ctrl"] * len(want) and [c[1][0] for c in calls] == want, (n, calls)
        assert out[0] is wc.qpos and out[1] is wc.qvel
        for _, args in calls:
            assert len(args) == 9 and args[1].value == wc.qpos.data_ptr() and args[2].value == wc.qvel.data_ptr() \
                and args[3].value == wc.qacc_warmstart.data_ptr() and args[4] is None
