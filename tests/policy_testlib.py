"""What the policy layer's tests share (tests/test_policy_*_host.py, tests/test_gpu_policy_*.py): the header's enums, the check of
the prototypes, and on the GPU the small conversions, the env constructors, PolicyEnv.step() stage by stage and the graph
capture against an eager twin.  Not a test module: imported like policy_reference.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "tsidb.h").read_text()


def header_enums(prefix=""):
    """{name: value} of the enumerators of include/tsidb.h that start with `prefix`: explicit values, running offsets and
    expressions over earlier names (`= TSIDB_POL_P_CMD_LO + 3`) resolved"""
    en = {}
    for body in re.findall(r"\benum\s*\{(.*?)\}\s*;", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S), re.S):
        nxt = 0
        for item in body.split(","):
            name, _, expr = (s.strip() for s in item.strip().partition("="))
            if name:
                en[name] = nxt = int(eval(expr, {"__builtins__": {}}, en)) if expr else nxt
                nxt += 1
    return {k: v for k, v in en.items() if k.startswith(prefix)}


def assert_prototypes(names):
    """the binding has every name with as many arguments as the header declares, and both libraries export them"""
    from tsid_control_amd import _lib
    libs = sorted((ROOT / "tsid_control_amd").glob("libtsidb*.so"))
    assert len(libs) >= 2
    for name in names:
        assert name in _lib.SYMBOLS
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", HEADER)
        assert m, name
        nargs = len(m.group(1).split(","))
        for lib in libs:
            fn = getattr(_lib.load(lib), name)
            assert len(fn.argtypes) == nargs and fn.restype is C.c_int, (name, lib.name)


# ---------------------------------------------------------------------------- on the GPU
def host(t):
    return t.detach().cpu().numpy().copy()


def rel(a, b):
    """largest |a - b| / max(1, |b|); NaN only where both are"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    with np.errstate(invalid="ignore"):
        return float(np.nanmax(np.concatenate([[0.0], (np.abs(a - b) / np.maximum(1.0, np.abs(b))).reshape(-1)])))


def same(a, b):
    """bit for bit, NaN where the other has NaN"""
    return torch.equal(a, b) or bool((torch.isnan(a) == torch.isnan(b)).all()) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def conf_of(dtype="f64", v0=False, closed_loop=False):
    """the v1 or the v0 robot's conf; closed_loop: as PolicyEnv(tsid=...) needs it"""
    from tsid_control_amd import RobotConfig, op3_v0_conf
    conf = op3_v0_conf() if v0 else RobotConfig()
    conf.dtype = dtype
    if closed_loop:
        conf.closed_loop = True
        conf.reference_quirks = False
    if v0:
        conf.done_base_height = 0.12    # (the v0 robot stands lower than the v1 robot's default fall height)
    return conf


def make_env(n, conf="f64", v0=False, **kw):
    """PolicyEnv of n envs on cuda:0; conf: a RobotConfig, or the dtype of conf_of(dtype, v0)"""
    from tsid_control_amd import PolicyEnv
    return PolicyEnv(conf_of(conf, v0) if isinstance(conf, str) else conf, num_envs=n, device="cuda:0", **kw)


def staged_step(env, action, after_act=None, before_reward=None, after_reward=None, after_teacher=None):
    """PolicyEnv.step() stage by stage, with or without tsid (no terrain), with hooks where a test reads or writes what the
    next stage uses"""
    hook = lambda fn: fn and fn()
    env._act(action)
    hook(after_act)
    if env._dr_push:
        env._perturb()
    if env.tsid is None:
        env.wc.sim_steps(env.decimation)
    else:
        env._tsid_steps()
    hook(before_reward)
    env._reward()
    hook(after_reward)
    if env.tsid is not None:
        env._teacher()
        hook(after_teacher)
    env.wc.reset_done()
    if env.sched is not None:
        env._replan()
    if env._dr_reset:
        env._reset_noise()
    env._obs()
    if env.tsid is not None:
        env._teacher_obs()


def capture(fn, written):
    """fn() captured in a torch.cuda.graph on one stream: a warm-up on a side stream (lazy kernel loads), the tensors `written`
    rewound to what they held, the capture - which runs nothing: nothing may have moved.  Returns (graph, rewind)"""
    saved = [x.clone() for x in written]

    def rewind():
        for x, s in zip(written, saved):
            x.copy_(s)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    rewind()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for x, s in zip(written, saved):
        assert torch.equal(x, s)
    return g, rewind


def replay_against_eager(env, eager, actions):
    """env.step() captured (capture() above), then per action one replay against one eager step of the twin `eager`: every
    written tensor bit for bit.  Yields the step number after each comparison, for the test's own counters and assertions"""
    buf = torch.zeros_like(actions[0])
    g, _ = capture(lambda: env.step(buf), list(env.written()))
    for t, action in enumerate(actions):
        buf.copy_(action)
        g.replay()
        eager.step(action)
        torch.cuda.synchronize()
        for a, b in zip(env.written(), eager.written()):
            assert same(a, b), t
        yield t
