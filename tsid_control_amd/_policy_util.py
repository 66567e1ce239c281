"""What the policy classes (policy_actor.py, policy_normalizer.py, policy_learner.py, policy_optimizer.py, policy_symmetry.py)
share on the host: the argument checks with their messages, and the ctypes plumbing of a call on a PolicyActor's networks.
`who` is the class a message names: every error reads "<who>: <message>"."""
import ctypes as C

import torch

from . import _lib


def bad(who):
    """the error maker of a class: bad("PolicyActor")(msg) is TsidbError("PolicyActor: " + msg)"""
    return lambda msg: _lib.TsidbError(who + ": " + msg)


def number(who, name, x, lo=None, strict=False):
    """x as a float: a finite number, >= lo (strict: > lo)"""
    if isinstance(x, bool) or not isinstance(x, (int, float)) or x != x or x in (float("inf"), float("-inf")):
        raise bad(who)(f"{name} must be a finite number, got {x!r}")
    if lo is not None and (x <= lo if strict else x < lo):
        raise bad(who)(f"{name} must be {'>' if strict else '>='} {lo}, got {x!r}")
    return float(x)


def count(who, name, x):
    if isinstance(x, bool) or not isinstance(x, int) or x < 1:
        raise bad(who)(f"{name} must be a whole number >= 1, got {x!r}")
    return x


def flag(who, name, x):
    if not isinstance(x, bool):
        raise bad(who)(f"{name} must be a bool, got {x!r}")
    return x


def device_tensor(who, what, t, shape, dtype, device):
    """t, a contiguous tensor of that dtype on that device; shape: a tuple with None where any size goes, or None = any shape.
    what: the message, or a function that makes it (where it says what was got instead)"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != device or not t.is_contiguous() or (shape is not None and (
            t.dim() != len(shape) or any(want is not None and want != got for want, got in zip(shape, t.shape)))):
        raise bad(who)(what() if callable(what) else what)
    return t


def ptr(t):
    """a tensor's address as a call's argument or a struct's field takes it, None (NULL) for None"""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def net_refs(actor):
    """(byref of the actor's tsidb_policy_net, byref of the critic's or None) of a PolicyActor"""
    return C.byref(actor.actor_net.struct), C.byref(actor.critic_net.struct) if actor.critic_net is not None else None


def grown_workspace(owner, wc, query, actor, M, dtype):
    """owner.workspace, grown to what the library's `query` entry asks for M rows if M is the most seen (owner._ws_rows;
    owner._ws_bytes: the bytes asked for)"""
    if owner.workspace is None or M > owner._ws_rows:
        n, item = C.c_size_t(0), torch.finfo(dtype).bits // 8
        wc._call(query, *net_refs(actor), M, C.byref(n))
        owner.workspace = torch.empty(max(1, (n.value + item - 1) // item), dtype=dtype, device=wc.device)
        owner._ws_rows, owner._ws_bytes = M, n.value
    return owner.workspace
