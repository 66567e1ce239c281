"""PolicySymmetry - the left / right mirror of a PolicyEnv's robot as signed permutations of the rows a PolicyActor reads and of
its action (rsl_rl's symmetry_cfg: data augmentation and the mirror loss; PolicyLearner(symmetry=...), include/tsidb.h
tsidb_policy_learn_sym).  No reference counterpart (the reference's only controller is TSID, main.py:113-129).

A mirror map of a row is mirror(x)[c] = sign[c] * x[perm[c]], an involution: perm[perm[c]] == c and sign[perm[c]] == sign[c].
With n the mirror normal in the base frame and M = I - 2 n n^T, a polar vector (a velocity, a position error, gravity) maps to
M v, an axial one (an angular velocity, a hinge axis) to -M w.  Everything is derived from the model blob's sim tree at the zero
pose and from the env's configuration: no joint names, no files.

The actuator table: all hinges turn about their body's local z.  n is the base axis about which the tree pairs best; the partner
of a body is the body of equal depth whose origin is nearest the reflected origin and whose axis is parallel to the reflected
axis; the sign is s = -(M z_b) . z_b' - a rotation about a reflected axis is seen reversed.
"""
import numpy as np
import torch

from . import _lib
from ._policy_util import bad
from .policy_actor import PolicyActor

_bad = bad("PolicySymmetry")


def _quat_mat(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def body_frames(model):
    """(origin [NB, 3], hinge axis [NB, 3], depth [NB]) of the sim tree at the zero pose in the base frame (body 0 at the
    origin with the identity rotation)"""
    par = np.asarray(model["mj_parent"], dtype=np.int64)
    nb = len(par)
    pos, quat = np.asarray(model["mj_pos"], dtype=np.float64).reshape(nb, 3), np.asarray(model["mj_quat"], dtype=np.float64).reshape(nb, 4)
    R, p, depth = [np.eye(3)] * nb, np.zeros((nb, 3)), np.zeros(nb, dtype=np.int64)
    for b in range(1, nb):
        a = int(par[b])
        if not 0 <= a < b:
            raise _bad(f"mj_parent[{b}] = {a}: the tree must list a parent before its children")
        R[b], p[b], depth[b] = R[a] @ _quat_mat(quat[b]), p[a] + R[a] @ pos[b], depth[a] + 1
    return p, np.stack([r[:, 2] for r in R]), depth


def _pair_bodies(p, z, depth, n):
    """(partner [NB], sign [NB], cost) of the tree reflected about the plane of normal n through the base origin; partner -1
    where no body of equal depth has a parallel axis"""
    M = np.eye(3) - 2.0 * np.outer(n, n)
    nb = len(p)
    partner, sign, cost = np.full(nb, -1, dtype=np.int64), np.zeros(nb), 0.0
    for b in range(1, nb):
        best = None
        for c in range(1, nb):
            s = -float((M @ z[b]) @ z[c])
            if depth[c] != depth[b] or abs(s) <= 0.99:
                continue
            d = float(np.linalg.norm(M @ p[b] - p[c]))
            if best is None or d < best[0]:
                best = (d, c, s)
        if best is None:
            cost += 1e9
            continue
        cost += best[0]
        partner[b], sign[b] = best[1], 1.0 if best[2] > 0 else -1.0
    return partner, sign, cost


def actuator_table(model):
    """(perm int32 [NA], sign float32 [NA], n [3]) of the actuators of a model blob (mj_parent, mj_pos, mj_quat, mj_act_dof)"""
    p, z, depth = body_frames(model)
    tries = [(_pair_bodies(p, z, depth, n), n) for n in np.eye(3)]
    (partner, bsign, cost), n = min(tries, key=lambda t: t[0][2])
    if np.any(partner[1:] < 0):                       # (a robot is symmetric to a few cm only - a head camera, a battery: the test
        raise _bad("the sim tree is symmetric about none of the base axes: a body has no partner")   # is the involution below)
    dof = np.asarray(model["mj_act_dof"], dtype=np.int64)
    body = dof - 5                                    # (the free joint takes dofs 0 .. 5; body b >= 1 has the hinge dof 5 + b)
    of_body = {int(b): a for a, b in enumerate(body)}
    perm, sign = np.zeros(len(dof), dtype=np.int32), np.zeros(len(dof), dtype=np.float32)
    for a, b in enumerate(body):
        c = int(partner[b])
        if c < 0 or c not in of_body:
            raise _bad(f"actuator {a} (body {int(b)}) has no mirrored actuator")
        perm[a], sign[a] = of_body[c], bsign[b]
    check_involution(perm, sign, "the actuator pairing")
    return perm, sign, n


def check_involution(perm, sign, what):
    perm, sign = np.asarray(perm), np.asarray(sign)
    k = len(perm)
    if perm.shape != (k,) or sign.shape != (k,) or k < 1 or not np.issubdtype(perm.dtype, np.integer):
        raise _bad(f"{what}: perm must be [k] whole numbers and sign [k], got shapes {perm.shape} and {sign.shape}")
    if perm.min() < 0 or perm.max() >= k:
        raise _bad(f"{what}: perm must stay inside its block of {k} columns")
    if not np.all(np.abs(sign) == 1.0):
        raise _bad(f"{what}: sign must be +1 or -1")
    if not (np.array_equal(perm[perm], np.arange(k)) and np.array_equal(sign[perm], sign)):
        raise _bad(f"{what} is not an involution (perm[perm[c]] == c and sign[perm[c]] == sign[c])")


def _vec(n, axial=False):
    """the table of a 3-vector: a reflection about a base axis permutes nothing and flips one component (polar) or the two
    others (axial)"""
    d = 1.0 - 2.0 * n * n
    return np.arange(3), -d if axial else d


def _cat(*tables):
    perm, sign, off = [], [], 0
    for p, s in tables:
        perm.append(np.asarray(p, dtype=np.int64) + off)
        sign.append(np.asarray(s, dtype=np.float64))
        off += len(p)
    return np.concatenate(perm), np.concatenate(sign)


def command_table(n):
    """(vx, vy) is polar, the yaw rate the z of an axial vector"""
    pol, ax = _vec(n), _vec(n, axial=True)
    return np.arange(3), np.array([pol[1][0], pol[1][1], ax[1][2]])


def obs_table(n, act):
    """include/tsidb.h tsidb_policy_obs: angular velocity, projected gravity, command, joint position, joint velocity, last action,
    the contact flags LF, RF"""
    return _cat(_vec(n, axial=True), _vec(n), command_table(n), act, act, act, ([1, 0], [1.0, 1.0]))


def priv_table(n):
    """base linear velocity (body frame), base height, and the columns up to TSIDB_POL_NPRIV"""
    rest = _lib.POL_NPRIV - 3
    return _cat(_vec(n), (np.arange(rest), np.ones(rest)))


def teacher_obs_table(n, act):
    """include/tsidb.h tsidb_policy_teacher_obs: contact_active of the two feet, CoM error, CoM velocity, the two foot errors, tau"""
    pol = _vec(n)
    feet = (np.array([3, 4, 5, 0, 1, 2]), np.concatenate([pol[1], pol[1]]))
    return _cat(([1, 0], [1.0, 1.0]), pol, pol, feet, act)


def height_scan_table(n, ter):
    """point p = ix * ny + iy of the grid (include/tsidb.h tsidb_policy_height_scan): the index along n reverses"""
    nx, ny = int(ter[_lib.POL_TER_SCAN_NX]), int(ter[_lib.POL_TER_SCAN_NY])
    axis = int(np.argmax(np.abs(n)))
    if axis == 2:
        raise _bad("height_scan: the mirror normal is the base z axis, the scan grid has no such direction")
    lo, hi = (ter[_lib.POL_TER_SCAN_X0], ter[_lib.POL_TER_SCAN_X1]) if axis == 0 else (ter[_lib.POL_TER_SCAN_Y0], ter[_lib.POL_TER_SCAN_Y1])
    count = nx if axis == 0 else ny
    if (count > 1 and lo != -hi) or (count == 1 and lo != 0.0):
        raise _bad(f"height_scan: the grid must be symmetric about 0 along the mirror normal, got {lo} .. {hi}")
    ix, iy = np.divmod(np.arange(nx * ny), ny)
    perm = (nx - 1 - ix) * ny + iy if axis == 0 else ix * ny + (ny - 1 - iy)
    return perm, np.ones(nx * ny)


def _slice(table, lo, hi, what):
    perm, sign = table
    inside = perm[lo:hi]
    if inside.min() < lo or inside.max() >= hi:
        raise _bad(f"{what}: the column range ({lo}, {hi}) is not closed under the mirror (column "
                   f"{lo + int(np.argmax((inside < lo) | (inside >= hi)))} pairs with one outside it)")
    return inside - lo, sign[lo:hi]


class PolicySymmetry:
    """env, actor: the PolicyEnv and its PolicyActor.  blocks: {i: (perm, sign)} for input block i of the actor, or
    {("actor" | "critic", i): (perm, sign)}, for every block given as a raw [N, k] tensor - a named block's table is derived.

    Tensors on the env's device: action_perm, actor_perm, critic_perm (int32; critic_* None without a critic), action_sign,
    actor_sign, critic_sign (float32).  normal: the mirror normal in the base frame."""

    def __init__(self, env, actor, blocks=None):
        if not isinstance(actor, PolicyActor) or actor.env is not env:
            raise _bad("actor must be a PolicyActor of env")
        if actor.normalizer is not None:
            raise _bad("an actor with a PolicyNormalizer is not supported: the storage holds normalised rows, and a mirror in "
                       "normalised coordinates is the robot's only if the statistics are symmetric themselves")
        self.env, self.actor = env, actor
        perm, sign, self.normal = actuator_table(env.wc.model)
        if len(perm) != env.NA:
            raise _bad(f"the model has {len(perm)} actuators, the env {env.NA}")
        self._act = (perm.astype(np.int64), sign.astype(np.float64))
        blocks = dict(blocks or {})
        dev = env.wc.device
        dev_pair = lambda t: (torch.as_tensor(t[0], dtype=torch.int32, device=dev), torch.as_tensor(t[1], dtype=torch.float32, device=dev))
        self.action_perm, self.action_sign = dev_pair(self._act)
        self.actor_perm, self.actor_sign = dev_pair(self._net_table("actor", actor.actor_net, blocks))
        self.critic_perm = self.critic_sign = None
        if actor.critic_net is not None:
            self.critic_perm, self.critic_sign = dev_pair(self._net_table("critic", actor.critic_net, blocks))

    def named_table(self, name):
        """(perm, sign) of one of the env's named tensors"""
        env, n, act = self.env, self.normal, self._act
        if name == "obs":
            return obs_table(n, act)
        if name == "priv":
            return priv_table(n)
        if name == "command":
            return command_table(n)
        if name == "teacher_obs":
            return teacher_obs_table(n, act)
        if name == "height_scan":
            ter = getattr(env, "ter_params", None)
            if ter is None:
                raise _bad("height_scan: the env has no terrain")
            return height_scan_table(n, ter)
        if name == "obs_history":
            spec, sources = getattr(env, "obs_history_spec", None), getattr(env, "obs_history_sources", None)
            if spec is None or sources is None:
                raise _bad("obs_history: the env has no observation history")
            frame = _cat(*(_slice(self.named_table(src), lo, hi, f"obs_history source {src}") for src, lo, hi in sources))
            return _cat(*([frame] * int(spec.frames)))
        raise _bad(f"unknown input {name!r}")

    def _net_table(self, which, net, blocks):
        tables = []
        for i, (t, name) in enumerate(zip(net.blocks, net.block_names)):
            k = int(t.shape[1])
            if name is None:
                given = blocks.get((which, i), blocks.get(i))
                if given is None:
                    raise _bad(f"{which} input block {i} is a raw [N, {k}] tensor: give its table as blocks={{{i}: (perm, sign)}}")
                table = (np.asarray(given[0]), np.asarray(given[1], dtype=np.float64))
            else:
                table = self.named_table(name)
            check_involution(table[0], table[1], f"{which} input block {i}" + (f" ({name})" if name else ""))
            if len(table[0]) != k:
                raise _bad(f"{which} input block {i}: a table of {len(table[0])} columns for a block of {k}")
            tables.append(table)
        return _cat(*tables)

    def _table(self, which):
        if which == "actor":
            return self.actor_perm, self.actor_sign
        if which == "critic" and self.critic_perm is not None:
            return self.critic_perm, self.critic_sign
        raise _bad(f"which must be 'actor'{' or critic' if self.critic_perm is not None else ''}, got {which!r}")

    @staticmethod
    def _apply(x, perm, sign):
        if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.shape[-1] != perm.shape[0]:
            raise _bad(f"a row of {perm.shape[0]} columns is expected, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
        return x.index_select(-1, perm.to(device=x.device, dtype=torch.int64)) * sign.to(device=x.device, dtype=x.dtype)

    def mirror_obs(self, x, which="actor"):
        """the mirrored input rows of a network: x [..., K] -> sign * x[..., perm], a new tensor"""
        return self._apply(x, *self._table(which))

    def mirror_action(self, a):
        """the mirrored actions: a [..., NA] -> sign * a[..., perm], a new tensor"""
        return self._apply(a, self.action_perm, self.action_sign)
