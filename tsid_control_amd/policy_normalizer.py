"""PolicyNormalizer - rsl_rl's EmpiricalNormalization (empirical_normalization = True) for a PolicyActor: running mean and
variance of each network's input row, kept on the device by tsidb_policy_norm_update (include/tsidb.h; csrc/tsidb_norm.hpp:
float64, no atomics, one fixed order, two launches) and applied by the actor's own launch as it loads the env's tensors
(tsidb_policy_actor_norm: (x - mean) / (std + eps) as one float32 subtraction and one float32 product, then the clamp).  What
the actor stores - PolicyActor.actor_input, RolloutStorage.actor_input and their critic twins - are the normalised rows, as in
rsl_rl, so PolicyLearner recomputes the actor's outputs from them bit for bit and knows nothing of the normaliser.

Order, rsl_rl's: in training mode act() and every step of PolicyEnv.rollout first update the statistics with the current
observation and then evaluate with the updated ones; the rollout's closing value launch normalises with the current statistics
and does not update - that observation is counted by the next rollout's first step, so every observation enters once.

Not done here: a non-finite input poisons the statistics, as in rsl_rl - there is no masking.  The statistics are per process: a
batch split over ranks is not split-invariant, a rank merge belongs with a future all-reduce.  A variant that folds the partial
sums into the actor launch and normalises with the previous step's statistics would save a launch but departs from rsl_rl's
order; it is not built.
"""
import ctypes as C

import torch

from . import _lib
from ._policy_util import bad, flag, net_refs, number, ptr

_NETS = (("actor", "obs_normalizer"), ("critic", "critic_obs_normalizer"))
_bad = bad("PolicyNormalizer")


class _State:
    """one network's state: stats [2, K] float64 (mean, variance), count [1] int64, affine [2, K] float32 (shift, scale), and
    the tsidb_policy_norm struct over them"""

    def __init__(self, K, device, eps, clip, until):
        self.K, self.eps = K, eps
        self.stats = torch.zeros(2, K, dtype=torch.float64, device=device)
        self.stats[1] = 1.0
        self.count = torch.zeros(1, dtype=torch.int64, device=device)
        self.affine = torch.zeros(2, K, dtype=torch.float32, device=device)
        self.fill_affine()
        self.struct = _lib.PolicyNorm(self.affine.data_ptr(), clip or 0.0, self.stats.data_ptr(), self.count.data_ptr(), eps, until or 0)

    def fill_affine(self):
        """affine from stats, with torch ops on the device: shift = (float)mean, scale = (float)(1 / (sqrt(var) + eps))"""
        self.affine[0].copy_(self.stats[0])
        self.affine[1].copy_(1.0 / (torch.sqrt(self.stats[1]) + self.eps))

    def tensors(self):
        return [self.stats, self.count, self.affine]


class PolicyNormalizer:
    """PolicyActor(..., normalizer=PolicyNormalizer(...)).  eps: std + eps divides (> 0; rsl_rl's 1e-2).  clip: the normalised
    values are clamped to +-clip (> 0; None = no clamp).  until: a whole number >= 1 - once a network's count has reached it an
    update changes nothing (the count is compared on the device, no host read; None = no limit).  critic: False leaves the
    critic's rows raw and keeps no state for it.

    Tensors, once the actor is built, per network (actor, critic): stats [2, K] float64 (running mean, running variance; 0 and 1
    at first), count [1] int64, affine [2, K] float32 (shift, scale: all the actor's launch reads); workspace."""

    def __init__(self, eps=1e-2, clip=None, until=None, critic=True):
        self.eps = number("PolicyNormalizer", "eps", eps, 0, strict=True)
        self.clip = None if clip is None else number("PolicyNormalizer", "clip", clip, 0, strict=True)
        if until is not None and (isinstance(until, bool) or not isinstance(until, int) or until < 1):
            raise _bad(f"until must be a whole number >= 1 or None, got {until!r}")
        self.until = until
        self.with_critic = flag("PolicyNormalizer", "critic", critic)
        self.training = True
        self.policy = None
        self.actor = self.critic = self.workspace = None

    def _attach(self, policy):
        """called by PolicyActor's constructor: allocates the state for its networks on the env's device"""
        if self.policy is not None:
            raise _bad("this normaliser already belongs to a PolicyActor (its state has that actor's columns): build one per actor")
        wc = policy.env.wc
        self.policy = policy
        self.actor = _State(policy.actor_net.K, wc.device, self.eps, self.clip, self.until)
        if policy.critic_net is not None and self.with_critic:
            self.critic = _State(policy.critic_net.K, wc.device, self.eps, self.clip, self.until)
        nseg = (policy.env.num_envs + _lib.POL_NORM_SEG_ROWS - 1) // _lib.POL_NORM_SEG_ROWS
        self.workspace = torch.zeros(nseg * 2 * sum(s.K for s in self._states()), dtype=torch.float64, device=wc.device)

    def _states(self):
        return [s for s in (self.actor, self.critic) if s is not None]

    def _need(self):
        if self.policy is None:
            raise _bad("not attached: pass it to PolicyActor(..., normalizer=...) first")

    def train(self, mode=True):
        """act() and rollout() update the statistics before they evaluate (the default)"""
        self.training = flag("PolicyNormalizer", "mode", mode)
        return self

    def eval(self):
        """act() and rollout() normalise with the statistics as they are"""
        return self.train(False)

    def update(self):
        """one tsidb_policy_norm_update call on the env's current tensors (two launches on the current stream, both networks in
        each): the N rows enter each network's statistics and its affine pair is rewritten"""
        self._need()
        wc = self.policy.env.wc
        a, c = net_refs(self.policy)
        wc._call("tsidb_policy_norm_update", a, c if self.critic is not None else None,
                 C.byref(self.actor.struct), C.byref(self.critic.struct) if self.critic is not None else None,
                 ptr(self.workspace), C.c_size_t(self.workspace.numel() * 8), wc._stream())

    def written(self):
        """stats, count, affine of each network and the workspace: what update() writes"""
        self._need()
        return [t for s in self._states() for t in s.tensors()] + [self.workspace]

    def state_dict(self):
        """{"obs_normalizer": {...}, "critic_obs_normalizer": {...}} (the critic's only where it has a state), each with rsl_rl's
        EmpiricalNormalization buffers: _mean, _var, _std [1, K] (float64 here) and count (an int64 scalar) - clones"""
        self._need()
        out = {}
        for (attr, key) in _NETS:
            s = getattr(self, attr)
            if s is not None:
                out[key] = {"_mean": s.stats[0:1].clone(), "_var": s.stats[1:2].clone(), "_std": torch.sqrt(s.stats[1:2]),
                            "count": s.count[0].clone()}
        return out

    def load_state_dict(self, state):
        """the statistics of a state_dict() or of rsl_rl's normalisers (any float dtype, any device); affine is recomputed from
        them with torch ops on the device"""
        self._need()
        if not isinstance(state, dict):
            raise _bad(f"state must be a dict, got {type(state).__name__}")
        todo = []
        for (attr, key) in _NETS:
            s = getattr(self, attr)
            if s is None:
                continue
            d = state.get(key)
            if not isinstance(d, dict):
                raise _bad(f"state has no {key!r}")
            for name in ("_mean", "_var"):
                t = d.get(name)
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != (1, s.K) or not t.is_floating_point():
                    what = (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__
                    raise _bad(f"{key}: {name} must be a [1, {s.K}] float tensor (the {attr}'s input row has {s.K} columns), got {what}")
            if "_std" in d and (not isinstance(d["_std"], torch.Tensor) or tuple(d["_std"].shape) != (1, s.K)):
                raise _bad(f"{key}: _std must be a [1, {s.K}] tensor")
            c = d.get("count")
            if not isinstance(c, torch.Tensor) or c.numel() != 1 or c.is_floating_point() or c.dtype == torch.bool:
                raise _bad(f"{key}: count must be a whole-number tensor of one element")
            todo.append((s, d))
        for s, d in todo:
            s.stats[0].copy_(d["_mean"][0])
            s.stats[1].copy_(d["_var"][0])
            s.count.copy_(d["count"].reshape(1))
            s.fill_affine()
