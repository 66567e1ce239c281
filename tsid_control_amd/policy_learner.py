"""PolicyLearner - the loss and the gradients of a PPO update on the device (include/tsidb.h tsidb_policy_learn;
csrc/tsidb_learner.hpp): the clipped surrogate, the clipped value loss and the entropy bonus of rsl_rl's PPO on one minibatch
of a RolloutStorage, and the gradient of every weight and bias of the PolicyActor's two networks and of log_std, written into
their .grad.  The forward pass is the actor kernel's own, so the recomputed log-probability is the stored one's twin.  No
reference counterpart (the reference's only controller is TSID, main.py:113-129).

What stays the caller's unless PolicyOptimizer is used (policy_optimizer.py: gradient clipping, Adam and rsl_rl's adaptive step
size in three launches): the optimiser (any torch.optim over the same tensors: its step is what the next act() and the next
backward() compute with, nothing is copied), gradient clipping, schedules.  What stays the caller's: all-reduces, observation
normalisation (PolicyNormalizer) - all work on .grad as they do after loss.backward().  .grad is OVERWRITTEN by every
backward(), never accumulated.

No parameter needs requires_grad, log_std included: backward() gives every parameter that has none a zero float32 .grad of
its own, reads the pointers again at every call (zero_grad(set_to_none=True) is harmless), and torch's optimisers step every
parameter that has a .grad.  A .grad the caller set is used as it is if it is float32, contiguous and on the device.
"""
import ctypes as C
from functools import partial

import torch

from . import _lib
from ._policy_util import bad, count, device_tensor, flag, grown_workspace, net_refs, number, ptr
from .policy_actor import PolicyActor, RolloutStorage

_WHO = "PolicyLearner"
_bad, _number, _count, _flag, _tensor = bad(_WHO), partial(number, _WHO), partial(count, _WHO), partial(flag, _WHO), partial(device_tensor, _WHO)


class PolicyLearner:
    """actor: the PolicyActor whose networks and log_std are learned.  clip: the surrogate's and the value loss's range (> 0);
    value_coef, entropy_coef (>= 0): loss = L_pi + value_coef L_v - entropy_coef entropy; value_clip: the clipped value loss
    (False: the plain squared error); normalize_advantage: advantages minus their mean, over their std + 1e-8, of the whole
    storage.  imitation_coef (>= 0), imitation_loss ("mse" or "huber", delta 1): a term imitation_coef L_im on the distance of the
    actor's mean from the storage's teacher labels (a RolloutStorage built with teacher = True; include/tsidb.h
    tsidb_policy_learn_imit), weighted by teacher_weight, with the surrogate kept off the rows the env executed the teacher's
    action on (teacher_executed); surrogate_coef (>= 0) scales L_pi - loss = surrogate_coef L_pi + value_coef L_v - entropy_coef
    entropy + imitation_coef L_im, so surrogate_coef = value_coef = entropy_coef = 0 is pure distillation (rsl_rl's Distillation)
    and the defaults are PPO as it is, with the calls it made before the term existed.  imit_stats [4] float32
    (_lib.POL_IMIT_STATS): L_im, the sum of the weights, the rows with a weight, the rows whose surrogate was skipped.
    symmetry: a PolicySymmetry of the actor (policy_symmetry.py; None = none, the calls and the bits as ever) - backward() goes
    through tsidb_policy_learn_sym (include/tsidb.h).  symmetry_augment: every row also counts as its mirror image (rsl_rl's
    use_data_augmentation); mirror_coef (>= 0): the weight of L_sym = mean |mu(S_o x) - S_a mu(x)|^2 (rsl_rl's mirror loss).
    sym_stats [2] float32 (_lib.POL_SYM_STATS): L_sym - formed at mirror_coef = 0 too - and the mirrored rows used.  Not with
    the imitation term.

    Tensors: stats [8] float32, written by backward() - policy_loss, value_loss, entropy, approx_kl, clip_fraction, loss, rows,
    bad_indices (_lib.POL_LEARN_STATS); adv_stats [2] (mean, 1 / std); workspace (grown to the largest minibatch seen)."""

    def __init__(self, actor, clip=0.2, value_coef=1.0, entropy_coef=0.0, value_clip=True, normalize_advantage=True, imitation_coef=0.0,
                 imitation_loss="mse", surrogate_coef=1.0, symmetry=None, symmetry_augment=True, mirror_coef=0.0):
        if not isinstance(actor, PolicyActor):
            raise _bad(f"actor must be a PolicyActor, got {type(actor).__name__}")
        self.actor, self.env = actor, actor.env
        self.clip = _number("clip", clip, 0.0, strict=True)
        self.value_coef, self.entropy_coef = _number("value_coef", value_coef, 0.0), _number("entropy_coef", entropy_coef, 0.0)
        self.value_clip, self.normalize_advantage = _flag("value_clip", value_clip), _flag("normalize_advantage", normalize_advantage)
        self.imitation_coef, self.surrogate_coef = _number("imitation_coef", imitation_coef, 0.0), _number("surrogate_coef", surrogate_coef, 0.0)
        if imitation_loss not in _lib.POL_IMIT_LOSSES:
            raise _bad(f"imitation_loss must be one of {_lib.POL_IMIT_LOSSES}, got {imitation_loss!r}")
        self.imitation_loss = imitation_loss
        self.symmetry, self.mirror_coef = symmetry, _number("mirror_coef", mirror_coef, 0.0)
        self.symmetry_augment = _flag("symmetry_augment", symmetry_augment)
        if symmetry is not None:
            self._check_symmetry(symmetry)
        elif self.mirror_coef != 0.0:
            raise _bad("mirror_coef needs a symmetry")
        dev = self.env.wc.device
        self.stats = torch.zeros(len(_lib.POL_LEARN_STATS), dtype=torch.float32, device=dev)
        self.adv_stats = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)
        self.imit_stats = torch.zeros(len(_lib.POL_IMIT_STATS), dtype=torch.float32, device=dev)
        self.sym_stats = torch.zeros(len(_lib.POL_SYM_STATS), dtype=torch.float32, device=dev) if symmetry is not None else None
        self.workspace, self._ws_rows = None, 0
        self._cfg = _lib.PolicyLearnCfg(self.clip, self.value_coef, self.entropy_coef, int(value_clip))

    def _check_symmetry(self, sym):
        """the tables before they reach the library: of this actor, on the device, every perm inside its row"""
        from .policy_symmetry import PolicySymmetry
        a, dev = self.actor, self.env.wc.device
        if not isinstance(sym, PolicySymmetry) or sym.actor is not a:
            raise _bad("symmetry must be a PolicySymmetry of this learner's actor")
        if self._imit_on:
            raise _bad("a symmetry with the imitation term (imitation_coef != 0 or surrogate_coef != 1) is not supported")
        if a.normalizer is not None:
            raise _bad("a symmetry with a PolicyNormalizer is not supported")
        sizes = [("actor", sym.actor_perm, sym.actor_sign, a.actor_net.K), ("action", sym.action_perm, sym.action_sign, self.env.NA)]
        if a.critic_net is not None:
            sizes.append(("critic", sym.critic_perm, sym.critic_sign, a.critic_net.K))
        for name, perm, sign, k in sizes:
            for t, dt in ((perm, torch.int32), (sign, torch.float32)):
                _tensor(f"symmetry: the {name} table must be contiguous [{k}] int32 and float32 tensors on {dev}", t, (k,), dt, dev)
            if int(perm.min()) < 0 or int(perm.max()) >= k:
                raise _bad(f"symmetry: the {name} perm must stay inside [0, {k})")

    @property
    def _imit_on(self):
        """anything but PPO as it is: backward() goes through tsidb_policy_learn_imit"""
        return self.imitation_coef != 0.0 or self.surrogate_coef != 1.0

    def parameters(self):
        """every tensor backward() writes a .grad of: the weights and biases of the actor, of the critic, and log_std - what an
        optimiser is built over"""
        nets = [self.actor.actor_net] + ([self.actor.critic_net] if self.actor.critic_net is not None else [])
        return [t for net in nets for w, b in net.layers for t in (w, b) if t is not None] + [self.actor.log_std]

    def _grad(self, p):
        g = p.grad
        if g is None:
            p.grad = g = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
        return _tensor(lambda: f"a .grad must be a contiguous float32 tensor of its parameter's shape on {p.device}, got "
                             f"{(tuple(g.shape), g.dtype, g.device, g.stride())}", g, tuple(p.shape), torch.float32, p.device)

    def _grads_of(self, net):
        s = _lib.PolicyGrads()
        for i, (w, b) in enumerate(net.layers):
            s.weight[i] = self._grad(w).data_ptr()
            s.bias[i] = self._grad(b).data_ptr() if b is not None else None
        return s

    def _variant(self):
        """(workspace query, entry, maker of the entry's extra struct or None) of this learner's backward()"""
        if self.symmetry is not None:
            return "tsidb_policy_learn_sym_workspace", "tsidb_policy_learn_sym", self._sym_struct
        if self._imit_on:
            return "tsidb_policy_learn_imit_workspace", "tsidb_policy_learn_imit", self._imit_struct
        return "tsidb_policy_learn_workspace", "tsidb_policy_learn", None

    def _sym_struct(self, storage):
        sy = self.symmetry
        self._last_sym = _lib.PolicySymmetryTables(ptr(sy.actor_perm), ptr(sy.actor_sign), ptr(sy.critic_perm), ptr(sy.critic_sign),
                                                   ptr(sy.action_perm), ptr(sy.action_sign), int(self.symmetry_augment), self.mirror_coef,
                                                   ptr(self.sym_stats))
        return self._last_sym              # (alive until the next call, as the batch)

    def _imit_struct(self, storage):
        self._last_imit = _lib.PolicyImit(ptr(storage.teacher_action), ptr(storage.teacher_weight), ptr(storage.teacher_executed),
                                          self.imitation_coef, self.surrogate_coef, _lib.POL_IMIT_LOSSES.index(self.imitation_loss),
                                          ptr(self.imit_stats))
        return self._last_imit             # (alive until the next call, as the batch)

    def fill_adv_stats(self, storage):
        """adv_stats = (mean, 1 / (std + 1e-8)) of storage.advantage, with torch ops on the current stream: no host sync"""
        adv = storage.advantage
        torch.stack([adv.mean(), 1.0 / (adv.std() + 1e-8)], out=self.adv_stats)

    def backward(self, storage, index, stats=None, adv_stats=None):
        """The loss of the stored rows index [M] (int32, on the device; any order, duplicates allowed, flat t * N + e into the
        first T * N rows) and its gradients into .grad, in three launches on the current stream.  Returns stats ([8] float32:
        self.stats, or the tensor given).  adv_stats: None = self.adv_stats, filled from this storage by this call when
        normalize_advantage is set; update() fills it once and passes it."""
        wc, a = self.env.wc, self.actor
        if not isinstance(storage, RolloutStorage) or storage.actor is not a:
            raise _bad("storage must be a RolloutStorage of this learner's actor")
        if storage.advantage is None:
            raise _bad("storage.gae() has not run: there are no advantages and returns")
        if self.imitation_coef > 0 and storage.teacher_action is None:
            raise _bad("imitation_coef > 0 needs a storage with the teacher's labels (RolloutStorage(..., teacher=True))")
        got = lambda: (tuple(index.shape), index.dtype, index.device) if isinstance(index, torch.Tensor) else type(index).__name__
        bad_index = lambda: f"index must be a contiguous [M >= 1] int32 tensor on {wc.device}, got {got()}"
        if _tensor(bad_index, index, (None,), torch.int32, wc.device).shape[0] < 1:
            raise _bad(bad_index())
        if stats is None:
            stats = self.stats
        else:
            _tensor(f"stats must be a contiguous [{len(_lib.POL_LEARN_STATS)}] float32 tensor on {wc.device}", stats, (len(_lib.POL_LEARN_STATS),),
                    torch.float32, wc.device)
        if adv_stats is None and self.normalize_advantage:
            self.fill_adv_stats(storage)
        M = int(index.shape[0])
        query, entry, extra = self._variant()
        ws = grown_workspace(self, wc, query, a, M, torch.float32)
        batch = _lib.PolicyLearnBatch(*(ptr(t) for t in (storage.actor_input, storage.critic_input, storage.action, storage.logp, storage.value,
                                                         storage.advantage, storage.returns, index)), storage.steps * self.env.num_envs, M,
                                      ptr(self.adv_stats) if self.normalize_advantage else None)
        ag = self._grads_of(a.actor_net)
        cg = self._grads_of(a.critic_net) if a.critic_net is not None else None
        self._last = (batch, ag, cg)       # (alive until the next call: the library copies them during the call, a recorder may look later)
        self._last_storage, self._last_index = storage, index    # (what a PolicyOptimizer's KL is taken over)
        wc._call(entry, *net_refs(a), C.byref(batch), C.byref(ag), C.byref(cg) if cg is not None else None, ptr(a.log_std),
                 C.c_void_p(self._grad(a.log_std).data_ptr()), C.byref(self._cfg), *((C.byref(extra(storage)),) if extra is not None else ()),
                 ptr(ws), C.c_size_t(ws.numel() * 4), ptr(stats), wc._stream())
        return stats

    def outputs(self, M):
        """(mu [M, NA], v [M] or None): the actor's and the critic's outputs on the rows of the last backward() of M rows, views
        of the workspace (include/tsidb.h: its first floats; with a symmetry the arrays hold 2 Mp rows, the originals first)"""
        Mp, NA = (M + 15) // 16 * 16, self.env.NA
        mu = self.workspace[:Mp * NA].view(Mp, NA)[:M]
        v0 = (2 * Mp if self.symmetry is not None else Mp) * NA
        return mu, (self.workspace[v0:v0 + M] if self.actor.critic_net is not None else None)

    def update(self, storage, optimizer, epochs=5, minibatches=4, generator=None):
        """One PPO update on a storage whose gae() has run: per epoch a torch.randperm(T * N) on the device (generator: a
        torch.Generator of the device, None = the default one), cut into `minibatches` slices; per slice backward() and
        optimizer.step().  An optimizer with a snapshot() method (PolicyOptimizer: the rollout's log_std, for its KL) has it called
        once, first.  Returns the stats of every slice, [epochs * minibatches, 8]; no host sync anywhere."""
        wc = self.env.wc
        epochs, minibatches = _count("epochs", epochs), _count("minibatches", minibatches)
        if not isinstance(storage, RolloutStorage) or storage.advantage is None:
            raise _bad("update needs a RolloutStorage whose gae() has run")
        rows = storage.steps * self.env.num_envs
        if minibatches > rows:
            raise _bad(f"{minibatches} minibatches of {rows} stored rows")
        if self.normalize_advantage:
            self.fill_adv_stats(storage)
        out = torch.zeros(epochs * minibatches, len(_lib.POL_LEARN_STATS), dtype=torch.float32, device=wc.device)
        if hasattr(optimizer, "snapshot"):
            optimizer.snapshot()
        for ep in range(epochs):
            perm = torch.randperm(rows, generator=generator, dtype=torch.int32, device=wc.device)
            for k in range(minibatches):
                self.backward(storage, perm[k * rows // minibatches:(k + 1) * rows // minibatches], stats=out[ep * minibatches + k],
                              adv_stats=self.adv_stats)
                optimizer.step()
        return out

    def written(self):
        """the tensors backward() writes: what a caller that captures it in a graph keeps alive (imit_stats while the imitation
        term or a surrogate_coef is on: the plain call does not write it)"""
        return [self._grad(p) for p in self.parameters()] + [self.stats, self.adv_stats] + ([self.imit_stats] if self._imit_on else []) + ([self.sym_stats] if self.symmetry is not None else []) + ([self.workspace] if self.workspace is not None else [])
