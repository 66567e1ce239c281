"""PolicyOptimizer - what rsl_rl's PPO runs per minibatch behind the loss, on the device (include/tsidb.h tsidb_policy_opt_step;
csrc/tsidb_optim.hpp): torch's clip_grad_norm_ over every parameter of a PolicyLearner, torch.optim.Adam's default step on
them in place, and rsl_rl's adaptive step size (schedule = "adaptive") from the exact Gaussian KL between the rollout's policy
and the current one - three launches, no host read: lr lives on the device.  No reference counterpart (the reference's only
controller is TSID, main.py:113-129).

It drops into PolicyLearner.update(storage, optimizer) where a torch.optim optimiser goes: update() calls snapshot() once (the
rollout's log_std, for the KL) and step() after every backward().  The parameters are stepped in place, so the next act() and
the next backward() compute with the step; .grad is read, never written - the clip factor is applied inside the step.

Not built: weight decay, amsgrad; a rank all-reduce (all-reduce .grad before step(); the KL is this rank's); per-row sigma.
"""
import ctypes as C
from functools import partial

import torch

from . import _lib
from ._policy_util import bad, device_tensor, flag, grown_workspace, net_refs, number, ptr
from .policy_learner import PolicyLearner

_NSTATS = len(_lib.POL_OPT_STATS)
_bad, _number = bad("PolicyOptimizer"), partial(number, "PolicyOptimizer")


def _betas(betas):
    if not isinstance(betas, (tuple, list)) or len(betas) != 2:
        raise _bad(f"betas must be a pair, got {betas!r}")
    out = tuple(_number(f"betas[{i}]", b, 0.0) for i, b in enumerate(betas))
    for i, b in enumerate(out):
        if b >= 1.0:
            raise _bad(f"betas[{i}] must be < 1, got {b!r}")
    return out


class PolicyOptimizer:
    """learner: the PolicyLearner whose parameters() are stepped, in that order.  lr: the initial step size (> 0); betas (each in
    [0, 1)), eps (> 0): Adam's; max_grad_norm: clip_grad_norm_'s max_norm (>= 0; 0 or None = no clipping, the norm is still
    reported); desired_kl: None = a constant lr, > 0 = rsl_rl's adaptive rule inside [lr_min, lr_max] (0 < lr_min <= lr_max);
    skip_nonfinite: a step whose gradient norm (or KL) is not finite changes nothing and sets stats[5].

    Tensors: lr [1] float32, step_count [1] int64, stats [8] float32 written by step() (_lib.POL_OPT_STATS: grad_norm,
    clip_coef, kl, lr, step, skipped, kl_rows, lr_direction), log_std_old [NA] (snapshot()), moments [2, P] float32 with the
    views exp_avg(p) / exp_avg_sq(p), workspace.  log: None, or a [k, 8] float32 tensor the caller sets - the i-th step() after
    that writes row i instead of stats (a host counter; behind row k - 1 stats again)."""

    def __init__(self, learner, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0, desired_kl=None, lr_min=1e-5, lr_max=1e-2,
                 skip_nonfinite=True):
        if not isinstance(learner, PolicyLearner):
            raise _bad(f"learner must be a PolicyLearner, got {type(learner).__name__}")
        self.learner = learner
        lr = _number("lr", lr, 0.0, strict=True)
        self.betas, self.eps = _betas(betas), _number("eps", eps, 0.0, strict=True)
        self.max_grad_norm = 0.0 if max_grad_norm is None else _number("max_grad_norm", max_grad_norm, 0.0)
        self.desired_kl = None if desired_kl is None else _number("desired_kl", desired_kl, 0.0, strict=True)
        self.lr_min, self.lr_max = _number("lr_min", lr_min, 0.0, strict=True), _number("lr_max", lr_max, 0.0, strict=True)
        if self.lr_min > self.lr_max:
            raise _bad(f"lr_min must be <= lr_max, got {lr_min!r} and {lr_max!r}")
        self.skip_nonfinite = flag("PolicyOptimizer", "skip_nonfinite", skip_nonfinite)
        dev = learner.env.wc.device
        self._params = learner.parameters()
        self._offsets, n = [], 0
        for p in self._params:
            self._offsets.append(n)
            n += p.numel()
        self.P = n
        self.moments = torch.zeros(2, n, dtype=torch.float32, device=dev)
        self.lr = torch.full((1,), lr, dtype=torch.float32, device=dev)
        self.step_count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.stats = torch.zeros(_NSTATS, dtype=torch.float32, device=dev)
        self.log_std_old = learner.actor.log_std.detach().clone()
        self.workspace, self._ws_rows = None, -1
        self._log, self._log_i = None, 0
        self._cfg = self._make_cfg()

    def _make_cfg(self):
        return _lib.PolicyOptCfg(self.betas[0], self.betas[1], self.eps, self.max_grad_norm, self.desired_kl or 0.0, self.lr_min, self.lr_max,
                                 int(self.skip_nonfinite))

    # ---------------------------------------------------------------- tensors
    def parameters(self):
        return list(self._params)

    def _moment(self, which, p):
        for q, off in zip(self._params, self._offsets):
            if q is p:
                return self.moments[which, off:off + p.numel()].view(p.shape)
        raise _bad("not a parameter of this optimiser's learner")

    def exp_avg(self, p):
        """the first moment of parameter p: a view of moments"""
        return self._moment(0, p)

    def exp_avg_sq(self, p):
        """the second moment of parameter p: a view of moments"""
        return self._moment(1, p)

    @property
    def log(self):
        return self._log

    @log.setter
    def log(self, t):
        if t is not None:
            device_tensor("PolicyOptimizer", f"log must be None or a contiguous [k, {_NSTATS}] float32 tensor on {self.lr.device}", t,
                          (None, _NSTATS), torch.float32, self.lr.device)
        self._log, self._log_i = t, 0

    def written(self):
        """the tensors step() writes: what a caller that captures it in a graph keeps alive, and rewinds after its warm-up (the
        parameters detached: the same memory, writable in place whether or not they require grad)"""
        return [p.detach() for p in self._params] + [self.moments, self.lr, self.step_count, self.stats] + \
            ([self.workspace] if self.workspace is not None else []) + ([self._log] if self._log is not None else [])

    # ---------------------------------------------------------------- the step
    def snapshot(self):
        """log_std_old = log_std, a torch copy on the current stream: the rollout's policy, before the first step of an update()"""
        self.log_std_old.copy_(self.learner.actor.log_std)

    def step(self):
        """One step on the .grad tensors as they are now, in three launches on the current stream.  With desired_kl the KL is taken
        over the storage, the index and the workspace of the learner's last backward().  Returns stats (or the row of log)."""
        l = self.learner
        a, wc = l.actor, l.env.wc
        if getattr(l, "_last", None) is None:
            raise _bad("no backward() has run: there are no gradients (and no minibatch for the KL)")
        ag = l._grads_of(a.actor_net)
        cg = l._grads_of(a.critic_net) if a.critic_net is not None else None
        kl, M = None, 0
        if self.desired_kl is not None:
            storage, index = l._last_storage, l._last_index
            M = int(index.shape[0])
            kl = _lib.PolicyOptKl(l.workspace.data_ptr(), storage.mean.data_ptr(), index.data_ptr(), storage.steps * l.env.num_envs, M)
        ws = grown_workspace(self, wc, "tsidb_policy_opt_workspace", a, M, torch.float64)
        self._last_M = M
        stats = self.stats
        if self._log is not None and self._log_i < self._log.shape[0]:
            stats = self._log[self._log_i]
            self._log_i += 1
        state = _lib.PolicyOptState(self.moments.data_ptr(), self.lr.data_ptr(), self.step_count.data_ptr(), self.log_std_old.data_ptr(),
                                    stats.data_ptr())
        self._last = (ag, cg, state, kl)   # (alive until the next call: the library copies them during the call, a recorder may look later)
        wc._call("tsidb_policy_opt_step", *net_refs(a), C.byref(ag), C.byref(cg) if cg is not None else None, ptr(a.log_std),
                 C.c_void_p(l._grad(a.log_std).data_ptr()), C.byref(self._cfg), C.byref(state), C.byref(kl) if kl is not None else None,
                 ptr(ws), C.c_size_t(ws.numel() * 8), wc._stream())
        return stats

    def norm_kl64(self):
        """[2] float64, a view of the workspace: the gradient norm and the KL of the last step() as they were formed, before
        stats' float32 cast (include/tsidb.h: behind the workspace's partial sums)"""
        if self.workspace is None:
            raise _bad("no step() has run")
        n = sum((p.numel() + _lib.POL_OPT_CHUNK - 1) // _lib.POL_OPT_CHUNK for p in self._params)
        n += 2 * ((self._last_M + _lib.POL_LEARN_SEG_ROWS - 1) // _lib.POL_LEARN_SEG_ROWS)
        return self.workspace[n:n + 2]

    # ---------------------------------------------------------------- checkpoints, in torch.optim.Adam's layout
    def state_dict(self):
        """torch.optim.Adam's state_dict over learner.parameters(): state[i] = {step, exp_avg, exp_avg_sq} and one param group;
        loads into torch.optim.Adam(learner.parameters()).  Reads lr and step_count back: a host sync."""
        group = torch.optim.Adam([torch.zeros(1)], lr=float(self.lr.item()), betas=self.betas, eps=self.eps).state_dict()["param_groups"][0]
        group["params"] = list(range(len(self._params)))
        step = float(self.step_count.item())
        state = {}
        if step > 0:
            state = {i: dict(step=torch.tensor(step, dtype=torch.float32), exp_avg=self.exp_avg(p).clone(), exp_avg_sq=self.exp_avg_sq(p).clone())
                     for i, p in enumerate(self._params)}
        return dict(state=state, param_groups=[group])

    def load_state_dict(self, sd):
        """a state_dict() of this class or of torch.optim.Adam over the same parameters: lr, betas, eps, the step and the moments"""
        groups = sd.get("param_groups") if isinstance(sd, dict) else None
        if not isinstance(groups, (list, tuple)) or len(groups) != 1 or "state" not in sd:
            raise _bad("load_state_dict needs torch.optim.Adam's layout with one param group")
        g, state = groups[0], sd["state"]
        if len(g["params"]) != len(self._params):
            raise _bad(f"the checkpoint has {len(g['params'])} parameters, the learner {len(self._params)}")
        if g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False):
            raise _bad("weight_decay, amsgrad and maximize are not built")
        lr = g["lr"]
        lr = _number("lr", float(lr.item()) if isinstance(lr, torch.Tensor) else lr, 0.0, strict=True)
        self.betas, self.eps = _betas(tuple(g["betas"])), _number("eps", g["eps"], 0.0, strict=True)
        self._cfg = self._make_cfg()
        steps = set()
        with torch.no_grad():
            self.moments.zero_()
            for i, p in zip(g["params"], self._params):
                s = state.get(i)
                if s is None:
                    steps.add(0)
                    continue
                for key, view in (("exp_avg", self.exp_avg(p)), ("exp_avg_sq", self.exp_avg_sq(p))):
                    if tuple(s[key].shape) != tuple(p.shape):
                        raise _bad(f"the checkpoint's {key} of parameter {i} is {tuple(s[key].shape)}, the parameter {tuple(p.shape)}")
                    view.copy_(s[key])
                steps.add(int(float(s["step"])))
            if len(steps) != 1:
                raise _bad(f"the checkpoint's parameters are at different steps: {sorted(steps)}")
            self.step_count.fill_(steps.pop())
            self.lr.fill_(lr)
