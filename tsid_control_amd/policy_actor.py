"""PolicyActor - the policy of a PolicyEnv on the device: a dense actor and an optional critic evaluated on the env's own
tensors in one launch (include/tsidb.h tsidb_policy_actor; csrc/tsidb_actor.hpp), the Gaussian sample with its
log-probability, and the storage of a rollout with its advantages (tsidb_policy_gae).  No reference counterpart (the
reference's only controller is TSID, main.py:113-129).

The parameters are torch tensors the caller owns - the weights and biases of torch.nn.Linear modules, a log_std vector - and
the kernel reads them in place at every launch: an optimiser step on them needs no call here.  The action noise is a hash of
(seed, stream 21 / 22, actuator, env_offset + env, episode, ep_len), as every other draw of the environment: no generator
state, a captured rollout replays, a batch split over ranks samples what the unsplit batch samples, and two act() calls on
the same observation return the same sample.
"""
import ctypes as C

import torch

from . import _lib
from ._policy_util import bad, device_tensor, flag, net_refs, ptr
from .policy_env import _whole_below

_INPUT_NAMES = ("obs", "priv", "height_scan", "teacher_obs", "command", "obs_history")
_bad = bad("PolicyActor")


def _layers_of(net, activation, name):
    """[(weight, bias)], activation name of a torch.nn.Sequential of Linear layers with one activation type between them, or of
    a list of (weight, bias) pairs"""
    if isinstance(net, torch.nn.Sequential):
        kinds = {torch.nn.ELU: "elu", torch.nn.Tanh: "tanh", torch.nn.ReLU: "relu"}
        layers, found, want_linear = [], None, True
        for m in net:
            if want_linear:
                if not isinstance(m, torch.nn.Linear):
                    raise _bad(f"{name}: expected a Linear layer, got {type(m).__name__} (a stack is Linear, activation, Linear, ...)")
                layers.append((m.weight, m.bias))
            else:
                if type(m) not in kinds:
                    raise _bad(f"{name}: activation {type(m).__name__} is not one of ELU, Tanh, ReLU")
                if isinstance(m, torch.nn.ELU) and m.alpha != 1.0:
                    raise _bad(f"{name}: ELU alpha must be 1, got {m.alpha}")
                if found not in (None, kinds[type(m)]):
                    raise _bad(f"{name}: one activation type per network, got {found} and {kinds[type(m)]}")
                found = kinds[type(m)]
            want_linear = not want_linear
        if want_linear and layers:
            raise _bad(f"{name}: the last layer must be a Linear (the output is linear)")
        return layers, found or activation or "elu"
    if isinstance(net, (list, tuple)):
        layers = []
        for i, item in enumerate(net):
            if not isinstance(item, (list, tuple)) or len(item) != 2:
                raise _bad(f"{name}: layer {i} must be a (weight, bias) pair")
            layers.append(tuple(item))
        return layers, activation or "elu"
    raise _bad(f"{name} must be a torch.nn.Sequential or a list of (weight, bias) pairs, got {type(net).__name__}")


class _Net:
    """one network as the library takes it: the tsidb_policy_net struct and the tensors behind its pointers"""

    def __init__(self, env, net, inputs, activation, name, last, last_name):
        wc = env.wc
        layers, act = _layers_of(net, activation, name)
        if act not in _lib.POL_ACTIVATIONS:
            raise _bad(f"{name}: activation must be one of {_lib.POL_ACTIVATIONS}, got {act!r}")
        if not 1 <= len(layers) <= _lib.POL_NET_MAXLAYERS:
            raise _bad(f"{name}: 1 .. {_lib.POL_NET_MAXLAYERS} layers, got {len(layers)}")
        if isinstance(inputs, (str, torch.Tensor)):
            inputs = (inputs,)
        if not 1 <= len(inputs) <= _lib.POL_NET_MAXBLOCKS:
            raise _bad(f"{name}_inputs: 1 .. {_lib.POL_NET_MAXBLOCKS} blocks, got {len(inputs)}")
        self.blocks, self.block_names = [], [b if isinstance(b, str) else None for b in inputs]   # (the names: PolicySymmetry's tables)
        for b in inputs:
            if isinstance(b, str):
                if b not in _INPUT_NAMES:
                    raise _bad(f"{name}_inputs: unknown input {b!r} (known: {_INPUT_NAMES}, or an [N, k] tensor)")
                t = getattr(env, b, None)
                if t is None:
                    raise _bad(f"{name}_inputs: the env has no {b} (height_scan needs terrain with a scan, teacher_obs needs tsid, "
                               "obs_history needs obs_history=)")
            else:
                t = b
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != env.num_envs or t.shape[1] < 1 or t.dtype != wc.dtype \
                    or t.device != wc.device or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
                what = (tuple(t.shape), t.dtype, t.device, t.stride()) if isinstance(t, torch.Tensor) else type(t).__name__
                raise _bad(f"{name}_inputs: a block must be an [{env.num_envs}, k] {wc.dtype} tensor on {wc.device} with unit column stride, got {what}")
            self.blocks.append(t)
        self.K = sum(int(t.shape[1]) for t in self.blocks)
        if not 1 <= self.K <= _lib.POL_NET_MAXWIDTH:
            raise _bad(f"{name}_inputs: the input row has {self.K} columns, 1 .. {_lib.POL_NET_MAXWIDTH} allowed")
        self.layers, self.activation, fan_in = [], act, self.K
        for i, (w, b) in enumerate(layers):
            if w is None:
                raise _bad(f"{name}: layer {i} has no weight")
            for t, what in ((w, "weight"), (b, "bias")):
                if t is not None:
                    device_tensor("PolicyActor", f"{name}: layer {i} {what} must be a contiguous float32 tensor on {wc.device}", t, None,
                                  torch.float32, wc.device)
            if w.dim() != 2 or w.shape[1] != fan_in:
                raise _bad(f"{name}: layer {i} weight must be [width, {fan_in}] (its input has {fan_in} columns), got {tuple(w.shape)}")
            width = int(w.shape[0])
            if not 1 <= width <= _lib.POL_NET_MAXWIDTH:
                raise _bad(f"{name}: layer {i} width {width} is outside 1 .. {_lib.POL_NET_MAXWIDTH}")
            if b is not None and tuple(b.shape) != (width,):
                raise _bad(f"{name}: layer {i} bias must be [{width}], got {tuple(b.shape)}")
            self.layers.append((w, b))
            fan_in = width
        if fan_in != last:
            raise _bad(f"{name}: the last width must be {last_name} = {last}, got {fan_in}")
        s = self.struct = _lib.PolicyNet()
        s.n_layers, s.activation, s.n_blocks = len(self.layers), _lib.POL_ACTIVATIONS.index(act), len(self.blocks)
        for i, (w, b) in enumerate(self.layers):
            s.width[i], s.weight[i], s.bias[i] = int(w.shape[0]), w.data_ptr(), (b.data_ptr() if b is not None else None)
        for i, t in enumerate(self.blocks):
            s.block[i], s.block_ld[i], s.block_cols[i] = t.data_ptr(), int(t.stride(0)), int(t.shape[1])


class PolicyActor:
    """env: the PolicyEnv whose tensors are the inputs.  actor, critic (None = no value): a torch.nn.Sequential of Linear layers
    with one activation type (ELU, Tanh or ReLU) between them, or a list of (weight, bias) pairs with activation = "elu" / "tanh" /
    "relu"; 1 .. 4 layers of at most 512 outputs, the actor's last width NA, the critic's 1; float32, contiguous, on the env's
    device; the tensors are kept and read in place at every launch.  actor_inputs, critic_inputs (None = the actor's): the column
    blocks of the input row, up to 4 and 512 columns in total - "obs", "priv", "height_scan", "teacher_obs", "command", "obs_history"
    (the stacked frames of an env built with obs_history=, which the env keeps current inside step(): frames * K columns count
    against the 512), or any [N, k] tensor of the env's dtype (a strided row view is fine).  log_std: [NA] float32, read in place (None = zeros, kept as
    self.log_std).  seed: of the action noise (None = the env's seed); env_offset (None = the randomisation's, else 0).
    normalizer: a PolicyNormalizer (policy_normalizer.py) - running mean and variance of each network's input row, applied as
    the launch loads the row; actor_input / critic_input then hold the normalised rows.  None = the raw rows, as ever.

    Tensors, written by act(): action [N, NA] (the env's dtype: hand it to env.step), action32, mean [N, NA], logp [N], value [N]
    (None without a critic), actor_input [N, K_actor], critic_input [N, K_critic] (float32)."""

    def __init__(self, env, actor, critic=None, actor_inputs=("obs",), critic_inputs=None, log_std=None, seed=None, env_offset=None,
                 activation=None, normalizer=None):
        wc = env.wc
        self.env, self.NA = env, env.NA
        N, NA = env.num_envs, env.NA
        self.actor_net = _Net(env, actor, actor_inputs, activation, "actor", NA, "NA")
        self.critic_net = None
        if critic is not None:
            self.critic_net = _Net(env, critic, actor_inputs if critic_inputs is None else critic_inputs, activation, "critic", 1, "1")
        elif critic_inputs is not None:
            raise _bad("critic_inputs without a critic")
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=wc.device)
        if log_std is None:
            log_std = f32(NA)
        self.log_std = device_tensor("PolicyActor", f"log_std must be a contiguous ({NA},) float32 tensor on {wc.device}", log_std, (NA,),
                                     torch.float32, wc.device)
        if seed is None:
            seed = int(env.params[_lib.POL_P_SEED]) if getattr(env, "params", None) is not None else 0
        if env_offset is None:
            dr = getattr(env, "dr_params", None)
            env_offset = int(dr[_lib.POL_DR_ENV_OFFSET]) if dr is not None else 0
        self.seed, self.env_offset = _whole_below("PolicyActor", "seed", seed, 32), _whole_below("PolicyActor", "env_offset", env_offset, 31)
        self.action = torch.zeros(N, NA, dtype=wc.dtype, device=wc.device)
        self.action32, self.mean, self.logp = f32(N, NA), f32(N, NA), f32(N)
        self.value = f32(N) if critic is not None else None
        self.actor_input = f32(N, self.actor_net.K)
        self.critic_input = f32(N, self.critic_net.K) if critic is not None else None
        self.normalizer = None
        if normalizer is not None:
            from .policy_normalizer import PolicyNormalizer
            if not isinstance(normalizer, PolicyNormalizer):
                raise _bad(f"normalizer must be a PolicyNormalizer or None, got {type(normalizer).__name__}")
            normalizer._attach(self)
            self.normalizer = normalizer

    def _launch(self, sample, actor=True, critic=True, action=None, action32=None, mean=None, logp=None, value=None, actor_input=None,
                critic_input=None):
        """one tsidb_policy_actor call writing the given tensors (None = not written)"""
        wc = self.env.wc
        out = _lib.PolicyActorOut(*(ptr(t) for t in (action, action32, mean, logp, value, actor_input, critic_input)))
        self._out = out      # (alive until the next call: the library copies it during the call, a recorder may look later)
        a, c = net_refs(self)
        nets = (a if actor else None, c if critic else None)
        rest = (C.byref(out), ptr(self.log_std), C.c_uint64(self.seed), C.c_uint64(self.env_offset),
                _lib.POL_ACTOR_SAMPLE if sample else 0, wc._stream())
        nz = self.normalizer
        if nz is None:
            wc._call("tsidb_policy_actor", C.byref(self.env._bufs), *nets, *rest)
        else:
            wc._call("tsidb_policy_actor_norm", C.byref(self.env._bufs), *nets, C.byref(nz.actor.struct) if actor else None,
                     C.byref(nz.critic.struct) if nets[1] is not None and nz.critic is not None else None, *rest)

    def observe(self):
        """with a normaliser in training mode: its update() on the env's current tensors - what act() and every step of
        PolicyEnv.rollout do before they evaluate; else nothing"""
        if self.normalizer is not None and self.normalizer.training:
            self.normalizer.update()

    def act(self, deterministic=False):
        """One launch on the env's current tensors: the actor, the critic, and unless deterministic the sample.  Returns a dict
        of the preallocated tensors action, action32, mean, logp, value (updated in place by every call; value None without a
        critic).  deterministic: action = mean, logp = the density at the mean.  With a normaliser in training mode its
        update() comes first (two more launches), and the rows are normalised with the updated statistics."""
        self.observe()
        self._launch(not deterministic, action=self.action, action32=self.action32, mean=self.mean, logp=self.logp, value=self.value,
                     actor_input=self.actor_input, critic_input=self.critic_input)
        return dict(action=self.action, action32=self.action32, mean=self.mean, logp=self.logp, value=self.value)

    def written(self):
        """the tensors act() writes, the normaliser's state among them"""
        own = [t for t in (self.action, self.action32, self.mean, self.logp, self.value, self.actor_input, self.critic_input) if t is not None]
        return own + (self.normalizer.written() if self.normalizer is not None else [])


class RolloutStorage:
    """[T, N, ...] tensors of PolicyEnv.rollout: actor_input, critic_input (None without a critic), action, mean [T, N, .], logp
    [T, N] in float32, value [T + 1, N] float32 (the last row: the critic on the observation after the last step; zeros without a
    critic), reward, done [T, N] in the env's dtype, timeout [T, N] int32; advantage, returns [T, N] float32 once gae() has run.

    teacher = True (an env with tsid set, in "position" or "motor" mode) adds what PolicyEnv.rollout records of the TSID teacher
    (include/tsidb.h tsidb_policy_teacher_mix): teacher_action [T, N, NA] float32, the label of each stored row; teacher_weight
    [T, N] float32, 0 for the rows whose env had just been restarted (their label belongs to the fallen robot); teacher_executed
    [T, N] int32, 1 where the env executed the teacher's action instead of the stored one.  action and logp stay the policy's own
    sample and density.  The default allocates nothing new."""

    teacher_action = teacher_weight = teacher_executed = None

    def __init__(self, env, actor, steps, teacher=False):
        wc = env.wc
        T, N, NA = int(steps), env.num_envs, env.NA
        self.env, self.actor, self.steps = env, actor, T
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=wc.device)
        self.actor_input = z(T, N, actor.actor_net.K)
        self.critic_input = z(T, N, actor.critic_net.K) if actor.critic_net is not None else None
        self.action, self.mean, self.logp = z(T, N, NA), z(T, N, NA), z(T, N)
        self.value = z(T + 1, N)
        self.reward, self.done, self.timeout = z(T, N, dt=wc.dtype), z(T, N, dt=wc.dtype), z(T, N, dt=torch.int32)
        self.advantage = self.returns = None
        if flag("RolloutStorage", "teacher", teacher):
            if getattr(env, "tsid", None) is None:
                raise _lib.TsidbError("RolloutStorage: teacher = True needs an env with tsid = 'stand' or 'walk': there is no teacher to label with")
            if getattr(env, "mode", None) not in ("position", "motor"):
                raise _lib.TsidbError(f"RolloutStorage: teacher = True needs mode 'position' or 'motor', got {getattr(env, 'mode', None)!r} "
                                      "(in residual mode teacher_action is 0 by definition: there is nothing to imitate)")
            self.teacher_action, self.teacher_weight = z(T, N, NA), z(T, N)
            self.teacher_executed = z(T, N, dt=torch.int32)

    def tensors(self):
        return [t for t in (self.actor_input, self.critic_input, self.action, self.mean, self.logp, self.value, self.reward, self.done,
                            self.timeout, self.advantage, self.returns, self.teacher_action, self.teacher_weight, self.teacher_executed)
                if t is not None]

    def gae(self, gamma=0.99, lam=0.95):
        """(advantage, returns), each [T, N] float32: rsl_rl's generalised advantage estimation of the stored rollout, one launch
        on the current stream (tsidb_policy_gae); the two tensors are allocated once and rewritten by every call"""
        wc = self.env.wc
        if self.advantage is None:
            self.advantage, self.returns = torch.zeros_like(self.logp), torch.zeros_like(self.logp)
        wc._call("tsidb_policy_gae", self.steps, ptr(self.reward), ptr(self.done), ptr(self.timeout), ptr(self.value), C.c_float(gamma),
                 C.c_float(lam), ptr(self.advantage), ptr(self.returns), wc._stream())
        return self.advantage, self.returns


def rollout_written(storage):
    """Every tensor a PolicyEnv.rollout into `storage` writes beyond the env's own (PolicyEnv.written()): what a caller that
    captures a rollout in a graph keeps alive, and rewinds after its warm-up if it compares runs."""
    yield from storage.tensors()    # (a teacher storage's labels, weights and executed flags among them)
    yield storage.actor.action
    beta = getattr(storage.env, "_teacher_beta", None)
    if beta is not None:
        yield beta
    if storage.actor.normalizer is not None:
        yield from storage.actor.normalizer.written()
