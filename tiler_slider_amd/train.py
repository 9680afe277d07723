"""Trainable policies (lib/libtiler_slider_train.so, include/tiler_slider_train.h): the logits of a logged trajectory as a
differentiable function of the network's parameters.

PolicyNet holds the four parameters of the one-hidden-layer MLP in the kernels' layout, so that the MlpPolicy of policy() shares
their storage: after opt.step() the next rollout_policy() plays the new weights without a copy.  trajectory_logits() is one
k_train_forward launch; with a PolicyNet whose parameters require grad its result carries a grad_fn whose backward is one
k_train_backward launch.  The loss stays the user's, in torch, on [K, N, 4] floats.  There is no CPU path and no torch fallback.
"""
import ctypes as C
import math

import torch

from . import _train_cabi as tc
from .policy import MlpPolicy, _prepare


class PolicyNet(torch.nn.Module):
    """logits = relu(x @ w1 + b1) @ w2 + b2 on x = env.encode_onehot().flatten(1), the parameters in the kernels' layout:
    w1 [features, hidden], b1 [hidden], w2 [hidden, 4], b2 [4], float32 on a CUDA device, initialised as torch.nn.Linear
    initialises (uniform in +- 1 / sqrt(fan_in)) from `generator` (a torch.Generator of that device, or None)."""

    def __init__(self, features, hidden, device, generator=None):
        super().__init__()
        features, hidden = int(features), int(hidden)
        if features < 1 or not 1 <= hidden <= tc._policy_cabi.POLICY_MAX_HIDDEN:
            raise ValueError(f"features must be >= 1 and 1 <= hidden <= {tc._policy_cabi.POLICY_MAX_HIDDEN}, got {features}, {hidden}")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"the network must live on the environment's GPU, got {device}")

        def uniform(shape, fan_in):
            bound = 1.0 / math.sqrt(fan_in)
            return torch.nn.Parameter((torch.rand(shape, device=device, dtype=torch.float32, generator=generator) * 2 - 1) * bound)

        self.features, self.hidden = features, hidden
        self.w1, self.b1 = uniform((features, hidden), features), uniform((hidden,), features)
        self.w2, self.b2 = uniform((hidden, 4), hidden), uniform((4,), hidden)

    def policy(self):
        """The MlpPolicy that shares the parameters' storage: it plays whatever they hold when a kernel reads them."""
        return MlpPolicy.from_kernel_layout(self.w1, self.b1, self.w2, self.b2)

    @classmethod
    def from_linear(cls, l1, l2):
        """From two torch.nn.Linear layers (both with bias), l2(relu(l1(x))): a copy, transposed into the kernels' layout."""
        if l1.bias is None or l2.bias is None:
            raise ValueError("both layers need a bias")
        if l2.weight.shape[0] != 4 or l2.weight.shape[1] != l1.weight.shape[0]:
            raise ValueError(f"l1 must be [H, D] and l2 [4, H], got {tuple(l1.weight.shape)} and {tuple(l2.weight.shape)}")
        net = cls(l1.weight.shape[1], l1.weight.shape[0], l1.weight.device)
        with torch.no_grad():
            net.w1.copy_(l1.weight.t())
            net.b1.copy_(l1.bias)
            net.w2.copy_(l2.weight.t())
            net.b2.copy_(l2.bias)
        return net

    def to_linear(self):
        """(l1, l2): two torch.nn.Linear layers holding copies of the parameters, l2(relu(l1(x))) the same network."""
        l1 = torch.nn.Linear(self.features, self.hidden, device=self.w1.device, dtype=torch.float32)
        l2 = torch.nn.Linear(self.hidden, 4, device=self.w1.device, dtype=torch.float32)
        with torch.no_grad():
            l1.weight.copy_(self.w1.t())
            l1.bias.copy_(self.b1)
            l2.weight.copy_(self.w2.t())
            l2.bias.copy_(self.b2)
        return l1, l2

    def forward(self, x):
        """The dense network on planes x [n, features] (for comparison; the kernels never build the planes)."""
        return torch.relu(x @ self.w1 + self.b1) @ self.w2 + self.b2

    def extra_repr(self):
        return f"features={self.features}, hidden={self.hidden}"


class _Samples:
    """What both launches of one trajectory_logits() call share: the environment, the cells of the samples and their count, and
    the level tensors (obstacles, targets) as they were at the forward - held here, so that the backward reads the levels the
    forward read even if the environment is given other buffers in between."""

    def __init__(self, env, first, pos_log, steps):
        self.env, self.first, self.pos_log, self.steps = env, first, pos_log, steps
        self.blk, self.tgt = env._blk, env._tgt

    def state(self):
        """A ts_state of the held level tensors alone: the training calls read neither the cells nor the counters of the state."""
        from ._cabi import State
        from .vec_env import _ptr
        return State(None, None, _ptr(self.tgt), _ptr(self.blk), None, None, None)

    def train_in(self):
        from .vec_env import _ptr
        return tc.TrainIn(_ptr(self.first), _ptr(self.pos_log), self.steps, 0)

    def mlp(self, w1, b1, w2, b2):
        return tc.Mlp(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w1.shape[1], 0)

    def forward(self, w1, b1, w2, b2):
        env = self.env
        out = torch.empty((self.steps, env.num_envs, 4), dtype=torch.float32, device=env.device)
        if env.num_envs:
            mlp, tin, st = self.mlp(w1, b1, w2, b2), self.train_in(), self.state()
            env._call("ts_train_forward", C.byref(env._dims), C.byref(st), C.byref(mlp), C.byref(tin), out.data_ptr(), binding=tc)
        return out

    def backward(self, w1, b1, w2, b2, dlogits):
        env = self.env
        env._require_open()
        dlogits = dlogits.to(torch.float32).contiguous()
        if dlogits.data_ptr() & 15:
            dlogits = dlogits.clone()
        grads = [torch.zeros_like(t) for t in (w1, b1, w2, b2)]
        if env.num_envs:
            mlp, tin, st = self.mlp(w1, b1, w2, b2), self.train_in(), self.state()
            grad = tc.MlpGrad(*(g.data_ptr() for g in grads))
            env._call("ts_train_backward", C.byref(env._dims), C.byref(st), C.byref(mlp), C.byref(tin), dlogits.data_ptr(),
                      C.byref(grad), binding=tc)
        return grads


class _TrajectoryLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, samples, w1, b1, w2, b2):
        ctx.samples = samples
        ctx.save_for_backward(w1, b1, w2, b2)
        return samples.forward(w1, b1, w2, b2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits):
        return (None, *ctx.samples.backward(*ctx.saved_tensors, dlogits))


def _trajectory_cells(env, rollout):
    """(first, pos_log, steps) of the samples of `rollout` - or of the boards as they stand (rollout=None: steps = 1) -, checked
    against the environment: what trajectory_logits() and trajectory_outputs() share."""
    from .vec_env import Rollout
    T, N = env.n_tiles, env.num_envs
    if rollout is None:
        return env._pos, None, 1
    if not isinstance(rollout, Rollout):
        raise TypeError(f"rollout must be a Rollout (rollout_policy(..., log=('start', 'pos'))), got {type(rollout)}")
    if rollout.start_pos is None or rollout.pos_log is None:
        raise ValueError("the rollout must have logged its start and its cells: rollout_policy(..., log=('start', 'pos'))")
    first, pos_log = rollout.start_pos, rollout.pos_log
    steps = int(pos_log.shape[0]) if pos_log.dim() == 3 else -1
    if steps < 1 or tuple(first.shape) != (T, N) or tuple(pos_log.shape) != (steps, T, N):
        raise ValueError(f"the rollout's start_pos {tuple(first.shape)} and pos_log {tuple(pos_log.shape)} are not [{T}, {N}] and "
                         f"[steps >= 1, {T}, {N}] of this environment")
    for t in (first, pos_log):
        if t.device != env.device:
            raise ValueError(f"the rollout lives on {t.device}, the environment on {env.device}")
        if t.dtype != env._pos.dtype or not t.is_contiguous():
            raise ValueError(f"the rollout's cells must be contiguous {env._pos.dtype}")
    return first, pos_log, steps


def trajectory_logits(env, net, rollout=None):
    """VecTilerSliderEnv.trajectory_logits: see there."""
    if isinstance(net, PolicyNet):
        policy = net.policy()
    elif isinstance(net, MlpPolicy):
        policy = net
    else:
        raise TypeError(f"expected a PolicyNet or an MlpPolicy, got {type(net)}")
    _prepare(env, policy)  # the environment, the shape, the width, the features and the device
    first, pos_log, steps = _trajectory_cells(env, rollout)
    wants_grad = isinstance(net, PolicyNet) and torch.is_grad_enabled() and any(p.requires_grad for p in (net.w1, net.b1, net.w2, net.b2))
    if not wants_grad:
        return _Samples(env, first, pos_log, steps).forward(policy.w1, policy.b1, policy.w2, policy.b2)
    if rollout is None:
        first = first.clone()  # the backward reads the cells again: the boards may have moved by then
    return _TrajectoryLogits.apply(_Samples(env, first, pos_log, steps), net.w1, net.b1, net.w2, net.b2)
