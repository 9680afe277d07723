"""The actor-critic network (lib/libtiler_slider_ac.so, include/tiler_slider_ac.h): the logits AND the value of a logged
trajectory as differentiable functions of one network's parameters.

ActorCriticNet holds the four parameters of PolicyNet's one-hidden-layer MLP and a value head of its own (wv [hidden], bv [1]) on
the same hidden layer, all in the kernels' layout: policy() is the MlpPolicy that shares the actor's storage, so after opt.step()
the next rollout_policy() plays the new weights without a copy.  trajectory_outputs() is one k_ac_forward launch; with parameters
that require grad both results carry the grad_fn of one autograd.Function whose backward is one k_ac_backward launch.  The loss
stays the user's, in torch.  There is no CPU path and no torch fallback.
"""
import ctypes as C
import math

import torch

from . import _ac_cabi as ac
from .policy import MlpPolicy, _prepare
from .train import _Samples, _trajectory_cells


class ActorCriticNet(torch.nn.Module):
    """h = relu(x @ w1 + b1), logits = h @ w2 + b2, value = h @ wv + bv on x = env.encode_onehot().flatten(1), the parameters in the
    kernels' layout: w1 [features, hidden], b1 [hidden], w2 [hidden, 4], b2 [4], wv [hidden], bv [1], float32 on a CUDA device,
    initialised as torch.nn.Linear initialises (uniform in +- 1 / sqrt(fan_in); wv and bv as w2 and b2) from `generator` (a
    torch.Generator of that device, or None)."""

    def __init__(self, features, hidden, device, generator=None):
        super().__init__()
        features, hidden = int(features), int(hidden)
        limit = ac._train_cabi._policy_cabi.POLICY_MAX_HIDDEN
        if features < 1 or not 1 <= hidden <= limit:
            raise ValueError(f"features must be >= 1 and 1 <= hidden <= {limit}, got {features}, {hidden}")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"the network must live on the environment's GPU, got {device}")

        def uniform(shape, fan_in):
            bound = 1.0 / math.sqrt(fan_in)
            return torch.nn.Parameter((torch.rand(shape, device=device, dtype=torch.float32, generator=generator) * 2 - 1) * bound)

        self.features, self.hidden = features, hidden
        self.w1, self.b1 = uniform((features, hidden), features), uniform((hidden,), features)
        self.w2, self.b2 = uniform((hidden, 4), hidden), uniform((4,), hidden)
        self.wv, self.bv = uniform((hidden,), hidden), uniform((1,), hidden)

    def _params(self):
        return self.w1, self.b1, self.w2, self.b2, self.wv, self.bv

    def policy(self):
        """The MlpPolicy that shares the actor's storage: it plays whatever the parameters hold when a kernel reads them."""
        return MlpPolicy.from_kernel_layout(self.w1, self.b1, self.w2, self.b2)

    @classmethod
    def from_linear(cls, l1, l2, lv):
        """From three torch.nn.Linear layers (all with bias), l2(relu(l1(x))) the logits and lv(relu(l1(x))) the value: a copy,
        transposed into the kernels' layout."""
        if l1.bias is None or l2.bias is None or lv.bias is None:
            raise ValueError("all three layers need a bias")
        H = l1.weight.shape[0]
        if tuple(l2.weight.shape) != (4, H) or tuple(lv.weight.shape) != (1, H):
            raise ValueError(f"l1 must be [H, D], l2 [4, H] and lv [1, H], got {tuple(l1.weight.shape)}, {tuple(l2.weight.shape)} and "
                             f"{tuple(lv.weight.shape)}")
        net = cls(l1.weight.shape[1], H, l1.weight.device)
        with torch.no_grad():
            net.w1.copy_(l1.weight.t())
            net.b1.copy_(l1.bias)
            net.w2.copy_(l2.weight.t())
            net.b2.copy_(l2.bias)
            net.wv.copy_(lv.weight[0])
            net.bv.copy_(lv.bias)
        return net

    def to_linear(self):
        """(l1, l2, lv): three torch.nn.Linear layers holding copies of the parameters, (l2(relu(l1(x))), lv(relu(l1(x)))) the same
        network."""
        dev = self.w1.device
        l1 = torch.nn.Linear(self.features, self.hidden, device=dev, dtype=torch.float32)
        l2 = torch.nn.Linear(self.hidden, 4, device=dev, dtype=torch.float32)
        lv = torch.nn.Linear(self.hidden, 1, device=dev, dtype=torch.float32)
        with torch.no_grad():
            l1.weight.copy_(self.w1.t())
            l1.bias.copy_(self.b1)
            l2.weight.copy_(self.w2.t())
            l2.bias.copy_(self.b2)
            lv.weight.copy_(self.wv.unsqueeze(0))
            lv.bias.copy_(self.bv)
        return l1, l2, lv

    def forward(self, x):
        """(logits [n, 4], value [n]) of the dense network on planes x [n, features] (for comparison; the kernels never build the
        planes)."""
        h = torch.relu(x @ self.w1 + self.b1)
        return h @ self.w2 + self.b2, h @ self.wv + self.bv

    def extra_repr(self):
        return f"features={self.features}, hidden={self.hidden}"


class _AcSamples(_Samples):
    """train._Samples - the environment, the cells of the samples and the level tensors as they were at the forward - with the two
    launches of this library."""

    def head(self, wv, bv):
        return ac.ValueHead(wv.data_ptr(), bv.data_ptr())

    def forward(self, w1, b1, w2, b2, wv, bv):
        env = self.env
        logits = torch.empty((self.steps, env.num_envs, 4), dtype=torch.float32, device=env.device)
        values = torch.empty((self.steps, env.num_envs), dtype=torch.float32, device=env.device)
        if env.num_envs:
            mlp, head, tin, st = self.mlp(w1, b1, w2, b2), self.head(wv, bv), self.train_in(), self.state()
            env._call("ts_ac_forward", C.byref(env._dims), C.byref(st), C.byref(mlp), C.byref(head), C.byref(tin), logits.data_ptr(),
                      values.data_ptr(), binding=ac)
        return logits, values

    def backward(self, w1, b1, w2, b2, wv, bv, dlogits, dvalues):
        env = self.env
        env._require_open()
        N = env.num_envs
        dlogits = torch.zeros((self.steps, N, 4), dtype=torch.float32, device=env.device) if dlogits is None else dlogits.to(torch.float32).contiguous()
        dvalues = torch.zeros((self.steps, N), dtype=torch.float32, device=env.device) if dvalues is None else dvalues.to(torch.float32).contiguous()
        if dlogits.data_ptr() & 15:
            dlogits = dlogits.clone()
        if dvalues.data_ptr() & 3:
            dvalues = dvalues.clone()
        grads = [torch.zeros_like(t) for t in (w1, b1, w2, b2, wv, bv)]
        if N:
            mlp, head, tin, st = self.mlp(w1, b1, w2, b2), self.head(wv, bv), self.train_in(), self.state()
            grad = ac.MlpGrad(*(g.data_ptr() for g in grads[:4]))
            head_grad = ac.ValueHeadGrad(grads[4].data_ptr(), grads[5].data_ptr())
            env._call("ts_ac_backward", C.byref(env._dims), C.byref(st), C.byref(mlp), C.byref(head), C.byref(tin), dlogits.data_ptr(),
                      dvalues.data_ptr(), C.byref(grad), C.byref(head_grad), binding=ac)
        return grads


class _TrajectoryOutputs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, samples, w1, b1, w2, b2, wv, bv):
        ctx.samples = samples
        ctx.set_materialize_grads(False)  # a loss that uses one output passes None for the other: zero-filled in backward()
        ctx.save_for_backward(w1, b1, w2, b2, wv, bv)
        return samples.forward(w1, b1, w2, b2, wv, bv)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits, dvalues):
        return (None, *ctx.samples.backward(*ctx.saved_tensors, dlogits, dvalues))


def trajectory_outputs(env, net, rollout=None):
    """VecTilerSliderEnv.trajectory_outputs: see there."""
    if not isinstance(net, ActorCriticNet):
        raise TypeError(f"expected an ActorCriticNet, got {type(net)}")
    _prepare(env, net.policy())  # the environment, the shape, the width, the features and the device
    first, pos_log, steps = _trajectory_cells(env, rollout)
    params = net._params()
    if not (torch.is_grad_enabled() and any(p.requires_grad for p in params)):
        return _AcSamples(env, first, pos_log, steps).forward(*(p.detach() for p in params))
    if rollout is None:
        first = first.clone()  # the backward reads the cells again: the boards may have moved by then
    return _TrajectoryOutputs.apply(_AcSamples(env, first, pos_log, steps), *params)
