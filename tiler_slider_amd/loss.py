"""The fused actor-critic loss (lib/libtiler_slider_loss.so, include/tiler_slider_loss.h): PPO, A2C or cross-entropy over the
samples of a logged trajectory, with its gradient, in one pass.

actor_critic_loss_grads() is the raw form: the loss' scalars and its gradient with respect to the logits and the values, four
launches on the current stream, no host synchronisation.  actor_critic_loss() wraps it in one autograd function, so that
`.loss.backward()` reaches the network behind the logits.  VecTilerSliderEnv.trajectory_loss() feeds it from a Rollout and a
TrajectoryReturns.  The plain-torch loss stays what it was: this is an opt-in for the three objectives everyone writes.  There
is no CPU path and no torch fallback.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _loss_cabi as lc

LossInfo = namedtuple("LossInfo", ("loss", "policy", "value", "entropy", "approx_kl", "clip_frac", "count"))
LossInfo.__doc__ = """0-dim float32 views of the call's scalars (include/tiler_slider_loss.h), all means over the live samples: the loss, its
policy term, the squared value error, the entropy, the approximate KL to the old policy and the share of samples PPO's clip
cut (both 0 without old_logits), and the number of live samples.  Device tensors: reading one synchronises, nothing else does."""

_workspaces = {}  # (device index, stream) -> uint8 tensor: the partial sums of one call; calls on one stream are ordered


def _workspace(device, stream, n_samples):
    need = lc.workspace_bytes(n_samples)
    ws = _workspaces.get((device.index, stream))
    if ws is None or ws.numel() < need:
        # the largest a call can need: the grid is bounded, so this is allocated once per device and stream
        ws = _workspaces[device.index, stream] = torch.empty(max(need, lc.workspace_bytes(lc.THREADS * lc.MAX_BLOCKS)), dtype=torch.uint8, device=device)
    return ws


def _check(logits, act, mask, adv, old_logits, values, ret):
    """The arguments as contiguous tensors of the call's dtypes: ValueErrors in the wording of targets._check_rollout."""
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() < 1 or logits.shape[-1] != 4:
        raise ValueError("logits must be a float32 tensor of shape [..., 4]")
    if logits.device.type != "cuda":
        raise ValueError(f"the loss runs on the GPU, logits live on {logits.device}")
    lead = tuple(logits.shape[:-1])

    def one(name, t, shape, dtypes):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise ValueError(f"{name} {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)} is not {list(shape)} of these logits")
        if t.device != logits.device:
            raise ValueError(f"{name} lives on {t.device}, the logits on {logits.device}")
        if t.dtype not in dtypes or not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous {' or '.join(str(d) for d in dtypes)}")
        return t.view(torch.uint8) if t.dtype == torch.bool else t

    if not logits.is_contiguous():
        raise ValueError("logits must be contiguous torch.float32")
    if act is None:
        raise ValueError("act is needed: the actions played, or the labels")
    f32 = (torch.float32,)
    return (lead, one("act", act, lead, (torch.uint8,)), one("mask", mask, lead, (torch.bool, torch.uint8)), one("adv", adv, lead, f32),
            one("old_logits", old_logits, lead + (4,), f32), one("values", values, lead, f32), one("ret", ret, lead, f32))


def _aligned(t, to):
    return t if t is None or t.data_ptr() % to == 0 else t.clone()


def _run(logits, values, act, mask, adv, old_logits, ret, clip, value_coef, entropy_coef, normalize_adv):
    """(scalars float32 [8], dlogits, dvalues or None): the checks and the one C-ABI call."""
    lead, act, mask, adv, old_logits, values, ret = _check(logits, act, mask, adv, old_logits, values, ret)
    if (values is None) != (ret is None):
        raise ValueError("values and ret come together: both or neither")
    if normalize_adv and adv is None:
        raise ValueError("normalize_adv needs adv")
    clip, value_coef, entropy_coef = float(clip), float(value_coef), float(entropy_coef)
    if not clip >= 0.0 or value_coef != value_coef or entropy_coef != entropy_coef:
        raise ValueError("clip must be >= 0 and the coefficients numbers")
    if old_logits is not None and clip == 0.0:
        raise ValueError("old_logits needs clip > 0")
    dev = logits.device
    detached = lambda t, to: None if t is None else _aligned(t.detach(), to)
    z, old, adv, v, ret = detached(logits, 16), detached(old_logits, 16), detached(adv, 4), detached(values, 4), detached(ret, 4)
    n = z.numel() // 4
    dlogits = torch.empty_like(z)
    dvalues = None if v is None else torch.empty(lead, dtype=torch.float32, device=dev)
    scalars = torch.empty(lc.SCALARS, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if n:
        ptr = lambda t: None if t is None else t.data_ptr()
        lin = lc.LossIn(ptr(z), ptr(old), ptr(act), ptr(mask), ptr(adv), ptr(v), ptr(ret), n, clip, value_coef, entropy_coef, int(bool(normalize_adv)))
        lout = lc.LossOut(ptr(dlogits), ptr(dvalues), scalars.data_ptr(), _workspace(dev, stream, n).data_ptr())
    else:  # no sample: the call zeroes the scalars and looks at no other pointer
        lin, lout = lc.LossIn(n_samples=0), lc.LossOut(scalars=scalars.data_ptr())
    with torch.cuda.device(dev):
        rc = lc.lib().ts_actor_critic_loss(C.byref(lin), C.byref(lout), stream)
    if rc:
        lc.check(rc, "ts_actor_critic_loss")
    return scalars, dlogits, dvalues


def _info(scalars, loss=None):
    fields = scalars[:len(LossInfo._fields)].unbind(0)
    return LossInfo(*fields) if loss is None else LossInfo(loss, *fields[1:])


def actor_critic_loss_grads(logits, act, *, mask=None, adv=None, old_logits=None, values=None, ret=None, clip=0.0, value_coef=0.5,
                            entropy_coef=0.0, normalize_adv=False):
    """(LossInfo, dlogits, dvalues): the loss of include/tiler_slider_loss.h over the samples logits [..., 4] (float32), act [...]
    (uint8: the action played or the label; a byte above 3 is no sample) and its gradient - dlogits like logits, dvalues like
    values (None without a value term), both exactly 0 on samples that are not live.  mask [...] (bool or uint8), adv, values and
    ret [...] (float32) are optional: without adv the policy term is a cross-entropy, with old_logits [..., 4] and clip > 0 it is
    PPO's clipped ratio, values and ret (both or neither) add value_coef (values - ret)^2; normalize_adv standardises adv over the
    live samples.  Nothing is read from autograd: pass the result on with
    torch.autograd.backward((logits, values), (dlogits, dvalues)).  Four launches on the current stream, a workspace cached per
    device and stream, no host synchronisation; sums without float atomics, so two calls on the same inputs agree bit for bit."""
    scalars, dlogits, dvalues = _run(logits, values, act, mask, adv, old_logits, ret, clip, value_coef, entropy_coef, normalize_adv)
    return _info(scalars), dlogits, dvalues


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, values, args):
        scalars, dlogits, dvalues = _run(logits, values, *args)
        ctx.has_values = dvalues is not None
        ctx.save_for_backward(*((dlogits, dvalues) if ctx.has_values else (dlogits,)))
        ctx.mark_non_differentiable(scalars)
        return scalars[0].clone(), scalars

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad, _):
        dlogits = ctx.saved_tensors[0]
        dvalues = ctx.saved_tensors[1] if ctx.has_values else None
        return (dlogits * grad if ctx.needs_input_grad[0] else None,
                dvalues * grad if ctx.has_values and ctx.needs_input_grad[1] else None, None)


def actor_critic_loss(logits, act, *, mask=None, adv=None, old_logits=None, values=None, ret=None, clip=0.0, value_coef=0.5,
                      entropy_coef=0.0, normalize_adv=False):
    """LossInfo of actor_critic_loss_grads() on the same arguments, whose `.loss` carries the grad_fn of ONE once-differentiable
    function: the forward runs the four launches and keeps dlogits and dvalues, the backward returns them times the incoming
    scalar - one torch multiply each over [..., 4] and [...], which a hand-written loop saves by using the raw form.  Under
    torch.no_grad(), or when neither logits nor values requires grad, `.loss` has no grad_fn.  The other fields never have one."""
    args = (act, mask, adv, old_logits, ret, clip, value_coef, entropy_coef, normalize_adv)
    if not (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (logits, values))):
        return _info(_run(logits, values, *args)[0])
    loss, scalars = _Loss.apply(logits, values, args)
    return _info(scalars, loss)


def trajectory_loss(env, logits, rollout, targets=None, values=None, labels=None, clip=0.0, value_coef=0.5, entropy_coef=0.0,
                    normalize_adv=False):
    """VecTilerSliderEnv.trajectory_loss: see there."""
    from .targets import TrajectoryReturns
    from .vec_env import Rollout
    env._require_open()
    if not isinstance(rollout, Rollout):
        raise TypeError(f"rollout must be a Rollout (rollout_policy(..., log=...)), got {type(rollout)}")
    if targets is not None and not isinstance(targets, TrajectoryReturns):
        raise TypeError(f"targets must be a TrajectoryReturns (trajectory_returns(...)), got {type(targets)}")
    N = env.num_envs
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3 or tuple(logits.shape[1:]) != (N, 4):
        raise ValueError(f"logits must be a float32 tensor of shape [K, {N}, 4] on {env.device}")
    if logits.device != env.device:
        raise ValueError(f"the logits live on {logits.device}, the environment on {env.device}")
    steps = int(logits.shape[0])
    if labels is not None:
        act = labels
    else:
        act = rollout.act_log
        if act is None:
            raise ValueError('the rollout must have logged its actions: log=("act", ...)')
    if tuple(act.shape) != (steps, N):
        raise ValueError(f"the rollout's {'labels' if labels is not None else 'act_log'} {tuple(act.shape)} is not {[steps, N]} of these logits")
    old = None
    if clip > 0.0:
        old = rollout.logits_log
        if old is None:
            raise ValueError('clip > 0 is PPO and needs the old policy: the rollout must have logged its logits: log=("logits", ...)')
    if normalize_adv and targets is None:
        raise ValueError("normalize_adv needs targets")
    if values is not None and targets is None:
        raise ValueError("a value term needs targets: the returns the values are set against")
    kw = dict(clip=clip, value_coef=value_coef, entropy_coef=entropy_coef, normalize_adv=normalize_adv, old_logits=old)
    if targets is not None:
        kw.update(mask=targets.mask, adv=targets.adv)
        if values is not None:
            kw.update(values=values, ret=targets.ret)
    return actor_critic_loss(logits, act, **kw)
