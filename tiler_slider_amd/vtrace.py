"""V-trace targets (lib/libtiler_slider_vtrace.so, include/tiler_slider_vtrace.h): off-policy returns and advantages of a logged
rollout whose actions were not drawn from the network being trained - a mixed or epsilon-greedy rollout, or a log replayed after
the weights have moved.

trajectory_vtrace() is one k_traj_vtrace launch over a Rollout's flags_log, act_log and logits_log (and expert_log, pos_log
where they matter): the behaviour probability of every action played, the truncated importance weights, and the backward
recursion of trajectory_returns() with them inside.  There is no CPU path and no torch fallback.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _policy_cabi as pc
from . import _vtrace_cabi as vc
from .targets import RewardWeights, TrajectoryReturns, _check_rollout, _values


class VtraceTargets(namedtuple("VtraceTargets", ("reward", "adv", "ret", "mask", "weight", "log_mu"))):
    """reward, adv, ret float32 [K, N] and mask bool [K, N] as TrajectoryReturns' - `ret` the V-trace target v_s, `adv` the
    policy-gradient advantage with its truncated weight rho included -, weight float32 [K, N]: the importance weight pi / mu of
    the action played, unclipped (+inf where mu is 0), log_mu float32 [K, N]: the log of its behaviour probability.  All are 0 where
    mask is False."""
    __slots__ = ()

    @property
    def returns(self):
        """TrajectoryReturns(reward, adv, ret, mask): what trajectory_loss(logits, rollout, vt.returns, values=v) takes - at
        clip=0 that is the V-trace actor-critic loss."""
        return TrajectoryReturns(self.reward, self.adv, self.ret, self.mask)


def _threshold(x, name):
    x = float(x)
    if not 0.0 <= x <= 1.0:
        raise ValueError(f"{name} must be 0..1")
    return int(round(x * 2**32))


def _log_tensor(env, t, name, asked, shape, dtype):
    if t is None:
        raise ValueError(f'the rollout must have logged its {asked}: log=("{asked}", ...)')
    if tuple(t.shape) != shape:
        raise ValueError(f"the rollout's {name} {tuple(t.shape)} is not {list(shape)} of this environment")
    if t.device != env.device:
        raise ValueError(f"the rollout lives on {t.device}, the environment on {env.device}")
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"the rollout's {name} must be contiguous {dtype}")
    return t


def trajectory_vtrace(env, rollout, logits=None, values=None, last_value=None, gamma=0.99, lam=1.0, rho_bar=1.0, c_bar=1.0, select="sample",
                      epsilon=0.0, beta=0.0, reward=None):
    """VecTilerSliderEnv.trajectory_vtrace: see there."""
    from ._cabi import State
    from .vec_env import _ptr
    w = RewardWeights() if reward is None else reward
    if not isinstance(w, RewardWeights):
        raise TypeError(f"reward must be a RewardWeights, got {type(w)}")
    w = RewardWeights(*(float(x) for x in w))
    gamma, lam, rho_bar, c_bar = float(gamma), float(lam), float(rho_bar), float(c_bar)
    if not (0.0 <= gamma <= 1.0 and 0.0 <= lam <= 1.0):
        raise ValueError("gamma and lam must be 0..1")
    if not (rho_bar >= 0.0 and c_bar >= 0.0):
        raise ValueError("rho_bar and c_bar must be >= 0 (inf: no clipping)")
    if select not in pc.SELECTS:
        raise ValueError(f"select must be one of {sorted(pc.SELECTS)}, got {select!r}")
    eps_t, beta_t = _threshold(epsilon, "epsilon"), _threshold(beta, "beta")
    if not vc.vtrace_supported(env._dims):
        from ._rollout_cabi import ROLLOUT_MAX_SIZE, ROLLOUT_MAX_TILES
        raise ValueError(f"trajectory_vtrace() covers boards up to {ROLLOUT_MAX_SIZE}x{ROLLOUT_MAX_SIZE} with at most {ROLLOUT_MAX_TILES} tiles "
                         f"and {ROLLOUT_MAX_TILES} targets; {env.size}x{env.size} with {env.n_tiles} tiles and {env.n_targets} targets is beyond that")
    cells, progress = w.dist != 0.0 or w.progress != 0.0, w.progress != 0.0
    steps, start, pos_log, flags_log = _check_rollout(env, rollout, True, cells, progress)
    N = env.num_envs
    act_log = _log_tensor(env, rollout.act_log, "act_log", "act", (steps, N), torch.uint8)
    mu_logits = _log_tensor(env, rollout.logits_log, "logits_log", "logits", (steps, N, 4), torch.float32)
    expert_log = None
    if beta_t:
        if rollout.expert_log is None:
            raise ValueError('beta > 0 needs the expert\'s moves: the rollout must have logged them, log=("expert", ...)')
        expert_log = _log_tensor(env, rollout.expert_log, "expert_log", "expert", (steps, N), torch.uint8)
    if logits is not None:
        if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.device != env.device or tuple(logits.shape) != (steps, N, 4):
            raise ValueError(f"logits must be a float32 tensor of shape [{steps}, {N}, 4] on {env.device}")
        logits = logits.detach().contiguous()
    values, stride = _values(env, values, steps)
    if last_value is not None:
        if not isinstance(last_value, torch.Tensor) or last_value.dtype != torch.float32 or last_value.device != env.device or tuple(last_value.shape) != (N,):
            raise ValueError(f"last_value must be a float32 tensor of shape [{N}] on {env.device}")
        last_value = last_value.detach().contiguous()
    out = torch.empty((5, steps, N), dtype=torch.float32, device=env.device)
    mask = torch.empty((steps, N), dtype=torch.uint8, device=env.device)
    if N:
        tin = vc.VtraceIn(_ptr(start), _ptr(pos_log), _ptr(flags_log), _ptr(values), _ptr(last_value), steps, stride, gamma, lam, *w,
                          _ptr(act_log), _ptr(expert_log), _ptr(mu_logits), _ptr(logits), pc.SELECTS[select], 0, eps_t, beta_t, rho_bar, c_bar)
        tout = vc.VtraceOut(_ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), _ptr(out[4]), _ptr(mask))
        st = State(None, None, _ptr(env._tgt), _ptr(env._blk), None, None, None)
        env._call("ts_traj_vtrace", C.byref(env._dims), C.byref(st), C.byref(tin), C.byref(tout), binding=vc)
    return VtraceTargets(out[0], out[1], out[2], mask.view(torch.bool), out[3], out[4])
