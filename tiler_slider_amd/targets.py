"""Trajectory targets (lib/libtiler_slider_targets.so, include/tiler_slider_targets.h): what a loss over a logged rollout is
computed against.

trajectory_returns() is one k_traj_returns launch over a Rollout's flags_log (and pos_log, where the reward looks at the cells):
per-step rewards, GAE(gamma, lambda) advantages, returns and the mask of the steps that played a transition.
trajectory_labels() is one k_traj_labels launch: the answer of a DistanceTable on every board the rollout visited.  There is no
CPU path and no torch fallback.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _targets_cabi as gc

RewardWeights = namedtuple("RewardWeights", ("step", "win", "timeout", "invalid", "dist", "progress"), defaults=(0.0, 1.0, 0.0, 0.0, 0.0, 0.0))
RewardWeights.__doc__ = """The six weights of include/tiler_slider_targets.h's r_k: a constant per played step, SUCCESS, TIMEOUT, INVALID_MOVE,
the Manhattan reward m() of the cells after the step, and its plain difference m(after) - m(before).  Default: 1 for a win."""

TrajectoryReturns = namedtuple("TrajectoryReturns", ("reward", "adv", "ret", "mask"))
TrajectoryReturns.__doc__ = """reward, adv, ret float32 [K, N]; mask bool [K, N]: False where the step played no transition (the board was
done on entry, or the action byte was no move) - reward, adv and ret are 0 there."""


def _check_rollout(env, rollout, need_flags, need_pos, need_start):
    """The rollout's logs, validated against the environment: (steps, start_pos, pos_log, flags_log), None where not needed."""
    from .vec_env import Rollout
    env._require_open()
    if env.host_mapped:
        raise ValueError("trajectory targets need device buffers (host_mapped=False)")
    if not isinstance(rollout, Rollout):
        raise TypeError(f"rollout must be a Rollout (rollout(..., log=...) or rollout_policy(..., log=...)), got {type(rollout)}")
    T, N = env.n_tiles, env.num_envs
    flags, pos, start = rollout.flags_log, rollout.pos_log, rollout.start_pos
    if need_flags and flags is None:
        raise ValueError('the rollout must have logged its flags: log=("flags", ...)')
    if need_pos and pos is None:
        raise ValueError('the rollout must have logged its cells: log=("pos", ...)')
    if need_start and start is None:
        raise ValueError('the rollout must have logged its start: log=("start", ...)')
    lead = flags if need_flags else pos
    steps = int(lead.shape[0]) if lead.dim() >= 1 else -1
    if steps < 1:
        raise ValueError("the rollout has no step")
    want = {"flags_log": (flags if need_flags else None, (steps, N), torch.uint8),
            "pos_log": (pos if need_pos else None, (steps, T, N), env._pos.dtype),
            "start_pos": (start if need_start else None, (T, N), env._pos.dtype)}
    for name, (t, shape, dtype) in want.items():
        if t is None:
            continue
        if tuple(t.shape) != shape:
            raise ValueError(f"the rollout's {name} {tuple(t.shape)} is not {list(shape)} of this environment")
        if t.device != env.device:
            raise ValueError(f"the rollout lives on {t.device}, the environment on {env.device}")
        if t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"the rollout's {name} must be contiguous {dtype}")
    return steps, want["start_pos"][0], want["pos_log"][0], want["flags_log"][0]


def _values(env, values, steps):
    """(tensor or None, stride): float32 [K, N], contiguous (1) or column c of a contiguous [K, N, 4] tensor (4), read in place."""
    if values is None:
        return None, 1
    N = env.num_envs
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.device != env.device or tuple(values.shape) != (steps, N):
        raise ValueError(f"values must be a float32 tensor of shape [{steps}, {N}] on {env.device}")
    values = values.detach()
    if values.is_contiguous():
        return values, 1
    if tuple(values.stride()) == (4 * N, 4):
        return values, 4
    raise ValueError(f"values must be contiguous, or a column view of a contiguous [{steps}, {N}, 4] tensor (strides ({4 * N}, 4)); "
                     f"got strides {tuple(values.stride())}")


def trajectory_returns(env, rollout, gamma=0.99, lam=1.0, values=None, last_value=None, reward=None):
    """VecTilerSliderEnv.trajectory_returns: see there."""
    from ._cabi import State
    from .vec_env import _ptr
    w = RewardWeights() if reward is None else reward
    if not isinstance(w, RewardWeights):
        raise TypeError(f"reward must be a RewardWeights, got {type(w)}")
    w = RewardWeights(*(float(x) for x in w))
    gamma, lam = float(gamma), float(lam)
    if not (0.0 <= gamma <= 1.0 and 0.0 <= lam <= 1.0):
        raise ValueError("gamma and lam must be 0..1")
    if not gc.targets_supported(env._dims, gc.RETURNS):
        from ._rollout_cabi import ROLLOUT_MAX_SIZE, ROLLOUT_MAX_TILES
        raise ValueError(f"trajectory_returns() covers boards up to {ROLLOUT_MAX_SIZE}x{ROLLOUT_MAX_SIZE} with at most {ROLLOUT_MAX_TILES} tiles "
                         f"and {ROLLOUT_MAX_TILES} targets; {env.size}x{env.size} with {env.n_tiles} tiles and {env.n_targets} targets is beyond that")
    cells, progress = w.dist != 0.0 or w.progress != 0.0, w.progress != 0.0
    steps, start, pos_log, flags_log = _check_rollout(env, rollout, True, cells, progress)
    N = env.num_envs
    values, stride = _values(env, values, steps)
    if last_value is not None:
        if not isinstance(last_value, torch.Tensor) or last_value.dtype != torch.float32 or last_value.device != env.device or tuple(last_value.shape) != (N,):
            raise ValueError(f"last_value must be a float32 tensor of shape [{N}] on {env.device}")
        last_value = last_value.detach().contiguous()
    out = torch.empty((3, steps, N), dtype=torch.float32, device=env.device)
    mask = torch.empty((steps, N), dtype=torch.uint8, device=env.device)
    if N:
        tin = gc.ReturnsIn(_ptr(start), _ptr(pos_log), _ptr(flags_log), _ptr(values), _ptr(last_value), steps, stride, gamma, lam, *w)
        tout = gc.ReturnsOut(_ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(mask))
        st = State(None, None, _ptr(env._tgt), _ptr(env._blk), None, None, None)
        env._call("ts_traj_returns", C.byref(env._dims), C.byref(st), C.byref(tin), C.byref(tout), binding=gc)
    return TrajectoryReturns(out[0], out[1], out[2], mask.view(torch.bool))


def trajectory_labels(env, rollout, table, rows=None):
    """VecTilerSliderEnv.trajectory_labels: see there."""
    from ._cabi import State
    from .vec_env import _ptr
    steps, start, pos_log, _ = _check_rollout(env, rollout, False, True, True)
    dist, n_rows, rows = env._check_table(table, rows)
    N = env.num_envs
    moves = torch.empty((steps, N), dtype=torch.int16, device=env.device)
    best = torch.empty((steps, N), dtype=torch.uint8, device=env.device)
    action = torch.empty((steps, N), dtype=torch.uint8, device=env.device)
    if N:
        tin = gc.LabelsIn(_ptr(start), _ptr(pos_log), _ptr(dist), _ptr(rows), n_rows, steps, 0)
        tout = gc.LabelsOut(_ptr(moves), _ptr(best), _ptr(action))
        st = State(None, None, None, _ptr(env._blk), None, None, None)
        env._call("ts_traj_labels", C.byref(env._dims), C.byref(st), C.byref(tin), C.byref(tout), binding=gc)
    return moves, best, action
