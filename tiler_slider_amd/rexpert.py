"""Reach-table experts (lib/libtiler_slider_rexpert.so, include/tiler_slider_rexpert.h): the two consumers of a ReachTable that an
imitation loop needs on shapes beyond the dense tables' index space.

rollout_reach() is one k_rexpert_rollout launch: K steps of the epsilon-greedy expert of a ReachTable, with every output
rollout("table") gives.  trajectory_labels_reach() is one k_rexpert_labels launch: the table's answer on every board a Rollout
visited.  There is no CPU path and no torch fallback.
"""
import ctypes as C

import torch

from . import _rexpert_cabi as ec


def _require_shape(env):
    if not ec.rexpert_supported(env._dims):
        raise ValueError(f"reach-table experts play boards up to {ec.ROLLOUT_MAX_SIZE}x{ec.ROLLOUT_MAX_SIZE} with at most {ec.ROLLOUT_MAX_TILES} tiles and "
                         f"{ec.ROLLOUT_MAX_TILES} targets; {env.size}x{env.size} with {env.n_tiles} tiles and {env.n_targets} targets is beyond that")


def rollout_reach(env, steps, table, rows=None, epsilon=0.0, seed=0, step_index=0, board_offset=0, stats=True, log=(), advance=True):
    """VecTilerSliderEnv.rollout(policy="reach"): see there."""
    from .vec_env import Rollout, _ptr
    env._require_open()
    if not env._started:
        raise RuntimeError("Call reset() before rollout().")
    if env.host_mapped:
        raise ValueError("rollout needs device buffers (host_mapped=False)")
    _require_shape(env)
    steps = int(steps)
    if not 0 <= steps <= ec.ROLLOUT_MAX_STEPS:
        raise ValueError(f"steps must be 0..{ec.ROLLOUT_MAX_STEPS}")
    if not 0.0 <= float(epsilon) <= 1.0:
        raise ValueError("epsilon must be 0..1")
    n_rows, rows = env._check_reach_table(table, rows)
    N = env.num_envs
    cfg = ec.RexpertCfg(steps, env._mode, 1 if advance else 0, 0, int(seed) & (2**64 - 1), int(step_index), int(board_offset),
                        int(round(float(epsilon) * 2**32)), _ptr(table.table), table.slots, _ptr(table.count), n_rows, _ptr(rows))
    names = env._ROLLOUT_STATS if stats is True else () if not stats else tuple(stats)
    logs = (log,) if isinstance(log, str) else tuple(log)
    if set(names) - set(env._ROLLOUT_STATS) or set(logs) - set(env._ROLLOUT_LOGS + env._ROLLOUT_START):
        raise ValueError(f"stats are {env._ROLLOUT_STATS}, logs {env._ROLLOUT_LOGS + env._ROLLOUT_START}")
    got = {name: torch.zeros(N, dtype=torch.uint8 if name == "flags" else torch.int32, device=env.device) for name in names}
    start_pos = env._pos.clone() if "start" in logs else None  # before the launch: with advance=True it overwrites the only other copy
    for name in logs:
        if name == "start":
            continue
        shape = (steps, env.n_tiles, N) if name == "pos" else (steps, N)
        got[name + "_log"] = torch.zeros(shape, dtype=env._pos.dtype if name == "pos" else torch.uint8, device=env.device)
    bound = dict(got)
    if advance:  # the environment's own flag byte becomes the last step's, as after step(); a Rollout's `flags` is then that tensor
        bound["flags"] = env._flags
        if "flags" in got:
            got["flags"] = env._flags
    out = ec.RolloutOut(*(_ptr(bound.get(f)) for f in ec.OUT_FIELDS))
    if steps and N and bound:
        env._call("ts_rexpert_rollout", C.byref(env._dims), C.byref(env._state), C.byref(cfg), C.byref(out), binding=ec)
        if advance and env.obs_dtype is not None:  # one encode into the current buffer: env._obs stays truthful
            env._call("ts_encode" if env.obs_dtype == torch.float32 else "ts_encode_u8", C.byref(env._dims), C.byref(env._state), _ptr(env._obs))
            env._sync_shown()
    return Rollout(steps, **got) if start_pos is None else Rollout(steps, start_pos=start_pos, **got)


def trajectory_labels_reach(env, rollout, table, rows=None):
    """VecTilerSliderEnv.trajectory_labels() of a ReachTable: see there."""
    from ._cabi import State
    from .targets import _check_rollout
    from .vec_env import _ptr
    steps, start, pos_log, _ = _check_rollout(env, rollout, False, True, True)
    _require_shape(env)
    n_rows, rows = env._check_reach_table(table, rows)
    N = env.num_envs
    moves = torch.empty((steps, N), dtype=torch.int16, device=env.device)
    best = torch.empty((steps, N), dtype=torch.uint8, device=env.device)
    action = torch.empty((steps, N), dtype=torch.uint8, device=env.device)
    if N:
        tin = ec.RexpertLabelsIn(_ptr(start), _ptr(pos_log), _ptr(table.table), _ptr(table.count), _ptr(rows), table.slots, n_rows, steps, 0)
        tout = ec.LabelsOut(_ptr(moves), _ptr(best), _ptr(action))
        st = State(None, None, _ptr(env._tgt), _ptr(env._blk), None, None, None)
        env._call("ts_rexpert_labels", C.byref(env._dims), C.byref(st), C.byref(tin), C.byref(tout), binding=ec)
    return moves, best, action
