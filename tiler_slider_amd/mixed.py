"""Mixed rollouts (lib/libtiler_slider_mixed.so, include/tiler_slider_mixed.h): K steps in one launch in which a network and a
table expert share the play - DAgger's behaviour policy - with the table's answer on every board visited logged on the way.

rollout_mixed() is VecTilerSliderEnv.rollout_policy(expert=...): one k_mixed_rollout launch on a DistanceTable or a ReachTable
(PolicyTable and ReachPolicyTable are those).  There is no CPU path and no torch fallback.
"""
import ctypes as C

import torch

from . import _mixed_cabi as mc
from . import _policy_cabi as pc

EXPERT_LOGS = ("expert", "moves", "best", "who")


def rollout_mixed(env, steps, policy, expert, beta=0.0, rows=None, select="sample", epsilon=0.0, seed=0, step_index=0, board_offset=0, stats=True,
                  log=(), advance=True):
    """VecTilerSliderEnv.rollout_policy(expert=...): see there."""
    from ._rollout_cabi import ROLLOUT_MAX_STEPS
    from .policy import _prepare
    from .vec_env import ReachTable, Rollout, _ptr
    mlp = _prepare(env, policy)
    if select not in pc.SELECTS:
        raise ValueError(f"select must be one of {sorted(pc.SELECTS)}, got {select!r}")
    steps = int(steps)
    if not 0 <= steps <= ROLLOUT_MAX_STEPS:
        raise ValueError(f"steps must be 0..{ROLLOUT_MAX_STEPS}")
    if not 0.0 <= float(epsilon) <= 1.0:
        raise ValueError("epsilon must be 0..1")
    if not 0.0 <= float(beta) <= 1.0:
        raise ValueError("beta must be 0..1")
    N = env.num_envs
    cfg = mc.MixedCfg(steps, env._mode, pc.SELECTS[select], 1 if advance else 0, int(seed) & (2**64 - 1), int(step_index), int(board_offset),
                      int(round(float(epsilon) * 2**32)), int(round(float(beta) * 2**32)))
    if isinstance(expert, ReachTable):
        n_rows, rows = env._check_reach_table(expert, rows)
        cfg.kind, cfg.table, cfg.slots, cfg.count = mc.REACH, _ptr(expert.table), expert.slots, _ptr(expert.count)
    else:
        dist, n_rows, rows = env._check_table(expert, rows)
        cfg.kind, cfg.dense = mc.DENSE, _ptr(dist)
    cfg.n_rows, cfg.rows = n_rows, _ptr(rows)
    names = env._ROLLOUT_STATS if stats is True else () if not stats else tuple(stats)
    logs = (log,) if isinstance(log, str) else tuple(log)
    all_logs = env._ROLLOUT_LOGS + ("logits", "start") + EXPERT_LOGS
    if set(names) - set(env._ROLLOUT_STATS) or set(logs) - set(all_logs):
        raise ValueError(f"stats are {env._ROLLOUT_STATS}, logs {all_logs}")
    got = {name: torch.zeros(N, dtype=torch.uint8 if name == "flags" else torch.int32, device=env.device) for name in names}
    for name in logs:
        if name == "start":
            continue
        shape = {"pos": (steps, env.n_tiles, N), "logits": (steps, N, 4)}.get(name, (steps, N))
        dtype = env._pos.dtype if name == "pos" else torch.float32 if name == "logits" else torch.int16 if name == "moves" else torch.uint8
        got[name + "_log"] = torch.zeros(shape, dtype=dtype, device=env.device)
    bound = dict(got)
    if advance:  # the environment's own flag byte becomes the last step's, as after step(); a Rollout's `flags` is then that tensor
        bound["flags"] = env._flags
        if "flags" in got:
            got["flags"] = env._flags
    out = mc.MixedOut(*(_ptr(bound.get(f)) for f in mc.OUT_FIELDS))
    if "start" in logs:  # the cells before the launch: with advance=True the launch overwrites the only other copy
        got["start_pos"] = env._pos.clone()
    if steps and N and bound:
        env._call("ts_mixed_rollout", C.byref(env._dims), C.byref(env._state), C.byref(mlp), C.byref(cfg), C.byref(out), binding=mc)
        if advance and env.obs_dtype is not None:  # one encode into the current buffer: env._obs stays truthful
            env._call("ts_encode" if env.obs_dtype == torch.float32 else "ts_encode_u8", C.byref(env._dims), C.byref(env._state), _ptr(env._obs))
            env._sync_shown()
    return Rollout(steps, **got)
