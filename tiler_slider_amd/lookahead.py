"""Lookahead (lib/libtiler_slider_lookahead.so, include/tiler_slider_lookahead.h): a network's values backed up through a
full-width search of the exact environment.

lookahead() is one k_lookahead launch over the boards as they stand or over every board a logged rollout visited: the four
backed-up action values, their maximum, the move that attains it and the plies to the nearest win within the horizon.  The
results are targets - search-improved moves for step(), labels for trajectory_loss(labels=), TD / Q-learning targets - and carry
no grad_fn.  There is no CPU path and no torch fallback.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _lookahead_cabi as lc
from .targets import RewardWeights

Lookahead = namedtuple("Lookahead", ("q", "value", "best", "win_in"))
Lookahead.__doc__ = """q float32 [..., 4]: the backed-up value of each action; value float32 [...]: their maximum; best uint8 [...]: the lowest
action that attains it, 255 on a board that is already won (what step() leaves alone and trajectory_loss(labels=) reads as no
sample); win_in uint8 [...]: the least number of plies within the depth after which some action sequence has won, 0 if none.
[...] is [N] for the boards as they stand and [K, N] for a rollout's."""


def _network(net, leaf):
    """(MlpPolicy or None, (wv, bv) or None, leaf name) of lookahead()'s `net` and `leaf`."""
    from .actor_critic import ActorCriticNet
    from .policy import MlpPolicy
    from .train import PolicyNet
    if net is None:
        default, kinds = "zero", ("zero",)
    elif isinstance(net, ActorCriticNet):
        default, kinds = "value", ("value", "qmax", "zero")
    elif isinstance(net, (PolicyNet, MlpPolicy)):
        default, kinds = "qmax", ("qmax", "zero")
    else:
        raise TypeError(f"net must be an ActorCriticNet, a PolicyNet, an MlpPolicy or None, got {type(net)}")
    leaf = default if leaf is None else leaf
    if leaf not in lc.LEAVES:
        raise ValueError(f"leaf must be one of {sorted(lc.LEAVES)}, got {leaf!r}")
    if leaf not in kinds:
        raise ValueError(f'leaf "{leaf}" needs ' + ("an ActorCriticNet: a PolicyNet has no value head" if leaf == "value" else "a network")
                         + f", got {type(net).__name__}")
    if leaf == "zero":
        return None, None, leaf
    policy = net if isinstance(net, MlpPolicy) else net.policy()
    head = (net.wv.detach(), net.bv.detach()) if leaf == "value" else None
    return policy, head, leaf


def lookahead(env, net, depth=2, rollout=None, leaf=None, gamma=1.0, reward=None):
    """VecTilerSliderEnv.lookahead: see there."""
    from ._cabi import State
    from .policy import _prepare
    from .train import _trajectory_cells
    from .vec_env import _ptr
    policy, head, leaf = _network(net, leaf)
    depth, gamma = int(depth), float(gamma)
    if not 1 <= depth <= lc.MAX_DEPTH:
        raise ValueError(f"depth must be 1..{lc.MAX_DEPTH}, got {depth}")
    if not 0.0 <= gamma <= 1.0:
        raise ValueError("gamma must be 0..1")
    w = RewardWeights() if reward is None else reward
    if not isinstance(w, RewardWeights):
        raise TypeError(f"reward must be a RewardWeights, got {type(w)}")
    w = RewardWeights(*(float(x) for x in w))
    for field in ("timeout", "dist", "progress"):
        if getattr(w, field) != 0.0:
            raise ValueError(f"the search does not model reward.{field} (the step count and the Manhattan terms are outside it): it must be 0, "
                             f"got {getattr(w, field)}")
    if policy is not None:
        mlp = _prepare(env, policy)  # the environment, the shape, the width, the features and the device
    else:
        env._require_open()
        if not env._started:
            raise RuntimeError("Call reset() before a lookahead.")
        if env.host_mapped:
            raise ValueError("lookahead needs device buffers (host_mapped=False)")
        if not lc.lookahead_supported(env._dims, 1, lc.LEAVES["zero"]):
            from ._rollout_cabi import ROLLOUT_MAX_SIZE, ROLLOUT_MAX_TILES
            raise ValueError(f"lookahead searches boards up to {ROLLOUT_MAX_SIZE}x{ROLLOUT_MAX_SIZE} with at most {ROLLOUT_MAX_TILES} tiles and "
                             f"{ROLLOUT_MAX_TILES} targets; {env.size}x{env.size} with {env.n_tiles} tiles and {env.n_targets} targets is beyond that")
        mlp = None
    first, pos_log, steps = _trajectory_cells(env, rollout)
    N = env.num_envs
    q = torch.empty((steps, N, 4), dtype=torch.float32, device=env.device)
    value = torch.empty((steps, N), dtype=torch.float32, device=env.device)
    best = torch.empty((steps, N), dtype=torch.uint8, device=env.device)
    win_in = torch.empty((steps, N), dtype=torch.uint8, device=env.device)
    if N:
        vh = lc.ValueHead(head[0].data_ptr(), head[1].data_ptr()) if head is not None else None
        tin = lc.TrainIn(_ptr(first), _ptr(pos_log), steps, 0)
        cfg = lc.LookaheadCfg(depth, lc.LEAVES[leaf], gamma, w.step, w.win, w.invalid)
        out = lc.LookaheadOut(q.data_ptr(), value.data_ptr(), best.data_ptr(), win_in.data_ptr())
        st = State(None, None, _ptr(env._tgt), _ptr(env._blk), None, None, None)
        env._call("ts_lookahead", C.byref(env._dims), C.byref(st), C.byref(mlp) if mlp is not None else None,
                  C.byref(vh) if vh is not None else None, C.byref(tin), C.byref(cfg), C.byref(out), binding=lc)
    if rollout is None:
        return Lookahead(q[0], value[0], best[0], win_in[0])
    return Lookahead(q, value, best, win_in)
