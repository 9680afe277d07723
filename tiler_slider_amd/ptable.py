"""Policy tables (lib/libtiler_slider_ptable.so, include/tiler_slider_ptable.h): a network's greedy play on every placement of
every level, exactly, and its integer score against the optimal distance table.

VecTilerSliderEnv.build_policy_table(), walk_actions() and score_policy() are thin wrappers around the three functions at the
bottom.  There is no CPU path and no torch fallback: the tables come from k_ptable_actions / k_ptable_walk_* / k_ptable_score or
from nowhere.
"""
import ctypes as C

import torch

from . import _ptable_cabi as xc
from .policy import MlpPolicy
from .vec_env import DistanceTable, _ptr


class PolicyTable(DistanceTable):
    """What VecTilerSliderEnv.build_policy_table() and walk_actions() return: a DistanceTable - every call that takes one takes it -
    whose `dist` uint8 [L, states] is the number of moves the POLICY needs from each placement (0 .. 252), TABLE_INVALID,
    TABLE_DEEP (not won within max_depth) or TABLE_NONE (greedy play never wins from there); `act` uint8 [L, states] is the
    policy's move on each placement, 255 on an invalid one; `logits` float32 [L, states, 4] the values the moves were chosen
    from, or None."""

    def __init__(self, dist, act, logits, size, n_tiles, n_targets, multi_color, max_depth):
        super().__init__(dist, size, n_tiles, n_targets, multi_color, max_depth)
        self.act, self.logits = act, logits


class PolicyScore:
    """What VecTilerSliderEnv.score_policy() returns (include/tiler_slider_ptable.h: ts_ptable_score): eight int32 [L] device
    tensors - views of `columns` int32 [L, 8] - by name, counted over each level's valid placements:
        valid, solvable (the optimal table has a distance >= 1), solved (the policy table has one), optimal (solved in the least
        number of moves), agree (the policy's move is one of the expert's), excess (moves beyond the optimum, summed over what is
        both solved and solvable), deep (cut at max_depth), won (distance 0)
    and three 0-dim device tensors over all levels, computed on first use without a synchronisation:
        solved_share = solved / solvable, optimal_share = optimal / solvable, agreement = agree / solvable."""
    NAMES = ("valid", "solvable", "solved", "optimal", "agree", "excess", "deep", "won")

    def __init__(self, columns):
        self.columns = columns
        for k, name in enumerate(self.NAMES):
            setattr(self, name, columns[:, k])
        self._shares = {}

    def _share(self, name):
        if name not in self._shares:
            total = self.columns.sum(dim=0, dtype=torch.int64)
            self._shares[name] = total[self.NAMES.index(name)].double() / total[1].clamp(min=1).double()
        return self._shares[name]

    @property
    def solved_share(self):
        return self._share("solved")

    @property
    def optimal_share(self):
        return self._share("optimal")

    @property
    def agreement(self):
        return self._share("agree")

    def __repr__(self):
        return f"PolicyScore({', '.join(self.NAMES)}: [{self.columns.shape[0]}])"


def _states(env, hidden=1):
    env._require_open()
    if env.host_mapped:
        raise ValueError("policy tables need device buffers (host_mapped=False)")
    if not xc.ptable_supported(env._dims, hidden):
        raise ValueError(f"policy tables cover boards up to 8x8 with at most 8 targets whose index space (size * size) ** n_tiles is at most "
                         f"65536, and hidden widths 1 .. 64; {env.size}x{env.size} with {env.n_tiles} tiles, {env.n_targets} targets and "
                         f"{hidden} hidden units is beyond that")
    return (env.size * env.size) ** env.n_tiles


def _depth(max_depth):
    from ._table_cabi import TABLE_MAX_DEPTH
    if not 0 <= int(max_depth) <= TABLE_MAX_DEPTH:
        raise ValueError(f"max_depth must be 0..{TABLE_MAX_DEPTH}")
    return int(max_depth)


def _room(env, states, per_placement, max_bytes):
    nbytes = env.num_envs * states * per_placement
    if nbytes > int(max_bytes):
        raise ValueError(f"policy tables of {env.num_envs} levels x {states} placements take {nbytes} bytes, above max_bytes = {int(max_bytes)}: "
                         "build them on an environment of the distinct levels and pass rows= to the lookups")


def _walk(env, act, max_depth, states):
    dist = torch.empty((env.num_envs, states), dtype=torch.uint8, device=env.device)
    if env.num_envs:
        env._call("ts_ptable_walk", C.byref(env._dims), C.byref(env._state), _ptr(act), max_depth, _ptr(dist), binding=xc)
    return dist


def build_policy_table(env, policy, max_depth=252, max_bytes=4 << 30, logits=False):
    """VecTilerSliderEnv.build_policy_table: see there."""
    if not isinstance(policy, MlpPolicy) and callable(getattr(policy, "policy", None)):
        policy = policy.policy()  # a PolicyNet or an ActorCriticNet: its parameters, shared
    if not isinstance(policy, MlpPolicy):
        raise TypeError(f"policy must be an MlpPolicy, a PolicyNet or an ActorCriticNet, got {type(policy)}")
    states = _states(env, policy.hidden)
    max_depth = _depth(max_depth)
    mlp = policy._mlp(env)
    _room(env, states, 18 if logits else 2, max_bytes)
    L = env.num_envs
    act = torch.empty((L, states), dtype=torch.uint8, device=env.device)
    z = torch.empty((L, states, 4), dtype=torch.float32, device=env.device) if logits else None
    if L:
        env._call("ts_ptable_actions", C.byref(env._dims), C.byref(env._state), C.byref(mlp), _ptr(act), _ptr(z), binding=xc)
    dist = _walk(env, act, max_depth, states)
    return PolicyTable(dist, act, z, env.size, env.n_tiles, env.n_targets, env.multi_color, max_depth)


def walk_actions(env, act, max_depth=252):
    """VecTilerSliderEnv.walk_actions: see there."""
    states = _states(env)
    max_depth = _depth(max_depth)
    if not (isinstance(act, torch.Tensor) and act.dtype == torch.uint8):
        raise TypeError(f"act must be a uint8 tensor, got {type(act)}{'' if not isinstance(act, torch.Tensor) else ' of ' + str(act.dtype)}")
    if tuple(act.shape) != (env.num_envs, states) or act.device != env.device or not act.is_contiguous():
        raise ValueError(f"act must be a contiguous uint8 tensor of shape ({env.num_envs}, {states}) on {env.device}")
    dist = _walk(env, act, max_depth, states)
    return PolicyTable(dist, act, None, env.size, env.n_tiles, env.n_targets, env.multi_color, max_depth)


def score_policy(env, ptable, table):
    """VecTilerSliderEnv.score_policy: see there."""
    states = _states(env)
    if not isinstance(ptable, PolicyTable):
        raise TypeError(f"ptable must be a PolicyTable (build_policy_table(), walk_actions()), got {type(ptable)}")
    dist, n_rows, _ = env._check_table(ptable, None)
    optimal, _, _ = env._check_table(table, None)
    act = ptable.act
    if tuple(act.shape) != (n_rows, states) or act.device != env.device or act.dtype != torch.uint8:
        raise ValueError(f"ptable.act must be uint8 of shape ({n_rows}, {states}) on {env.device}")
    if not (dist.is_contiguous() and act.is_contiguous() and optimal.is_contiguous()):
        raise ValueError("the tables must be contiguous: the kernel reads them in place")
    score = torch.empty((env.num_envs, xc.SCORE_COLUMNS), dtype=torch.int32, device=env.device)
    if env.num_envs:
        env._call("ts_ptable_score", C.byref(env._dims), C.byref(env._state), _ptr(dist), _ptr(act), _ptr(optimal), _ptr(score), binding=xc)
    return PolicyScore(score)
