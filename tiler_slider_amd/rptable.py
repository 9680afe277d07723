"""Reach policy tables (lib/libtiler_slider_rptable.so, include/tiler_slider_rptable.h): build_policy_table(), walk_actions() and
score_policy() on the shapes beyond the dense tables' index space - a network's greedy play on every state of a ReachTable,
exactly, and its integer score against that table.

VecTilerSliderEnv.build_policy_table(..., table=rt), walk_actions(..., table=rt) and score_policy() of a ReachPolicyTable are thin
wrappers around the three functions at the bottom.  There is no CPU path and no torch fallback: the tables come from
k_rptable_actions / k_rptable_walk / k_rptable_score or from nowhere.
"""
import ctypes as C

import torch

from . import _rptable_cabi as xc
from .policy import MlpPolicy
from .ptable import PolicyScore, _depth
from .vec_env import ReachTable, _ptr


class ReachPolicyTable(ReachTable):
    """What VecTilerSliderEnv.build_policy_table(..., table=rt) and walk_actions(..., table=rt) return: a ReachTable - lookup(),
    lookup_bits(), build_reach_index() and through that place_at_distance() take it unchanged - whose `table` int64 [L, slots]
    holds, in the slots of rt's states, the number of moves the POLICY needs from each (1 .. 252), TABLE_DEEP (not won within
    max_depth) or TABLE_NONE (greedy play never wins from there); `count` is rt's own tensor; `root_moves` int16 [L] and
    `deepest` int32 [L] are the policy's; `act` uint8 [L, slots] is the policy's move on each state's slot, 255 on every other
    slot; `logits` float32 [L, slots, 4] the values the moves were chosen from, or None."""

    def __init__(self, table, source, root_moves, deepest, act, logits, max_depth):
        super().__init__(table, source.count, root_moves, deepest, source.capacity, source.size, source.n_tiles, source.n_targets,
                         source.multi_color, max_depth, source.root)
        self.act, self.logits = act, logits

    def actions(self, level):
        """(keys int64 [count] ascending, act uint8 [count]) of one level: the companion of entries(level).  Both empty for a FULL
        level."""
        row, act = self.table[level], self.act[level]
        if int(self.count[level]) < 0:
            row, act = row[:0], act[:0]
        live = row < 0
        keys, order = torch.sort(row[live] & ((1 << 48) - 1))
        return keys, act[live][order]

    def __repr__(self):
        return f"ReachPolicyTable({len(self)} levels x {self.slots} slots, capacity {self.capacity}, root {self.root!r})"


def _check(env, table, hidden=1):
    """The ReachTable of a reach policy call, validated against the environment: one row per board, its shape and device."""
    env._require_open()
    if env.host_mapped:
        raise ValueError("policy tables need device buffers (host_mapped=False)")
    n_rows = env._check_reach_table_itself(table)
    if not xc.rptable_supported(env._dims, hidden):
        raise ValueError(f"reach policy tables cover boards up to 8x8 with at most 8 tiles and 8 targets, and hidden widths 1 .. 64; "
                         f"{env.size}x{env.size} with {env.n_tiles} tiles, {env.n_targets} targets and {hidden} hidden units is beyond that")
    if n_rows != env.num_envs:
        raise ValueError(f"the table has {n_rows} levels for {env.num_envs} boards: a policy table is built on the environment of the table's levels")
    if not (table.table.is_contiguous() and table.count.is_contiguous()):
        raise ValueError("the table must be contiguous: the kernels read it in place")
    return n_rows


def _room(L, slots, per_slot, max_bytes):
    nbytes = L * slots * per_slot
    if nbytes > int(max_bytes):
        raise ValueError(f"reach policy tables of {L} levels x {slots} slots take {nbytes} bytes, above max_bytes = {int(max_bytes)}: "
                         "build them on an environment of the distinct levels and pass rows= to the lookups")


def _walk(env, rt, act, logits, max_depth):
    L, slots = len(rt), rt.slots
    table = torch.empty((L, slots), dtype=torch.int64, device=env.device)
    root_moves = torch.empty(L, dtype=torch.int16, device=env.device)
    deepest = torch.empty(L, dtype=torch.int32, device=env.device)
    if L:
        cfg = xc.RptableCfg(max_depth, xc.ROOTS[rt.root])
        out = xc.RptableOut(_ptr(table), _ptr(root_moves), _ptr(deepest))
        env._call("ts_rptable_walk", C.byref(env._dims), C.byref(env._state), _ptr(rt.table), slots, _ptr(rt.count), _ptr(act), C.byref(cfg),
                  C.byref(out), binding=xc)
    return ReachPolicyTable(table, rt, root_moves, deepest, act, logits, max_depth)


def build_policy_table(env, policy, table, max_depth=252, max_bytes=4 << 30, logits=False):
    """VecTilerSliderEnv.build_policy_table(..., table=rt): see there."""
    if not isinstance(policy, MlpPolicy) and callable(getattr(policy, "policy", None)):
        policy = policy.policy()  # a PolicyNet or an ActorCriticNet: its parameters, shared
    if not isinstance(policy, MlpPolicy):
        raise TypeError(f"policy must be an MlpPolicy, a PolicyNet or an ActorCriticNet, got {type(policy)}")
    L = _check(env, table, policy.hidden)
    max_depth = _depth(max_depth)
    mlp = policy._mlp(env)
    slots = table.slots
    _room(L, slots, 25 if logits else 9, max_bytes)
    act = torch.empty((L, slots), dtype=torch.uint8, device=env.device)
    z = torch.empty((L, slots, 4), dtype=torch.float32, device=env.device) if logits else None
    if L:
        env._call("ts_rptable_actions", C.byref(env._dims), C.byref(env._state), C.byref(mlp), _ptr(table.table), slots, _ptr(table.count),
                  _ptr(act), _ptr(z), binding=xc)
    return _walk(env, table, act, z, max_depth)


def walk_actions(env, act, table, max_depth=252, max_bytes=4 << 30):
    """VecTilerSliderEnv.walk_actions(..., table=rt): see there."""
    L = _check(env, table)
    max_depth = _depth(max_depth)
    if not (isinstance(act, torch.Tensor) and act.dtype == torch.uint8):
        raise TypeError(f"act must be a uint8 tensor, got {type(act)}{'' if not isinstance(act, torch.Tensor) else ' of ' + str(act.dtype)}")
    if tuple(act.shape) != (L, table.slots) or act.device != env.device or not act.is_contiguous():
        raise ValueError(f"act must be a contiguous uint8 tensor of shape ({L}, {table.slots}) on {env.device}")
    _room(L, table.slots, 9, max_bytes)
    return _walk(env, table, act, None, max_depth)


def score_policy(env, ptable, table):
    """VecTilerSliderEnv.score_policy() of a ReachPolicyTable: see there."""
    if not isinstance(table, ReachTable):
        raise TypeError(f"a ReachPolicyTable is scored against the ReachTable of its levels (build_reach_table()), got {type(table)}")
    L = _check(env, table)
    _check(env, ptable)
    if ptable.slots != table.slots:
        raise ValueError(f"the policy table has {ptable.slots} slots a level, the table {table.slots}: score a policy table against the table it was built on")
    act = ptable.act
    if tuple(act.shape) != (L, table.slots) or act.device != env.device or act.dtype != torch.uint8 or not act.is_contiguous():
        raise ValueError(f"ptable.act must be a contiguous uint8 tensor of shape ({L}, {table.slots}) on {env.device}")
    score = torch.empty((L, xc.SCORE_COLUMNS), dtype=torch.int32, device=env.device)
    if L:
        env._call("ts_rptable_score", C.byref(env._dims), C.byref(env._state), _ptr(ptable.table), _ptr(act), _ptr(table.table), table.slots,
                  _ptr(table.count), _ptr(score), binding=xc)
    return PolicyScore(score)
