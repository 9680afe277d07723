"""CPU yardstick of the mixed rollouts (test infrastructure, no test of its own): the definition of include/tiler_slider_mixed.h
restated on NumPy and the CPU oracle - policy_reference's logits_exact32 (integer weights) or float64 logits and its select,
table_reference.lookup / rtable_reference.lookup for the expert, rollout_reference's draws and mix64 for r and g,
OracleBatch.step(..., reward=True) for the step.  It shares no code with tiler_slider_amd/csrc/ts_mixed.hip: the reach table is
a Reference of sorted keys, not a hash table.  Imports neither torch nor the libraries at import time."""
import functools

import numpy as np

import policy_reference as pref
import rexpert_reference as rx
import rollout_reference as rref
import rtable_reference as rt
import table_reference as tref

DENSE, REACH = 0, 1
SALT = 0x6a09e667f3bcc909
WHO_NETWORK, WHO_EXPERT, WHO_RANDOM = 0, 1, 2
OUTPUTS = pref.OUTPUTS + ("expert_log", "moves_log", "best_log", "who_log")
STATS = ("wins", "finished", "first_win", "win_moves", "reward_sum", "flags")
OUT_DTYPES = dict(wins=np.int32, finished=np.int32, first_win=np.int32, win_moves=np.int32, reward_sum=np.int32, flags=np.uint8, act_log=np.uint8,
                  flags_log=np.uint8, pos_log=np.uint8, logits_log=np.float32, expert_log=np.uint8, moves_log=np.int16, best_log=np.uint8,
                  who_log=np.uint8)


def teach_of(r, beta_threshold):
    """teach of the definition: the low 32 bits of g = mix64(r ^ SALT) below beta * 2^32."""
    g = rref.mix64(np.asarray(r, np.uint64) ^ np.uint64(SALT))
    return (g & np.uint64(0xffffffff)) < np.uint64(beta_threshold)


def lookup(orc, kind, table, S, blk, tgt, pos, rows=None):
    """(moves int16, best uint8, action uint8) [N] of the boards on `pos`: `table` is uint8 [n_rows, states] (DENSE) or an
    rtable_reference.Reference (REACH)."""
    if kind == DENSE:
        return tref.lookup(orc, S, blk, pos, table, rows)
    return rt.lookup(orc, table, blk, tgt, pos, rows)


def rollout(orc, kind, table, S, mc, max_steps, blk, init, tgt, mlp, steps, select_mode, mode=0, *, pos=None, step_count=None, done=None,
            rows=None, threshold=0, beta=0, seed=0, step_index=0, board_offset=0, exact32=True, force_logits=None):
    """The loop of the definition from the state (pos, step_count, done) - default: freshly reset.  table=None: no table is read
    (beta must be 0), x is 255 everywhere and the three table logs are not returned.  force_logits [K, n, 4]: teacher forcing -
    the selection is made on these logits (a kernel's own), while `logits_log` still holds the yardstick's.  Returns the nine
    outputs, logits_log, the four logs, the state after, and what the run exercised: `who` int64 [3] board-steps by who played,
    `expert_differs` those of the expert's where x != e, `teach_no_move` board-steps with teach set, explore unset and x == 255,
    `kinds` int64 [5] (REACH: rexpert_reference.KINDS of the lookups), `wins`, `timeouts`, `resets` as counts of steps."""
    b = orc.OracleBatch(S, mc, max_steps, blk, init, tgt)
    n, T = b.n, b.n_tiles
    if pos is not None:
        b.pos[...] = pos
    if step_count is not None:
        b.step_count[...] = step_count
    if done is not None:
        b.done[...] = done
    assert table is not None or beta == 0
    out = {k: np.zeros(n, np.int32) for k in ("wins", "finished", "first_win", "win_moves", "reward_sum")}
    out["flags"] = np.zeros(n, np.uint8)
    for k in ("act_log", "flags_log", "expert_log", "best_log", "who_log"):
        out[k] = np.zeros((steps, n), np.uint8)
    out["moves_log"] = np.zeros((steps, n), np.int16)
    out["pos_log"] = np.zeros((steps, T, n), b.pos.dtype)
    out["logits_log"] = np.zeros((steps, n, 4), np.float32)
    who_count, kinds = np.zeros(3, np.int64), np.zeros(5, np.int64)
    differs = no_move = 0
    for k in range(steps):
        r = rref.draws(n, seed, step_index + k, board_offset)
        rnd = (r >> np.uint64(62)).astype(np.uint8)
        x1 = b.encode_onehot().reshape(n, -1)
        z = pref.logits_exact32(x1, mlp) if exact32 else pref.logits64(x1, mlp)[0].astype(np.float32)
        e = pref.select(z if force_logits is None else force_logits[k], r, select_mode)
        if table is None:
            m, bits, x = np.full(n, -1, np.int16), np.zeros(n, np.uint8), np.full(n, 255, np.uint8)
        else:
            m, bits, x = lookup(orc, kind, table, S, b.blk, b.tgt, b.pos, rows)
            if kind == REACH:
                kinds += rx.kinds_of(m)
        teach = teach_of(r, beta)
        explore = (r & np.uint64(0xffffffff)) < np.uint64(threshold)
        taught = teach & (x != 255)
        a = np.where(explore, rnd, np.where(taught, x, e)).astype(np.uint8)
        who = np.where(explore, WHO_RANDOM, np.where(taught, WHO_EXPERT, WHO_NETWORK)).astype(np.uint8)
        who_count += np.bincount(who, minlength=3)[:3]
        differs += int(((who == WHO_EXPERT) & (x != e)).sum())
        no_move += int((teach & ~explore & (x == 255)).sum())
        res = b.step(a, mode=mode, obs=False, reward=True)
        f = res["flags"]
        success = (f & rref.FLAG_SUCCESS) != 0
        out["wins"] += success
        out["finished"] += (f & (rref.FLAG_SUCCESS | rref.FLAG_TIMEOUT)) != 0
        out["first_win"] = np.where(success & (out["first_win"] == 0), k + 1, out["first_win"]).astype(np.int32)
        out["win_moves"] += np.where(success, b.step_count, 0).astype(np.int32)
        out["reward_sum"] += res["reward"]
        out["flags"] = f.copy()
        out["act_log"][k], out["flags_log"][k], out["pos_log"][k], out["logits_log"][k] = a, f, b.pos, z
        out["expert_log"][k], out["moves_log"][k], out["best_log"][k], out["who_log"][k] = x, m, bits, who
    out["pos"], out["step_count"], out["done"] = b.pos.copy(), b.step_count.copy(), b.done.copy()
    if table is None:
        for k in ("expert_log", "moves_log", "best_log"):
            del out[k]
    out["who"], out["expert_differs"], out["teach_no_move"], out["kinds"] = who_count, differs, no_move, kinds
    out["n_wins"] = int(out["wins"].sum())
    out["timeouts"] = int(((out["flags_log"] & rref.FLAG_TIMEOUT) != 0).sum())
    out["resets"] = int(((out["flags_log"] & rref.FLAG_AUTORESET) != 0).sum())
    return out


# ---- the base case (tests/test_gpu_mixed.py), its levels and the conditions asserted on the yardstick alone ----
BASE = dict(levels=128, steps=24, max_steps=12, beta=0.5, epsilon=0.125, seed=7, hidden=8)
# mode -> (select, kind of weights): strict with SAMPLE and logits that are multiples of 128, auto-reset with GREEDY
MODES = {0: (pref.SAMPLE, "int128"), 1: (pref.GREEDY, "int")}
REACH_SIZES = (2, 3, 4, 5, 6, 7, 8)
DENSE_SHAPES = ((2, 2, 0), (3, 2, 1), (4, 2, 2), (5, 2, 3), (6, 2, 4), (7, 2, 6), (8, 2, 8), (4, 4, 2), (6, 3, 4))   # (S, T, obstacles)
FLOORS = dict(expert=15, expert_differs=15, random=300, network=2000, teach_no_move=500, wins=5, timeouts=25, resets=150, kinds=50)


def features(S, T, Tt, mc):
    return (1 + T + Tt if mc else 3) * S * S


def base_mlp(S, T, Tt, mc, weights, hidden=BASE["hidden"]):
    return pref.random_mlp(np.random.default_rng(7), features(S, T, Tt, mc), hidden, weights)


@functools.lru_cache(maxsize=None)
def reach_levels(orc, S, mc):
    """(blk, init, tgt, ref): reach_cases.levels and their Reference at reach_cases.CAPACITY rooted on the initial cells."""
    import reach_cases as cases
    blk, init, tgt = cases.levels(orc, S, mc, BASE["levels"])
    return blk, init, tgt, rt.build(orc, S, mc, blk, tgt, init, rt.MAX_DEPTH, cases.CAPACITY)


@functools.lru_cache(maxsize=None)
def dense_levels(orc, S, T, K, mc):
    """(blk, init, tgt, table): generate_mt19937 levels 1000 .. 1127, the odd ones' targets where six moves leave the tiles."""
    import reach_cases as cases
    blk, init, tgt = orc.generate_mt19937(S, T, T, K, np.arange(1000, 1000 + BASE["levels"], dtype=np.uint32))
    tgt = tgt.copy()
    tgt[:, 1::2] = cases.walked(orc, S, blk, init, moves=6)[:, 1::2]
    tgt = np.ascontiguousarray(tgt)
    return blk, init, tgt, tref.table(orc, S, mc, blk, tgt, T)


@functools.lru_cache(maxsize=None)
def base_case(orc, kind, shape, mc, mode):
    """(levels, table, mlp, want) of the base case: `shape` is S (REACH) or (S, T, obstacles) (DENSE).  Computed once; nobody
    writes into it."""
    if kind == REACH:
        S = shape
        blk, init, tgt, table = reach_levels(orc, S, mc)
    else:
        S = shape[0]
        blk, init, tgt, table = dense_levels(orc, *shape, mc)
    sel, weights = MODES[mode]
    mlp = base_mlp(S, init.shape[0], tgt.shape[0], mc, weights)
    want = rollout(orc, kind, table, S, mc, BASE["max_steps"], blk, init, tgt, mlp, BASE["steps"], sel, mode, threshold=rref.threshold_of(BASE["epsilon"]),
                   beta=rref.threshold_of(BASE["beta"]), seed=BASE["seed"])
    return (blk, init, tgt), table, mlp, want


def summary(want):
    return dict(expert=int(want["who"][WHO_EXPERT]), expert_differs=want["expert_differs"], random=int(want["who"][WHO_RANDOM]),
                network=int(want["who"][WHO_NETWORK]), teach_no_move=want["teach_no_move"], wins=want["n_wins"], timeouts=want["timeouts"],
                resets=want["resets"], kinds=dict(zip(rx.KINDS, want["kinds"].tolist())))


def check_base(kind, S, mode, want):
    """The floors against a vacuous pass, from 3x3 up; returns summary(want)."""
    s = summary(want)
    if S >= 3:
        f = FLOORS
        assert s["expert"] >= f["expert"] and s["expert_differs"] >= f["expert_differs"] and s["random"] >= f["random"], (kind, S, mode, s)
        assert s["network"] >= f["network"] and s["teach_no_move"] >= f["teach_no_move"], (kind, S, mode, s)
        assert s["wins"] >= f["wins"] and s["timeouts"] >= f["timeouts"], (kind, S, mode, s)
        if mode == 1:
            assert s["resets"] >= f["resets"], (kind, S, mode, s)
        if kind == REACH:
            assert min(s["kinds"].values()) >= f["kinds"], (kind, S, mode, s)
    return s


# kernel name -> (S, select, kind): the occupancy cases, one per kernel of the library
OCC_WAVES, OCC_STEPS = 4096, 4
OCC_BOARDS = OCC_WAVES * 64 - 3
OCCUPANCY_CASES = {f"k_mixed_rollout<{S}, {sel}, {kind}>": (S, sel, kind) for S in range(1, 9) for sel in (pref.GREEDY, pref.SAMPLE) for kind in (DENSE, REACH)}
