"""CPU yardstick of the reach-table experts (test infrastructure, no test of its own): the loop of include/tiler_slider_rexpert.h
restated on NumPy and the CPU oracle - rollout_reference.rollout's loop with `rtable_reference.lookup` for the expert move, the
same draws, `OracleBatch.step(..., reward=True)` for the step - and the labels as `rtable_reference.lookup` on
targets_reference.cells_of(first, pos_log, k).  It shares no code with tiler_slider_amd/csrc/ts_rexpert.hip: the table is a
Reference of sorted keys, not a hash table.  Imports neither torch nor the libraries at import time."""
import numpy as np

import rtable_reference as rt
from rollout_reference import FLAG_AUTORESET, FLAG_SUCCESS, FLAG_TIMEOUT, draws, threshold_of  # noqa: F401 (threshold_of: for the tests)

KINDS = ("finite", "won", "none_deep", "full", "absent")   # lookups by kind: moves 1 .. 252, 0, NONE / DEPTH, FULL, ABSENT
OUTPUTS = ("wins", "finished", "first_win", "win_moves", "reward_sum", "flags", "act_log", "flags_log", "pos_log")


def kinds_of(moves):
    """int64 [5]: how many of `moves` are of each of KINDS."""
    m = np.asarray(moves)
    return np.array([(m >= 1).sum(), (m == 0).sum(), ((m == rt.SOLVE_NONE) | (m == rt.SOLVE_DEPTH)).sum(), (m == rt.SOLVE_FULL).sum(),
                     (m == rt.SOLVE_ABSENT).sum()], np.int64)


def rollout(orc, ref, S, mc, max_steps, blk, init, tgt, steps, mode=0, *, pos=None, step_count=None, done=None, rows=None, threshold=0,
            seed=0, step_index=0, board_offset=0):
    """The loop, from the state (pos, step_count, done) - default: freshly reset - on the Reference `ref` of the boards' levels
    (level rows[n], default n).  Returns a dict of the nine outputs of ts_rollout_out, the state after the loop (pos, step_count,
    done) and what the run exercised: `source` int64 [3] board-steps whose action came from the expert / the exploration draw /
    the no-expert fallback, `kinds` int64 [5] lookups by kind (KINDS), `resets` the AUTORESET steps, `timeouts` the TIMEOUT
    steps, and per-board bools `won`, `timed_out`."""
    b = orc.OracleBatch(S, mc, max_steps, blk, init, tgt)
    n, T = b.n, b.n_tiles
    if pos is not None:
        b.pos[...] = pos
    if step_count is not None:
        b.step_count[...] = step_count
    if done is not None:
        b.done[...] = done
    out = {k: np.zeros(n, np.int32) for k in ("wins", "finished", "first_win", "win_moves", "reward_sum")}
    out["flags"] = np.zeros(n, np.uint8)
    out["act_log"], out["flags_log"] = np.zeros((steps, n), np.uint8), np.zeros((steps, n), np.uint8)
    out["pos_log"] = np.zeros((steps, T, n), b.pos.dtype)
    source, kinds = np.zeros(3, np.int64), np.zeros(5, np.int64)
    for k in range(steps):
        r = draws(n, seed, step_index + k, board_offset)
        rnd = (r >> np.uint64(62)).astype(np.uint8)
        assert np.array_equal(rnd, orc.fill_actions(n, seed=seed, step_index=step_index + k, board_offset=board_offset))
        moves, _, e = rt.lookup(orc, ref, b.blk, b.tgt, b.pos, rows)
        kinds += kinds_of(moves)
        explore = (r & np.uint64(0xffffffff)) < np.uint64(threshold)
        a = np.where(explore | (e == 255), rnd, e).astype(np.uint8)
        source += (int((~explore & (e != 255)).sum()), int(explore.sum()), int((~explore & (e == 255)).sum()))
        res = b.step(a, mode=mode, obs=False, reward=True)
        f = res["flags"]
        success = (f & FLAG_SUCCESS) != 0
        out["wins"] += success
        out["finished"] += (f & (FLAG_SUCCESS | FLAG_TIMEOUT)) != 0
        out["first_win"] = np.where(success & (out["first_win"] == 0), k + 1, out["first_win"]).astype(np.int32)
        out["win_moves"] += np.where(success, b.step_count, 0).astype(np.int32)
        out["reward_sum"] += res["reward"]
        out["flags"] = f.copy()
        out["act_log"][k], out["flags_log"][k], out["pos_log"][k] = a, f, b.pos
    out["pos"], out["step_count"], out["done"] = b.pos.copy(), b.step_count.copy(), b.done.copy()
    out["source"], out["kinds"] = source, kinds
    out["won"] = out["wins"] > 0
    out["resets"] = int(((out["flags_log"] & FLAG_AUTORESET) != 0).sum())
    out["timeouts"] = int(((out["flags_log"] & FLAG_TIMEOUT) != 0).sum())
    out["timed_out"] = ((out["flags_log"] & FLAG_TIMEOUT) != 0).any(axis=0) if steps else np.zeros(n, bool)
    return out


def labels(orc, ref, blk, tgt, first, pos_log, steps, rows=None):
    """(moves int16, best uint8, action uint8) [K, N]: rtable_reference.lookup on c[k] = first, pos_log[0], ..., pos_log[K - 2]."""
    from targets_reference import cells_of
    got = [rt.lookup(orc, ref, blk, tgt, cells_of(first, pos_log, k), rows) for k in range(steps)]
    return tuple(np.stack([g[i] for g in got]) for i in range(3))


# ---- the non-degeneracy conditions of the base case (tests/test_gpu_rexpert.py), asserted on the yardstick alone ----
BASE = dict(levels=128, steps=24, max_steps=12, epsilon=0.25, seed=7)
FLOORS = {1: dict(expert=100, kinds=50, wins=20, resets=100, timeouts=50),   # TS_MODE_AUTORESET
          0: dict(expert=20, kinds=20, wins=15, resets=0, timeouts=50)}      # TS_MODE_STRICT


def base_case(orc, S, mc, mode):
    """(ref, blk, init, tgt, want): the base case of size S - reach_cases.levels, a table at reach_cases.CAPACITY rooted on the
    initial cells, K = 24, max_steps = 12, epsilon = 0.25, seed 7 - and the yardstick's rollout from a reset."""
    import reach_cases as cases
    blk, init, tgt = cases.levels(orc, S, mc, BASE["levels"])
    ref = rt.build(orc, S, mc, blk, tgt, init, rt.MAX_DEPTH, cases.CAPACITY)
    want = rollout(orc, ref, S, mc, BASE["max_steps"], blk, init, tgt, BASE["steps"], mode, threshold=threshold_of(BASE["epsilon"]), seed=BASE["seed"])
    return ref, blk, init, tgt, want


def summary(want):
    return dict(expert=int(want["source"][0]), kinds=dict(zip(KINDS, want["kinds"].tolist())), wins=int(want["won"].sum()), resets=want["resets"],
                timeouts=want["timeouts"])


def check_base(S, mode, want):
    """The caps against a vacuous pass, on one colour mode of the base case, from 3x3 up; returns summary(want)."""
    s = summary(want)
    if S >= 3:
        f = FLOORS[1 if mode else 0]
        assert s["expert"] >= f["expert"] and min(s["kinds"].values()) >= f["kinds"] and s["wins"] >= f["wins"], (S, mode, s)
        assert s["resets"] >= f["resets"] and s["timeouts"] >= f["timeouts"], (S, mode, s)
    return s
