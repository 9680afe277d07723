"""CPU yardstick of the fused rollouts (test infrastructure, no test of its own): the loop of include/tiler_slider_rollout.h
restated on NumPy and the CPU oracle - `orc.fill_actions` for the random draw, `table_reference.lookup` for the expert move,
`OracleBatch.step(..., reward=True)` for the step - with mix64 restated on uint64 for the explore bits (its top two bits must
reproduce orc.fill_actions at every step: asserted).  It shares no code with tiler_slider_amd/csrc/ts_rollout.hip.

Also the table of occupancy cases - one per kernel of the rollout library - that tests/test_gpu_rollout.py runs and
tests/test_rollout_cpu.py pins to the code object.  Imports neither torch nor the libraries at import time."""
import numpy as np

GIVEN, RANDOM, TABLE = 0, 1, 2
FLAG_SUCCESS, FLAG_TIMEOUT, FLAG_STEPPED_DONE, FLAG_AUTORESET, FLAG_BAD_ACTION = 0x04, 0x08, 0x10, 0x20, 0x40
K_BOARD_MUL, K_DRAW_MUL = 0xd1b54a32d192ed03, 0x9e3779b97f4a7c15
_M64 = (1 << 64) - 1


def mix64(z):
    """splitmix64's finaliser on a uint64 array (wrapping arithmetic)."""
    z = np.asarray(z, np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xbf58476d1ce4e5b9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94d049bb133111eb)
        z ^= z >> np.uint64(31)
    return z


def draws(n, seed, step_index, board_offset=0):
    """r uint64 [n] of step `step_index`: r >> 62 is ts_fill_actions' action, r & 0xffffffff the explore bits."""
    key = mix64(np.array([(int(seed) ^ ((int(step_index) * K_BOARD_MUL) & _M64)) & _M64], np.uint64))[0]
    with np.errstate(over="ignore"):
        counter = (np.arange(n, dtype=np.uint64) + np.uint64(int(board_offset) & _M64)) * np.uint64(K_DRAW_MUL)
        return mix64(counter + key)


def threshold_of(epsilon):
    return int(round(float(epsilon) * 2 ** 32))


def rollout(orc, S, mc, max_steps, blk, init, tgt, steps, policy, mode=0, *, pos=None, step_count=None, done=None, actions=None,
            table=None, rows=None, threshold=0, seed=0, step_index=0, board_offset=0):
    """The loop, from the state (pos, step_count, done) - default: freshly reset.  Returns a dict of the nine outputs of
    ts_rollout_out, the state after the loop (pos, step_count, done) and what the run exercised: `source` int64 [3] board-steps
    whose action came from the expert / the exploration draw / the no-expert fallback (TABLE), and per-board bools `won`,
    `timed_out`, `reset`."""
    import table_reference as tref
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
    source = np.zeros(3, np.int64)
    for k in range(steps):
        r = draws(n, seed, step_index + k, board_offset)
        rnd = (r >> np.uint64(62)).astype(np.uint8)
        assert np.array_equal(rnd, orc.fill_actions(n, seed=seed, step_index=step_index + k, board_offset=board_offset))
        if policy == GIVEN:
            a = np.ascontiguousarray(actions[k], np.uint8)
        elif policy == RANDOM:
            a = rnd
        else:
            e = tref.lookup(orc, S, b.blk, b.pos, table, rows)[2]
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
    out["source"] = source
    out["won"] = out["wins"] > 0
    out["timed_out"] = ((out["flags_log"] & FLAG_TIMEOUT) != 0).any(axis=0) if steps else np.zeros(n, bool)
    out["reset"] = ((out["flags_log"] & FLAG_AUTORESET) != 0).any(axis=0) if steps else np.zeros(n, bool)
    return out


OUTPUTS = ("wins", "finished", "first_win", "win_moves", "reward_sum", "flags", "act_log", "flags_log", "pos_log")

# kernel name -> (S, T, obstacles): one case per kernel of the rollout library, the shapes of the table library's occupancy
# cases (tests/table_harness.py); tests/test_rollout_cpu.py pins the names to the code object
_OCC_SHAPES = {1: (1, 0), 2: (2, 1), 3: (2, 1), 4: (2, 2), 5: (2, 3), 6: (2, 6), 7: (2, 8), 8: (2, 10)}
OCCUPANCY_CASES = {f"k_rollout<{S}, {P}>": (S, T, K, P) for S, (T, K) in _OCC_SHAPES.items() for P in (GIVEN, RANDOM, TABLE)}
