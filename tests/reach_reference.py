"""CPU yardstick of the hashed solver (test infrastructure): the breadth-first search of tests/solver_reference.py over the
oracle, restated for boards whose index space is beyond a dense table.

Three things differ from solver_reference: states are deduplicated by sorted int64 keys (board << 48 | ordered index) and not in
a dense boolean table of N x index space; `capacity` and `states` follow include/tiler_slider_reach.h; and `best` comes from that
header's definition - the four successor boards are solved and their optimum compared with the board's own.  It shares no code
and no method with the kernel: no hash set, no first-move bits carried along.

    search(...)   (moves int16 [N], states int32 [N])
    solve(...)    (moves int16 [N], best uint8 [N], states int32 [N])

The definition, restated on its own.  F(0) is the board as it stands, F(d) the non-won states first reached after d moves,
V(d) = |F(0) u .. u F(d)|.  A won board: moves 0, states 0.  Else for d = 1, 2, ...: all of F(d - 1) is expanded, then in this
order: a successor was won -> d; V(d) > capacity -> SOLVE_FULL; F(d) empty -> SOLVE_NONE; d == max_depth -> SOLVE_DEPTH.
max_depth = 0: SOLVE_DEPTH.  states = the number of states expanded = V(D - 1), D the depth at which the search stopped."""
import numpy as np

from level_solver import oracle_expand

SOLVE_NONE, SOLVE_DEPTH, SOLVE_FULL = -1, -2, -3
UNBOUNDED = 1 << 62


def search(orc, S, mc, blk, tgt, pos, max_depth=64, capacity=4096):
    """blk [W, N], tgt [Tt, N], pos [T, N]: the boards as they stand (device layout, numpy; cell ids inside the board)."""
    expand = oracle_expand(orc)
    blk, tgt, pos = np.ascontiguousarray(blk), np.ascontiguousarray(tgt), np.ascontiguousarray(pos)
    T, N = pos.shape
    assert N < (1 << 15) and (S * S) ** T <= (1 << 48)
    weights = np.array([(S * S) ** t for t in range(T)], np.int64).reshape(T, 1)
    key_of = lambda board, p: (board.astype(np.int64) << 48) | (p.astype(np.int64) * weights).sum(axis=0)
    won0 = orc.OracleBatch(S, mc, 2**30, blk, pos, tgt).won() != 0
    moves = np.where(won0, 0, SOLVE_NONE).astype(np.int16)
    states = np.zeros(N, np.int32)
    fb = np.flatnonzero(~won0)              # board of every frontier state
    fp = np.ascontiguousarray(pos[:, fb])   # its cells
    visited = np.sort(key_of(fb, fp))       # every state reached so far, of every board
    count = (~won0).astype(np.int64)        # V(d) of every board
    depth = 0
    while fb.size:
        if depth == max_depth:
            moves[np.unique(fb)] = SOLVE_DEPTH
            break
        depth += 1
        states[np.unique(fb)] = count[np.unique(fb)]      # all of V(depth - 1) is expanded once this depth has run
        lv = np.repeat(fb, 4)
        p4 = np.ascontiguousarray(np.repeat(fp, 4, axis=1))
        act = np.tile(np.arange(4, dtype=np.uint8), fb.size)
        new_pos, won = expand(S, mc, np.ascontiguousarray(blk[:, lv]), p4, np.ascontiguousarray(tgt[:, lv]), p4, act)
        solved = np.unique(lv[won])
        moves[solved] = depth
        keep = ~np.isin(lv, solved)
        lv, new_pos = lv[keep], new_pos[:, keep]
        keys = key_of(lv, new_pos)
        at = np.searchsorted(visited, keys)
        fresh = visited[np.minimum(at, visited.size - 1)] != keys   # (visited holds the root of every board that is searched)
        keys, first = np.unique(keys[fresh], return_index=True)   # one copy of a state reached twice in this depth
        fb, fp = lv[fresh][first], np.ascontiguousarray(new_pos[:, fresh][:, first])
        count += np.bincount(fb, minlength=N)
        live = np.setdiff1d(np.unique(lv), solved)                 # boards that expanded a frontier and found no win
        full = live[count[live] > capacity]
        moves[full] = SOLVE_FULL
        # a live board without a fresh state keeps SOLVE_NONE; a full board's states leave the search
        go = ~np.isin(fb, full)
        fb, fp, keys = fb[go], np.ascontiguousarray(fp[:, go]), keys[go]
        visited = np.sort(np.concatenate([visited, keys]))
    return moves, states


def solve(orc, S, mc, blk, tgt, pos, max_depth=64, capacity=4096):
    """(moves, best, states).  best by the definition: bit a set <=> moves >= 1 and the board after Move a is moves - 1 moves
    from won.  Only boards with moves >= 1 can have a bit, and a successor that is moves - 1 from won is found by a search of
    depth moves - 1, so the four successors of those boards are searched that deep, without a budget of states."""
    blk, tgt, pos = np.ascontiguousarray(blk), np.ascontiguousarray(tgt), np.ascontiguousarray(pos)
    moves, states = search(orc, S, mc, blk, tgt, pos, max_depth, capacity)
    best = np.zeros(pos.shape[1], np.uint8)
    for m in np.unique(moves[moves >= 1]):
        who = np.flatnonzero(moves == m)
        lv = np.repeat(who, 4)
        p4 = np.ascontiguousarray(pos[:, lv])
        act = np.tile(np.arange(4, dtype=np.uint8), who.size)
        b4, t4 = np.ascontiguousarray(blk[:, lv]), np.ascontiguousarray(tgt[:, lv])
        after, _ = oracle_expand(orc)(S, mc, b4, p4, t4, p4, act)
        m4, _ = search(orc, S, mc, b4, t4, after, int(m) - 1, UNBOUNDED)
        hit = (m4.reshape(who.size, 4) == int(m) - 1)
        best[who] = (hit * (1 << np.arange(4))).sum(axis=1).astype(np.uint8)
    return moves, best, states


def reachable(orc, S, mc, blk, tgt, pos):
    """int64 [N]: the size of the whole reachable set of boards that cannot be won, i.e. `states` of an unbounded search."""
    moves, states = search(orc, S, mc, blk, tgt, pos, 32767, UNBOUNDED)
    assert (moves == SOLVE_NONE).all()
    return states.astype(np.int64)
