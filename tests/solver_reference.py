"""CPU yardstick of the on-device solver (test infrastructure): breadth-first search over the oracle.

The reference has no solver.  The oracle is pinned to the reference by the goldens; this search pins ts_solve to the oracle:
every expansion is one batched `OracleBatch.step` (level_solver.oracle_expand), every win test the oracle's.  It shares no
code and no method with the kernel: states are deduplicated in a dense boolean table per board, and the `best` mask is not
carried along the search but computed as include/tiler_slider_search.h DEFINES it - by solving the four successor boards and
comparing their optimum with the board's own.

    optimum(...)          int16 [N]: 0 for a won board, the least number of moves, SOLVE_NONE or SOLVE_DEPTH
    solve(...)            (moves int16 [N], best uint8 [N]): bit a of best set <=> moves >= 1 and the board after Move a is
                          moves - 1 moves from won

With F(d) the states first reached after d moves: a board ends at the first d whose F(d) is empty (SOLVE_NONE), else at
d = max_depth with F(d) not empty (SOLVE_DEPTH) - the header's definition, restated here on its own."""
import numpy as np

from level_solver import oracle_expand

SOLVE_NONE, SOLVE_DEPTH = -1, -2


def optimum(orc, S, mc, blk, tgt, pos, max_depth=64):
    """blk [W, N], tgt [Tt, N], pos [T, N]: the boards as they stand (device layout, numpy)."""
    expand = oracle_expand(orc)
    blk, tgt, pos = np.ascontiguousarray(blk), np.ascontiguousarray(tgt), np.ascontiguousarray(pos)
    T, N = pos.shape
    C = S * S
    space = C ** T
    weights = np.array([C ** t for t in range(T)], np.int64).reshape(T, 1)
    index = lambda p: (p.astype(np.int64) * weights).sum(axis=0)
    standing = orc.OracleBatch(S, mc, 2**30, blk, pos, tgt)
    won0 = standing.won() != 0
    moves = np.full(N, SOLVE_NONE, np.int16)
    moves[won0] = 0
    seen = np.zeros((N, space), bool)
    fb = np.flatnonzero(~won0)          # board of every frontier state
    fp = pos[:, fb]                     # its cells
    seen[fb, index(fp)] = True
    depth = 0
    while fb.size:
        if depth == max_depth:
            moves[np.unique(fb)] = SOLVE_DEPTH
            break
        depth += 1
        lv = np.repeat(fb, 4)
        p4 = np.ascontiguousarray(np.repeat(fp, 4, axis=1))
        act = np.tile(np.arange(4, dtype=np.uint8), fb.size)
        new_pos, won = expand(S, mc, np.ascontiguousarray(blk[:, lv]), p4, np.ascontiguousarray(tgt[:, lv]), p4, act)
        solved = np.unique(lv[won])
        moves[solved] = depth
        keep = ~np.isin(lv, solved)
        lv, new_pos = lv[keep], new_pos[:, keep]
        idx = index(new_pos)
        fresh = ~seen[lv, idx]
        lv, new_pos, idx = lv[fresh], new_pos[:, fresh], idx[fresh]
        _, first = np.unique(lv * space + idx, return_index=True)   # one copy of a state reached twice in this depth
        fb, fp = lv[first], np.ascontiguousarray(new_pos[:, first])
        seen[fb, idx[first]] = True
    return moves


def solve(orc, S, mc, blk, tgt, pos, max_depth=64):
    blk, tgt, pos = np.ascontiguousarray(blk), np.ascontiguousarray(tgt), np.ascontiguousarray(pos)
    N = pos.shape[1]
    moves = optimum(orc, S, mc, blk, tgt, pos, max_depth)
    lv = np.repeat(np.arange(N), 4)
    p4 = np.ascontiguousarray(np.repeat(pos, 4, axis=1))
    act = np.tile(np.arange(4, dtype=np.uint8), N)
    b4, t4 = np.ascontiguousarray(blk[:, lv]), np.ascontiguousarray(tgt[:, lv])
    after, _ = oracle_expand(orc)(S, mc, b4, p4, t4, p4, act)
    m4 = optimum(orc, S, mc, b4, t4, after, max_depth).reshape(N, 4).astype(np.int32)
    hit = (moves >= 1)[:, None] & (m4 == moves.astype(np.int32)[:, None] - 1)
    best = (hit * (1 << np.arange(4))).sum(axis=1).astype(np.uint8)
    return moves, best


def fixture_groups(golden_dir, pack_levels):
    """The 400 screenshot levels grouped by shape: {(S, T, mc): (indices into the fixture, blk, init, tgt, min_moves)}."""
    import os
    with np.load(os.path.join(golden_dir, "levels_from_screenshots.npz")) as z:
        g = {k: z[k] for k in z.files}
    keys = {}
    for i in range(len(g["names"])):
        keys.setdefault((int(g["size"][i]), int(g["n_tiles"][i]), bool(g["multi"][i])), []).append(i)
    out = {}
    for (S, T, mc), ids in sorted(keys.items()):
        cells = lambda a, i, k: [tuple(int(v) for v in rc) for rc in a[i, :k]]
        blk, init, tgt = pack_levels(S, [cells(g["blocked"], i, int(g["n_blocked"][i])) for i in ids], [cells(g["tiles"], i, T) for i in ids],
                                     [cells(g["targets"], i, T) for i in ids])
        out[(S, T, mc)] = (np.array(ids), blk, init, tgt, g["min_moves"][ids].astype(np.int16))
    return out
