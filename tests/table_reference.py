"""CPU yardstick of the distance-to-win tables (test infrastructure): backward relaxation over the oracle's successor table.

It shares no method with the kernel (tiler_slider_amd/csrc/ts_table.hip: rounds over bitmaps in LDS).  Per board the VALID
placements are enumerated - all tiles on distinct cells, none on an obstacle -, one batched `OracleBatch.step` per move gives
every placement's four successors and one `won()` the placements at distance 0, and then
    dist[s] = min(dist[s], 1 + min_a dist[succ_a(s)])
is relaxed in NumPy until nothing changes.  The oracle is handed valid placements ONLY: with a tile on an obstacle or two tiles
on one cell it returns cells outside the board.  That no valid placement has an invalid successor is asserted here.

    exact(...)     int32 [N, states]: the distance of every placement, INVALID_PLACEMENT (-1) or UNREACHABLE
    cut(...)       uint8 [N, states]: the table of include/tiler_slider_table.h for a max_depth, from exact()'s answer
    table(...)     cut(exact(...))
    lookup(...)    (moves int16, best uint8, action uint8) [N]: what ts_table_lookup reports for boards on ANY uint8 rows

The stopping rule, restated on its own: with R(d) the valid placements at distance exactly d, a board stops at the first d
with R(d) empty, and everything unresolved becomes NONE; otherwise it stops at d = max_depth with R(d) not empty, and
everything unresolved becomes DEEP."""
import numpy as np

MAX_DEPTH, INVALID, DEEP, NONE = 252, 253, 254, 255
INVALID_PLACEMENT, UNREACHABLE = -1, 1 << 30


def index_weights(S, T):
    return np.array([(S * S) ** t for t in range(T)], np.int64).reshape(T, 1)


def index_of(S, pos):
    """idx = sum_t cell_t * (S * S) ** t of pos [T, N]."""
    return (pos.astype(np.int64) * index_weights(S, pos.shape[0])).sum(axis=0)


def exact(orc, S, mc, blk, tgt, T):
    """blk [W, N], tgt [Tt, N] (device layout, numpy), T tiles -> int32 [N, (S * S) ** T]."""
    blk, tgt = np.ascontiguousarray(blk, np.uint32), np.ascontiguousarray(tgt)
    N, C = blk.shape[1], S * S
    states = C ** T
    idx = np.arange(states, dtype=np.int64)
    cells = np.stack([(idx // C ** t) % C for t in range(T)]) if T else np.zeros((0, states), np.int64)
    distinct = np.ones(states, bool)
    for i in range(T):
        for j in range(i):
            distinct &= cells[i] != cells[j]
    c = np.arange(C)
    blocked = ((blk[c // 32, :] >> (c % 32).astype(np.uint32)[:, None]) & 1).T != 0     # [N, C]
    valid = np.broadcast_to(distinct, (N, states)).copy()
    for t in range(T):
        valid &= ~blocked[:, cells[t]]
    nb, ns = np.nonzero(valid)
    M = len(nb)
    pos = np.ascontiguousarray(cells[:, ns].astype(orc.cell_dtype(S)))
    b, t = np.ascontiguousarray(blk[:, nb]), np.ascontiguousarray(tgt[:, nb])
    won = orc.OracleBatch(S, mc, 2**30, b, pos, t).won() != 0
    succ = np.empty((4, M), np.int64)
    for a in range(4):
        batch = orc.OracleBatch(S, mc, 2**30, b, pos, t)
        batch.step(np.full(M, a, np.uint8), obs=False)
        assert (batch.pos < C).all()
        succ[a] = index_of(S, batch.pos)
        assert valid[nb, succ[a]].all(), "a valid placement has an invalid successor"
    dist = np.full(N * states, UNREACHABLE, np.int32)
    dist[np.flatnonzero(~valid.ravel())] = INVALID_PLACEMENT
    own = nb * states + ns
    dist[own[won]] = 0
    own, succ = own[~won], nb[~won] * states + succ[:, ~won]
    while True:
        new = np.minimum(dist[own], dist[succ].min(axis=0) + 1)
        if np.array_equal(new, dist[own]):
            break
        dist[own] = new
    return dist.reshape(N, states)


def cut(dist, max_depth=MAX_DEPTH):
    """The table for a max_depth 0 .. 252 from exact()'s distances."""
    assert 0 <= max_depth <= MAX_DEPTH
    N = dist.shape[0]
    finite = (dist >= 0) & (dist < UNREACHABLE)
    present = np.zeros((N, MAX_DEPTH + 2), bool)                       # present[n, d]: R(d) of board n is not empty
    nb, ns = np.nonzero(finite)
    present[nb, np.minimum(dist[nb, ns], MAX_DEPTH + 1)] = True
    present[:, MAX_DEPTH + 1] = False
    first_empty = present.argmin(axis=1)                               # the first d with R(d) empty
    exhausted = first_empty <= max_depth                               # stops there: unresolved -> NONE
    assert not (finite & (dist >= first_empty[:, None]))[exhausted].any()   # nothing finite lies beyond an empty R(d)
    out = np.where(finite & (dist <= max_depth), dist, np.where(exhausted[:, None], NONE, DEEP)).astype(np.uint8)
    out[dist == INVALID_PLACEMENT] = INVALID
    return out


def table(orc, S, mc, blk, tgt, T, max_depth=MAX_DEPTH):
    return cut(exact(orc, S, mc, blk, tgt, T), max_depth)


def to_moves(entries):
    """What ts_table_lookup reports for table entries: int16 with NONE and INVALID -> -1 (SOLVE_NONE), DEEP -> -2 (SOLVE_DEPTH)."""
    e = np.asarray(entries).astype(np.int16)
    return np.where(e <= MAX_DEPTH, e, np.where(e == DEEP, -2, -1)).astype(np.int16)


_LOWEST_BIT = np.array([255] + [(b & -b).bit_length() - 1 for b in range(1, 16)], np.uint8)


def is_placement(S, blk, pos):
    """bool [N]: the cells of pos [T, N], clipped to S * S - 1, are distinct and none of them is an obstacle of blk [W, N]."""
    blk = np.ascontiguousarray(blk, np.uint32)
    T, N = pos.shape
    p = np.minimum(np.asarray(pos).astype(np.int64), S * S - 1)
    ok = np.ones(N, bool)
    for i in range(T):
        ok &= ((blk[p[i] >> 5, np.arange(N)] >> (p[i] & 31).astype(np.uint32)) & 1) == 0
        for j in range(i):
            ok &= p[i] != p[j]
    return ok


def lookup(orc, S, blk, pos, rows_of_table, rows=None):
    """The rule of ts_table_lookup (include/tiler_slider_table.h) restated on NumPy, over whatever bytes it is given - a table that
    was built or one that nobody built.  blk [W, N], pos [T, N] (any cell ids: clipped to S * S - 1), rows_of_table uint8
    [n_rows, states]; board n reads row rows[n] (default: row n).  The board's own entry e gives moves = to_moves(e); for e in
    1 .. 252 bit a of best is set where the entry of the placement after Move a - one OracleBatch.step per move - is e - 1;
    action is the lowest set bit of best, 255 for none.  A board whose clipped cells are not a placement (a tile on an obstacle,
    two tiles on one cell) or whose row lies outside the table gets -1, 0, 255 and is never handed to the oracle."""
    blk = np.ascontiguousarray(blk, np.uint32)
    tab = np.asarray(rows_of_table)
    assert tab.dtype == np.uint8 and tab.ndim == 2
    T, N = pos.shape
    C = S * S
    assert blk.shape[1] == N and tab.shape[1] == C ** T
    r = np.arange(N, dtype=np.int64) if rows is None else np.asarray(rows).astype(np.int64)
    assert r.shape == (N,)
    p = np.minimum(np.asarray(pos).astype(np.int64), C - 1)
    ok = (r >= 0) & (r < tab.shape[0]) & is_placement(S, blk, pos)
    moves, best = np.full(N, -1, np.int16), np.zeros(N, np.uint8)
    v = np.flatnonzero(ok)
    if v.size:
        cells = np.ascontiguousarray(p[:, v].astype(orc.cell_dtype(S)))
        b, none = np.ascontiguousarray(blk[:, v]), np.zeros((0, v.size), orc.cell_dtype(S))   # a slide does not look at the targets
        e = tab[r[v], index_of(S, cells)].astype(np.int64)
        moves[v] = to_moves(e)
        asks = (e >= 1) & (e <= MAX_DEPTH)
        bits = np.zeros(v.size, np.uint8)
        for a in range(4):
            batch = orc.OracleBatch(S, False, 2**30, b, cells, none)
            batch.step(np.full(v.size, a, np.uint8), obs=False)
            assert (batch.pos < C).all()
            after = tab[r[v], index_of(S, batch.pos)].astype(np.int64)
            bits |= ((asks & (after == e - 1)).astype(np.uint8) << a).astype(np.uint8)
        best[v] = bits
    return moves, best, _LOWEST_BIT[best]
