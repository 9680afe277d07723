"""CPU yardstick of the reachable distance tables (test infrastructure): the closure of every level's root over the oracle with
sorted int64 keys - the search of tests/reach_reference.py that never stops at a win -, then the distances by rounds over
successor indices found with searchsorted.  It shares no hash set and no code with the kernel (tiler_slider_amd/csrc/ts_rtable.hip).

The definition (include/tiler_slider_rtable.h), restated on its own.  R is the least set that holds the root if it is not won and,
with every state, each of its four successors that is not won.  A level with |R| > capacity is FULL.  D = 1 + the least D over the
four successors, 0 on a won placement, by rounds d = 1, 2, ...: round d resolves the unresolved states with a successor at d - 1.
With R(d) the states at distance exactly d >= 1: a level stops at the first d <= max_depth with R(d) empty and everything
unresolved is NONE (255); otherwise it stops behind round max_depth and everything unresolved is DEEP (254).

    build(...)    a Reference: per level the sorted keys of R, their entries and successors, count, root_moves, deepest
    lookup(...)   (moves int16, best uint8, action uint8) [N]: what ts_rtable_lookup reports for boards wherever they stand"""
import numpy as np

from level_solver import oracle_expand

MAX_DEPTH, DEEP, NONE = 252, 254, 255
SOLVE_NONE, SOLVE_DEPTH, SOLVE_FULL, SOLVE_ABSENT = -1, -2, -3, -4
WON = -1   # a successor index: the board after that move is won

_LOWEST_BIT = np.array([255] + [(b & -b).bit_length() - 1 for b in range(1, 16)], np.uint8)


def to_moves(entries):
    """Entries as ts_table_lookup maps them: 1 .. 252 as they are, NONE -> -1, DEEP -> -2."""
    e = np.asarray(entries).astype(np.int16)
    return np.where((e >= 1) & (e <= MAX_DEPTH), e, np.where(e == DEEP, SOLVE_DEPTH, SOLVE_NONE)).astype(np.int16)


def keys_of(S, pos):
    """idx = sum_t cell_t * (S * S) ** t of pos [T, N] (cell ids inside the board)."""
    w = np.array([(S * S) ** t for t in range(pos.shape[0])], np.int64).reshape(-1, 1)
    return (pos.astype(np.int64) * w).sum(axis=0)


def cells_of(S, T, idx, dtype):
    C = S * S
    return np.ascontiguousarray(np.stack([(idx // C ** t) % C for t in range(T)]).astype(dtype)) if T else np.zeros((0, idx.size), dtype)


class Reference:
    """level, idx: every stored state, sorted by (level, idx); start [N + 1]: level n's states are start[n] .. start[n + 1];
    succ [4, M]: the position in these arrays of the state after each move, WON for a won successor; entry uint8 [M];
    count int32 [N] (|R| or SOLVE_FULL), root_moves int16 [N], deepest int32 [N], size int64 [N]: |R| as far as it was counted."""

    def keys(self, n):
        return self.idx[self.start[n]:self.start[n + 1]]

    def entries(self, n):
        return self.entry[self.start[n]:self.start[n + 1]]

    def cells(self, n):
        """[T, count] the placements of level n's states, in the order of keys(n)."""
        return cells_of(self.S, self.T, self.keys(n), self.cell_dtype)


def _closure(orc, S, mc, blk, tgt, root, capacity):
    """(sorted global keys level << 48 | idx of every state of every level that fits, size int64 [N]).  A level leaves the search
    once it holds more than `capacity` states."""
    expand = oracle_expand(orc)
    T, N = root.shape
    assert N < (1 << 15) and (S * S) ** T <= (1 << 48)
    won0 = orc.OracleBatch(S, mc, 2**30, blk, root, tgt).won() != 0
    fb = np.flatnonzero(~won0)
    fp = np.ascontiguousarray(root[:, fb])
    glob = lambda lv, p: (lv.astype(np.int64) << 48) | keys_of(S, p)
    visited = np.sort(glob(fb, fp))
    size = (~won0).astype(np.int64)
    full = size > capacity
    while fb.size:
        lv = np.repeat(fb, 4)
        p4 = np.ascontiguousarray(np.repeat(fp, 4, axis=1))
        act = np.tile(np.arange(4, dtype=np.uint8), fb.size)
        new_pos, won = expand(S, mc, np.ascontiguousarray(blk[:, lv]), p4, np.ascontiguousarray(tgt[:, lv]), p4, act)
        lv, new_pos = lv[~won], new_pos[:, ~won]
        keys = glob(lv, new_pos)
        at = np.searchsorted(visited, keys)
        fresh = visited[np.minimum(at, visited.size - 1)] != keys
        keys, first = np.unique(keys[fresh], return_index=True)
        fb, fp = lv[fresh][first], np.ascontiguousarray(new_pos[:, fresh][:, first])
        size += np.bincount(fb, minlength=N)
        full = size > capacity
        go = ~full[fb]
        fb, fp, keys = fb[go], np.ascontiguousarray(fp[:, go]), keys[go]
        visited = np.sort(np.concatenate([visited, keys]))
    return visited[~full[visited >> 48]], size, full


def build(orc, S, mc, blk, tgt, root, max_depth=MAX_DEPTH, capacity=1 << 40):
    """blk [W, N], tgt [Tt, N], root [T, N] (device layout, numpy; cell ids beyond the board are clamped here)."""
    assert 0 <= max_depth <= MAX_DEPTH
    C = S * S
    blk = np.ascontiguousarray(blk)
    tgt, root = np.ascontiguousarray(np.minimum(tgt, C - 1)), np.ascontiguousarray(np.minimum(root, C - 1))
    T, N = root.shape
    ref = Reference()
    ref.S, ref.T, ref.mc, ref.cell_dtype = S, T, mc, root.dtype
    glob, ref.size, full = _closure(orc, S, mc, blk, tgt, root, capacity)
    ref.level, ref.idx = (glob >> 48).astype(np.int64), glob & ((1 << 48) - 1)
    ref.start = np.searchsorted(ref.level, np.arange(N + 1))
    M = glob.size
    # the four successors of every state, one batched step per move, as positions in the sorted arrays
    pos = cells_of(S, T, ref.idx, root.dtype)
    b, t = np.ascontiguousarray(blk[:, ref.level]), np.ascontiguousarray(tgt[:, ref.level])
    expand = oracle_expand(orc)
    ref.succ = np.empty((4, M), np.int64)
    for a in range(4):
        after, won = expand(S, mc, b, pos, t, pos, np.full(M, a, np.uint8)) if M else (pos, np.zeros(0, bool))
        at = np.searchsorted(glob, (ref.level << 48) | keys_of(S, after))
        assert M == 0 or (glob[np.minimum(at, M - 1)][~won] == ((ref.level << 48) | keys_of(S, after))[~won]).all(), "R is not closed"
        ref.succ[a] = np.where(won, WON, at)
    # the rounds
    dist = np.full(M, NONE, np.int64)
    won_succ = (ref.succ == WON).any(axis=0)
    safe = np.maximum(ref.succ, 0)
    present = np.zeros((N, max_depth + 2), bool)   # present[n, d]: R(d) of level n is not empty
    for d in range(1, max_depth + 1):
        hit = won_succ if d == 1 else ((dist[safe] == d - 1) & (ref.succ != WON)).any(axis=0)
        hit = hit & (dist == NONE)
        if not hit.any():
            break
        dist[hit] = d
        present[ref.level[hit], d] = True
    present[:, 0] = True
    exhausted = ~present[:, :max_depth + 1].all(axis=1)            # some R(d), 1 <= d <= max_depth, is empty: unresolved -> NONE
    ref.entry = np.where(dist != NONE, dist, np.where(exhausted[ref.level], NONE, DEEP)).astype(np.uint8)
    ref.count = np.where(full, SOLVE_FULL, ref.size).astype(np.int32)
    ref.deepest = np.zeros(N, np.int32)
    finite = dist != NONE
    np.maximum.at(ref.deepest, ref.level[finite], dist[finite].astype(np.int32))
    # the root: won -> 0, FULL, else its entry
    won0 = orc.OracleBatch(S, mc, 2**30, blk, root, tgt).won() != 0
    ref.root_moves = np.where(won0, 0, SOLVE_FULL).astype(np.int16)
    live = np.flatnonzero(~won0 & ~full)
    at = np.searchsorted(glob, (live.astype(np.int64) << 48) | keys_of(S, root[:, live]))
    ref.root_moves[live] = to_moves(ref.entry[at])
    return ref


def lookup(orc, ref, blk, tgt, pos, rows=None):
    """The rule of ts_rtable_lookup restated: boards blk [W, N], tgt [Tt, N], pos [T, N] read level rows[n] (default n) of `ref`.
    A row outside the table -> -1, 0, 255; a won board -> 0, 0, 255; a FULL level -> SOLVE_FULL; a placement the level does not
    hold -> SOLVE_ABSENT; else the entry, and bit a of best where the successor by Move a is won and the entry is 1, or holds the
    entry less one."""
    S, C = ref.S, ref.S * ref.S
    blk = np.ascontiguousarray(blk)
    tgt, pos = np.ascontiguousarray(np.minimum(tgt, C - 1)), np.ascontiguousarray(np.minimum(pos, C - 1))
    N, L = pos.shape[1], len(ref.count)
    r = np.arange(N, dtype=np.int64) if rows is None else np.asarray(rows).astype(np.int64)
    inside = (r >= 0) & (r < L)
    rr = np.where(inside, r, 0)
    won = orc.OracleBatch(S, ref.mc, 2**30, blk, pos, tgt).won() != 0
    moves, best = np.full(N, SOLVE_NONE, np.int16), np.zeros(N, np.uint8)
    moves[inside & won] = 0
    full = inside & ~won & (ref.count[rr] == SOLVE_FULL)
    moves[full] = SOLVE_FULL
    ask = inside & ~won & ~full
    glob = (ref.level << 48) | ref.idx
    want = (rr << 48) | keys_of(S, pos)
    at = np.minimum(np.searchsorted(glob, want), max(glob.size - 1, 0))
    held = ask & (glob[at] == want if glob.size else np.zeros(N, bool))
    moves[ask & ~held] = SOLVE_ABSENT
    h = np.flatnonzero(held)
    e = ref.entry[at[h]].astype(np.int64)
    moves[h] = to_moves(e)
    s = ref.succ[:, at[h]]
    after = np.where(s == WON, 0, ref.entry[np.maximum(s, 0)].astype(np.int64))
    bits = (((e >= 1) & (e <= MAX_DEPTH))[None, :] & (after == e[None, :] - 1)) * (1 << np.arange(4))[:, None]
    best[h] = bits.sum(axis=0).astype(np.uint8)
    return moves, best, _LOWEST_BIT[best]
