"""CPU yardstick of the reach policy tables (test infrastructure, no test of its own): the definitions of
include/tiler_slider_rptable.h restated on NumPy over rtable_reference.Reference - per level the keys of R in ascending order, their
entries and their four successors as positions; no hash table, no probe, no list.  It shares no code with
tiler_slider_amd/csrc/ts_rptable.hip.  Everything here is FLAT: one value per state of the Reference, in its order (level, key);
rows_of() makes device-format rows on the host with rstarts_reference.fill_row and says which slot each state took, so whole
buffers can be compared.  Imports neither torch nor the libraries.

    actions(...)        (act uint8 [M], logits float32 [M, 4]) of an integer network: policy_reference.logits_exact32 / select
    walk(...)           (entry uint8 [M], deepest int32 [L], exhausted bool [L]) of an action per state, ANY bytes
    root_moves(...)     int16 [L] over given entries
    score(...)          int32 [L, 8]
    expert(ref)         uint8 [M]: the lowest best move of the reference, 255 where there is none
    mixed_policy(...)   the tabular policy of the input conditions
    rows_of(...)        (rows uint64 [L, slots], slot int64 [M])
    scatter(...)        a flat array laid into [L, slots] rows"""
import numpy as np

import policy_reference as pref
import rstarts_reference as rs
import rtable_reference as rt

MAX_DEPTH, DEEP, NONE, WON = rt.MAX_DEPTH, rt.DEEP, rt.NONE, rt.WON
NO_ACTION = 255
ABSENT = rt.SOLVE_ABSENT


def boards(orc, ref, blk, tgt, which=None):
    """One oracle board per state of the Reference (or per state of `which`, positions in it), standing on it."""
    C = ref.S * ref.S
    which = np.arange(ref.idx.size) if which is None else np.asarray(which)
    level = ref.level[which]
    pos = rt.cells_of(ref.S, ref.T, ref.idx[which], orc.cell_dtype(ref.S))
    return orc.OracleBatch(ref.S, ref.mc, 2 ** 30, np.ascontiguousarray(np.asarray(blk, np.uint32)[:, level]), pos,
                           np.ascontiguousarray(np.minimum(np.asarray(tgt), C - 1)[:, level]))


def actions(orc, ref, blk, tgt, mlp, chunk=1 << 14):
    """mlp = (w1 [H, D], b1, w2 [4, H], b2) in torch.nn.Linear's layout, integer weights: exact in float32."""
    M = ref.idx.size
    act, logits = np.zeros(M, np.uint8), np.zeros((M, 4), np.float32)
    for a in range(0, M, chunk):   # the one-hot planes stay small
        b = boards(orc, ref, blk, tgt, np.arange(a, min(a + chunk, M)))
        logits[a:a + chunk] = pref.logits_exact32(b.encode_onehot().reshape(b.n, -1), mlp)
    if M:
        act = pref.select(logits, None, pref.GREEDY)
    return act, logits


def successor(ref, act):
    """int64 [M]: succ of the header as a position, WON, or the state itself where act > 3."""
    act = np.asarray(act)
    me = np.arange(ref.idx.size)
    return np.where(act <= 3, ref.succ[np.minimum(act, 3), me], me)


def walk(ref, act, max_depth=MAX_DEPTH):
    assert 0 <= max_depth <= MAX_DEPTH
    M, L = ref.idx.size, len(ref.count)
    succ = successor(ref, act)
    dist = np.full(M, NONE, np.int64)
    present = np.zeros((L, max_depth + 2), bool)   # present[n, d]: something of level n lies at distance exactly d
    for d in range(1, max_depth + 1):
        hit = (succ == WON) if d == 1 else ((succ != WON) & (dist[np.maximum(succ, 0)] == d - 1))
        hit = hit & (dist == NONE)
        if not hit.any():
            break
        dist[hit] = d
        present[ref.level[hit], d] = True
    present[:, 0] = True
    exhausted = ~present[:, :max_depth + 1].all(axis=1)
    entry = np.where(dist != NONE, dist, np.where(exhausted[ref.level], NONE, DEEP)).astype(np.uint8)
    deepest = np.zeros(L, np.int32)
    finite = dist != NONE
    np.maximum.at(deepest, ref.level[finite], dist[finite].astype(np.int32))
    return entry, deepest, exhausted


def root_moves(orc, ref, blk, tgt, root, entry):
    """0 for a won root, SOLVE_FULL for a FULL level, SOLVE_ABSENT where the level does not hold the root, else its entry mapped."""
    C = ref.S * ref.S
    root, tgt = np.ascontiguousarray(np.minimum(root, C - 1)), np.ascontiguousarray(np.minimum(tgt, C - 1))
    won0 = orc.OracleBatch(ref.S, ref.mc, 2 ** 30, np.ascontiguousarray(blk), root, tgt).won() != 0
    out = np.where(won0, 0, rt.SOLVE_FULL).astype(np.int16)
    live = np.flatnonzero(~won0 & (ref.count >= 0))
    glob = (ref.level << 48) | ref.idx
    want = (live.astype(np.int64) << 48) | rt.keys_of(ref.S, root[:, live])
    at = np.minimum(np.searchsorted(glob, want), max(glob.size - 1, 0))
    held = glob[at] == want if glob.size else np.zeros(live.size, bool)
    out[live] = np.where(held, rt.to_moves(np.asarray(entry)[at]) if glob.size else 0, ABSENT)
    return out


def score(ref, p, act, o=None):
    """p [M]: the policy's entries (any bytes), act [M] any bytes, o [M]: the table's entries (default: the Reference's)."""
    L = len(ref.count)
    p, act = np.asarray(p).astype(np.int64), np.asarray(act)
    o = ref.entry.astype(np.int64) if o is None else np.asarray(o).astype(np.int64)
    succ = successor(ref, act)
    solvable, solved = (o >= 1) & (o <= MAX_DEPTH), (p >= 1) & (p <= MAX_DEPTH)
    after = np.where(succ == WON, 0, o[np.maximum(succ, 0)])
    agree = solvable & (act <= 3) & (after == o - 1)
    both = solved & solvable
    cols = (np.ones_like(solved), solvable, solved, solved & (p == o), agree, np.where(both, p - o, 0), p == DEEP, p == 0)
    out = np.zeros((L, 8), np.int64)
    for k, c in enumerate(cols):
        np.add.at(out[:, k], ref.level, c.astype(np.int64))
    return out.astype(np.int32)


def expert(ref):
    e = ref.entry.astype(np.int64)
    after = np.where(ref.succ == WON, 0, e[np.maximum(ref.succ, 0)])
    best = ((e >= 1) & (e <= MAX_DEPTH))[None, :] & (after == e[None, :] - 1)
    return np.where(best.any(axis=0), np.argmax(best, axis=0), NO_ACTION).astype(np.uint8)


def mixed_policy(ref, seed):
    """Expert on two states of three, a random byte otherwise, a random move on every fifth."""
    M = ref.idx.size
    rng = np.random.default_rng(seed)
    act = np.where(rng.random(M) < 2 / 3, expert(ref), rng.integers(0, 256, M)).astype(np.uint8)
    act[1::5] = rng.integers(0, 4, len(act[1::5]))
    return act


def rows_of(ref, slots, order="forward", full_seed=5):
    """Device-format rows of the Reference's entries, filled on the host; a FULL level (no state is kept for it) gets words of
    random bits, half of them with bit 63 set: nothing of it may be read as a state.  order "reversed": the states are inserted
    from the largest key down - other slots, the same sets."""
    L = len(ref.count)
    rows, slot = np.zeros((L, slots), np.uint64), np.zeros(ref.idx.size, np.int64)
    rng = np.random.default_rng(full_seed)
    for n in range(L):
        a, b = ref.start[n], ref.start[n + 1]
        if ref.count[n] < 0:
            assert a == b
            rows[n] = rng.integers(0, 1 << 63, slots, dtype=np.uint64) << np.uint64(rng.integers(0, 2))
            rows[n, ::2] |= rs.OCC
            continue
        assert b - a == ref.count[n] <= slots // 2
        row = rs.fill_row(ref.idx[a:b], ref.entry[a:b], slots, None if order == "forward" else range(b - a - 1, -1, -1))
        rows[n] = row
        held = np.flatnonzero(row)
        slot[a:b] = held[np.argsort(row[held] & rs.KEY_MASK)]   # the keys of a level ascend
    return rows, slot


def scatter(ref, slot, values, slots, fill, dtype=None):
    """[L, slots] (+ the trailing shape of values): `values` [M, ...] in the slots of their states, `fill` everywhere else."""
    values = np.asarray(values)
    out = np.full((len(ref.count), slots) + values.shape[1:], fill, dtype or values.dtype)
    out[ref.level, slot] = values
    return out


def table_words(ref, entry):
    """uint64 [M]: the slot words of the states with the given entries."""
    return rs.words_of(ref.idx, entry)


def deep_reference(orc, lv):
    """Of a level of deep_cases, from its init: (Reference, the chain policy restricted to R uint8 [|R|], its chains int32 [|R|])."""
    import deep_cases as deep
    ref = rt.build(orc, lv.S, lv.mc, lv.blk, lv.tgt, lv.init)
    act, chain = deep.chain_policy(orc, lv)
    return ref, act[ref.idx].copy(), chain[ref.idx].copy()
