"""CPU yardstick of the reach-table curricula (test infrastructure, no test of its own): the definition of
include/tiler_slider_rstarts.h restated on NumPy.  It starts from rtable_reference.Reference - per level the keys in ascending
order and their entries; no hash table -, orders a level by np.lexsort on (entry, key), finds `first` with np.searchsorted, and
places with a loop per board and the draw of rollout_reference.draws.  It shares no code and no method with
tiler_slider_amd/csrc/ts_rstarts.hip: no network, no tickets, no binary search of its own.
Imports neither torch nor the libraries at import time.

    index(ref, W)           (sorted uint64 [L, W], first int32 [L, 256]) of a Reference
    index_of_pairs(...)     the same for one level given as (keys, entries)
    fill_row(...)           a hash row made on the host from (key, entry) pairs by the header's slot format alone
    place(...)              what ts_rstarts_place reports and writes, as starts_reference.place does for the dense call"""
import numpy as np

import rollout_reference as rref

MAX_DEPTH, DEEP, NONE = 252, 254, 255
OCC = np.uint64(1 << 63)
KEY_MASK = np.uint64((1 << 48) - 1)
FIRST = 256
ALL, DONE = 0, 1
HOME_MUL = 0x9e3779b97f4a7c15

# kernel name -> (S, T, K): one occupancy case per placement kernel, on the shapes of reach_cases
N_OCC = 4096 * 64 - 3   # 262,141 boards: 4,096 waves, the last one ragged


def occupancy_cases():
    import reach_cases
    return {f"k_rstarts_place<{S}>": (S, T, K) for S, (T, K, _) in reach_cases.SHAPES.items()}


_CASES = {}


def case(orc, S, mc, capacity=None):
    """(blk, init, tgt, Reference, sorted, first) of reach_cases.levels(S, mc) at reach_cases.CAPACITY, built once per process and
    shared: nobody writes to it."""
    import reach_cases
    import rtable_reference as rt
    capacity = reach_cases.CAPACITY if capacity is None else capacity
    if (S, mc, capacity) not in _CASES:
        blk, init, tgt = reach_cases.levels(orc, S, mc)
        ref = rt.build(orc, S, mc, blk, tgt, init, MAX_DEPTH, capacity)
        _CASES[S, mc, capacity] = (blk, init, tgt, ref) + index(ref, capacity)
    return _CASES[S, mc, capacity]


def words_of(keys, entries):
    return OCC | (np.asarray(entries).astype(np.uint64) << np.uint64(48)) | np.asarray(keys).astype(np.uint64)


def index_of_pairs(keys, entries, W):
    """(sorted uint64 [W], first int32 [256]) of one level that holds the distinct `keys` with `entries`; more than W pairs: an
    empty index."""
    keys, entries = np.asarray(keys, np.int64), np.asarray(entries, np.int64)
    out, first = np.zeros(W, np.uint64), np.zeros(FIRST, np.int32)
    if keys.size > W:
        return out, first
    order = np.lexsort((keys, entries))   # the last key is the primary one
    out[:keys.size] = words_of(keys[order], entries[order])
    first[:] = np.searchsorted(entries[order], np.arange(FIRST), side="left")
    return out, first


def index(ref, W):
    """The band index of every level of an rtable_reference.Reference; a FULL level (count < 0) or one above W is empty."""
    L = len(ref.count)
    out, first = np.zeros((L, W), np.uint64), np.zeros((L, FIRST), np.int32)
    for n in range(L):
        if 0 <= ref.count[n] <= W:
            out[n], first[n] = index_of_pairs(ref.keys(n), ref.entries(n), W)
    return out, first


def home_of(key, slots):
    log2 = int(slots).bit_length() - 1
    return ((((int(key) * HOME_MUL) & ((1 << 64) - 1)) >> 32) & 0xffffffff) >> (32 - log2)


def fill_row(keys, entries, slots, order=None):
    """uint64 [slots]: every (key, entry) in the first free slot of its probe sequence - home slot, then slot + 1 modulo slots -,
    inserted in `order` (default: as given).  Another order gives other bits and the same set."""
    row = [0] * slots
    words, keys = words_of(keys, entries).tolist(), np.asarray(keys).tolist()
    for i in (range(len(words)) if order is None else order):
        at = home_of(keys[i], slots)
        while row[at]:
            at = (at + 1) & (slots - 1)
        row[at] = words[i]
    return np.array(row, np.uint64)


def synthetic_pairs(n, seed, key_bits=48):
    """n distinct keys below 2 ** key_bits and entries over 1 .. 40, DEEP and NONE, from `seed`."""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, 1 << key_bits, int(n * 1.1) + 8, dtype=np.int64))
    assert keys.size >= n
    keys = rng.permutation(keys)[:n]
    kinds = rng.integers(0, 10, n)
    entries = np.where(kinds < 7, rng.integers(1, 41, n), np.where(kinds < 8, DEEP, NONE)).astype(np.int64)
    return keys, entries


def place_many(sorted_, first, C, T, n_boards, lo=1, hi=MAX_DEPTH, band=None, rows=None, selected=None, seed=0, step_index=0, board_offset=0):
    """place() for batches too large for a loop per board: the same definition on whole arrays (tests/test_rstarts_cpu.py holds
    the two against each other).  Returns place()'s dict."""
    n_rows, W = sorted_.shape
    N = int(n_boards)
    R = rref.draws(N, seed, step_index, board_offset)
    r = np.arange(N, dtype=np.int64) if rows is None else np.asarray(rows).astype(np.int64)
    inside = (r >= 0) & (r < n_rows)
    rr = np.where(inside, r, 0)
    lo_n = np.full(N, int(lo), np.int64) if band is None else band[0].astype(np.int64)
    hi_n = np.full(N, int(hi), np.int64) if band is None else band[1].astype(np.int64)
    f = first.astype(np.int64)
    a, b = np.minimum(f[rr, lo_n], W), np.minimum(f[rr, np.minimum(hi_n, MAX_DEPTH) + 1], W)
    count = np.where(inside, np.maximum(b - a, 0), 0)
    finite = np.where(inside, np.minimum(f[rr, MAX_DEPTH + 1], W), 0)
    deepest = np.where(finite > 0, (sorted_[rr, np.maximum(finite - 1, 0)] >> np.uint64(48)) & np.uint64(0xff), 255).astype(np.uint8)
    placed = (count > 0) & (np.ones(N, bool) if selected is None else np.asarray(selected, bool))
    j = (((R >> np.uint64(32)) * count.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)   # count <= 2^30: below 2^62
    w = sorted_[rr, np.where(placed, a + j, 0)]
    key = np.where(placed, (w & KEY_MASK).astype(np.int64), -1)
    cells = np.stack([np.where(placed, (np.maximum(key, 0) // C ** t) % C, 0) for t in range(T)]).astype(np.uint8) if T else np.zeros((0, N), np.uint8)
    dist = np.where(placed, (w >> np.uint64(48)) & np.uint64(0xff), 255).astype(np.uint8)
    return dict(count=count.astype(np.int32), dist=dist, deepest=deepest, placed=placed, key=key, cells=cells)


def place(sorted_, first, C, T, n_boards, lo=1, hi=MAX_DEPTH, band=None, rows=None, selected=None, seed=0, step_index=0, board_offset=0):
    """sorted_ uint64 [n_rows, W], first int32 [n_rows, 256] of a built index, C = S * S cells, T tiles.  band uint8 [2, N]
    overrides lo / hi; rows int [N] (default: board n reads row n; an index outside is no row); selected bool [N] (default:
    every board).  Returns a dict: count int32 [N], dist uint8 [N], deepest uint8 [N], placed bool [N], key int64 [N] (-1 where not
    placed) and cells uint8 [T, N] (0 where not placed: compare under `placed` only)."""
    n_rows, W = sorted_.shape
    N = int(n_boards)
    R = rref.draws(N, seed, step_index, board_offset)
    out = dict(count=np.zeros(N, np.int32), dist=np.full(N, 255, np.uint8), deepest=np.full(N, 255, np.uint8),
               placed=np.zeros(N, bool), key=np.full(N, -1, np.int64), cells=np.zeros((T, N), np.uint8))
    for n in range(N):
        r = n if rows is None else int(rows[n])
        if not 0 <= r < n_rows:
            continue
        lo_n, hi_n = (int(band[0, n]), int(band[1, n])) if band is not None else (int(lo), int(hi))
        a, b = min(int(first[r, lo_n]), W), min(int(first[r, min(hi_n, MAX_DEPTH) + 1]), W)
        count = max(b - a, 0)
        out["count"][n] = count
        finite = min(int(first[r, MAX_DEPTH + 1]), W)
        if finite:
            out["deepest"][n] = (int(sorted_[r, finite - 1]) >> 48) & 0xff
        if count == 0 or (selected is not None and not selected[n]):
            continue
        j = ((int(R[n]) >> 32) * count) >> 32
        w = int(sorted_[r, a + j])
        key = w & ((1 << 48) - 1)
        out["placed"][n], out["key"][n], out["dist"][n] = True, key, (w >> 48) & 0xff
        for t in range(T):
            out["cells"][t, n] = (key // C ** t) % C
    return out
