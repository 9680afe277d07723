"""CPU yardstick of the curriculum starts (test infrastructure, no test of its own): the definition of
include/tiler_slider_starts.h restated on NumPy - a loop per board over np.flatnonzero(match), the draw from
rollout_reference.draws.  It shares no method with tiler_slider_amd/csrc/ts_starts.hip: no pieces, no prefix sums, no masks.
Imports neither torch nor the libraries at import time."""
import numpy as np

import rollout_reference as rref
from table_harness import _OCC_SHAPES

MAX_DEPTH = 252
ALL, DONE = 0, 1

# kernel name -> (S, T): one occupancy case per kernel of the starts library, on the shapes of the table library's cases.
# tests/test_gpu_starts.py runs them at OCC_BLOCKS one-wave blocks and more, tests/test_starts_cpu.py pins the names to the code object
OCCUPANCY_CASES = {f"k_starts_place<{_S}>": (_S, _T) for _S, (_T, _K) in _OCC_SHAPES.items()}
OCC_BLOCKS, OCC_ROWS = 4096, 128


def occupancy_boards(boards_per_block):
    """Boards that fill OCC_BLOCKS blocks and leave the last one ragged where a block holds more than one board."""
    return OCC_BLOCKS * boards_per_block + boards_per_block // 2 + 1


def place(table, C, T, n_boards, lo=1, hi=MAX_DEPTH, band=None, rows=None, selected=None, seed=0, step_index=0, board_offset=0):
    """table uint8 [n_rows, states] (any bytes), C = S * S cells, T tiles.  band uint8 [2, N] overrides lo / hi; rows int [N]
    (default: board n reads row n; an index outside the table is no row); selected bool [N] (default: every board).
    Returns a dict: count int32 [N], dist uint8 [N], deepest uint8 [N], placed bool [N], idx int64 [N] (-1 where not placed) and
    cells uint8 [T, N] (0 where not placed: compare under `placed` only)."""
    table = np.asarray(table, np.uint8)
    n_rows = table.shape[0]
    N = int(n_boards)
    R = rref.draws(N, seed, step_index, board_offset)
    out = dict(count=np.zeros(N, np.int32), dist=np.full(N, 255, np.uint8), deepest=np.full(N, 255, np.uint8),
               placed=np.zeros(N, bool), idx=np.full(N, -1, np.int64), cells=np.zeros((T, N), np.uint8))
    for n in range(N):
        r = n if rows is None else int(rows[n])
        if not 0 <= r < n_rows:
            continue
        e = table[r].astype(np.int64)
        lo_n, hi_n = (int(band[0, n]), int(band[1, n])) if band is not None else (int(lo), int(hi))
        matching = np.flatnonzero((e >= lo_n) & (e <= min(hi_n, MAX_DEPTH)))
        distances = e[e <= MAX_DEPTH]
        out["count"][n] = matching.size
        if distances.size:
            out["deepest"][n] = distances.max()
        if matching.size == 0 or (selected is not None and not selected[n]):
            continue
        j = ((int(R[n]) >> 32) * int(matching.size)) >> 32
        idx = int(matching[j])
        out["placed"][n], out["idx"][n], out["dist"][n] = True, idx, e[idx]
        for t in range(T):
            out["cells"][t, n] = (idx // C ** t) % C
    return out


def apply(ref, pos, init, step_count, done, write_pos, write_init):
    """The state after the call: copies of (pos, init, step_count, done) with the placed boards of `ref` written as the header says."""
    pos, init, step_count, done = pos.copy(), init.copy(), step_count.copy(), done.copy()
    p = ref["placed"]
    if write_pos:
        pos[:, p] = ref["cells"][:, p]
        step_count[p] = 0
        done[p] = 0
    if write_init:
        init[:, p] = ref["cells"][:, p]
    return pos, init, step_count, done
