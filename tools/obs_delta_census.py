#!/usr/bin/env python3
"""What the in-place step has to write: a census of the observation's changes per board-step, on the CPU with the oracle.

    python tools/obs_delta_census.py [--size 4] [--tiles 2] [--obstacles 2] [--boards 131072] [--settle 1024] [--steps 32]

bench.py's levels (LEVEL_SEED, multi colour, as many targets as tiles) and its ring of sixteen action buffers (ACTION_SEED),
auto-reset, max_steps 2**30.  After --settle steps, for each of --steps steps: channel 1 of the float32 observation before
and after (obs[n, cell, 1] = 1 + the highest tile on the cell, 0 without one) gives the floats that change; their byte
addresses in the [boards][cells][3] float32 buffer give the distinct 32-byte sectors, 64-byte pieces and 128-byte lines that
the step dirties (a sector may belong to two boards: the count is over the buffer, not per board).  Prints the means per
board-step - the table of profiles/update_requests.md.  No GPU, no torch."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVEL_SEED = 0x715311DE
ACTION_SEED = 0xAC710005
FLAG_AUTORESET = 0x20
QUANTITIES = ("floats", "sectors_32", "pieces_64", "lines_128", "boards_changed", "boards_autoreset")


def channel1(pos, cells):
    """[boards][cells] of obs[..., 1] in multi colour: ascending tiles, the highest on a cell stays."""
    n = pos.shape[1]
    plane = np.zeros((n, cells), np.uint8)
    cols = np.arange(n)
    for t in range(pos.shape[0]):
        plane[cols, np.minimum(pos[t], cells - 1)] = t + 1
    return plane


def census(oracle, size, tiles, obstacles, boards, settle, steps):
    """dict of QUANTITIES -> mean per board-step over `steps` steps after `settle` steps."""
    cells = size * size
    blk, init, tgt = oracle.generate(size, tiles, tiles, obstacles, boards, seed=LEVEL_SEED)
    ring = [oracle.fill_actions(boards, seed=ACTION_SEED, step_index=i) for i in range(16)]
    ref = oracle.OracleBatch(size, True, 2**30, blk, init, tgt)
    ref.reset()
    for k in range(settle):
        ref.step(ring[k & 15], mode=oracle.MODE_AUTORESET, obs=False)
    total = dict.fromkeys(QUANTITIES, 0)
    before = channel1(np.array(ref.pos), cells)
    for k in range(settle, settle + steps):
        flags = ref.step(ring[k & 15], mode=oracle.MODE_AUTORESET, obs=False)["flags"]
        after = channel1(np.array(ref.pos), cells)
        board, cell = np.nonzero(after != before)
        address = 4 * (board.astype(np.int64) * (cells * 3) + 3 * cell + 1)  # byte offset of obs[board, cell, 1]
        total["floats"] += address.size
        total["sectors_32"] += np.unique(address >> 5).size
        total["pieces_64"] += np.unique(address >> 6).size
        total["lines_128"] += np.unique(address >> 7).size
        total["boards_changed"] += np.unique(board).size
        total["boards_autoreset"] += int(((flags & FLAG_AUTORESET) != 0).sum())
        before = after
    return {q: total[q] / (boards * steps) for q in QUANTITIES}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=4)
    ap.add_argument("--tiles", type=int, default=2)
    ap.add_argument("--obstacles", type=int, default=2)
    ap.add_argument("--boards", type=int, default=131072)
    ap.add_argument("--settle", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=32)
    args = ap.parse_args()
    from oracle import binding as oracle
    got = census(oracle, args.size, args.tiles, args.obstacles, args.boards, args.settle, args.steps)
    print(f"# {args.boards} boards {args.size}x{args.size}, {args.tiles} tiles, {args.obstacles} obstacles; {args.steps} steps after {args.settle}")
    print("| Quantity per board-step | Value |\n|---|---|")
    names = {"floats": "channel-1 floats that change", "sectors_32": "distinct 32-byte sectors", "pieces_64": "distinct 64-byte pieces",
             "lines_128": "distinct 128-byte lines", "boards_changed": "boards that change at all", "boards_autoreset": "boards that autoreset"}
    for q in QUANTITIES:
        print(f"| {names[q]} | {got[q]:.3f} |")


if __name__ == "__main__":
    main()
