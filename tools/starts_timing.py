#!/usr/bin/env python3
"""Times the curriculum starts (include/tiler_slider_starts.h) beside the torch composition they replace, on one GPU: HIP events
on the launch stream after warm-up, three windows a row with the rows of a shape taken in turn, the median window, one process.

    python tools/starts_timing.py [--log FILE] [--reps 20] [--quick]

Shapes, 4x4 boards with two tiles (256 placements a level), band [1, 252]:

    1,048,576 boards against their own table of 256 MiB - two copies of it taken in turn, so that no launch finds its table
              in the Infinity Cache the launch before left it in
    1,048,576 boards over rows= onto the 1,024 rows of their distinct levels
    4,096     boards against their own table

Rows: `place_at_distance` is VecTilerSliderEnv.place_at_distance(set_initial=True) on an environment without an observation: the
one launch of ts_starts_place.  `torch` is what a user writes today for the same result - a mask over [N, states], sum, cumsum,
a comparison and argmax for the j-th match, the decode, and torch.where writes into pos, init, step_count and done (its draw is
torch.rand: the composition is timed, not compared).  For the first shape the table bytes over the time stand beside the 6.3 TB/s
of HBM reads.  profiles/starts_timing.log is where a run of this script belongs; run it under `timeout`.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="65,536 boards instead of 1,048,576")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import DistanceTable, VecTilerSliderEnv
    from tiler_slider_amd import _starts_cabi as sc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.log:  # rewritten at every line: what was measured survives a run that ends early
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            open(args.log, "w").write("\n".join(lines) + "\n")

    dev = torch.device("cuda", 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, reps):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    def time_rows(rows, windows=3):
        """rows: {label: (fn, reps)}; every fn warmed, then `windows` rounds over the rows in turn: {label: median us}."""
        for fn, _ in rows.values():
            for _ in range(3):
                fn()
        got = {k: [] for k in rows}
        for _ in range(windows):
            for k, (fn, reps) in rows.items():
                got[k].append(window(fn, reps))
        return {k: sorted(v)[len(v) // 2] for k, v in got.items()}

    def torch_place(env, dists, rows, lo, hi, turn):
        """The composition: every board onto a uniformly drawn placement of its row with lo <= distance <= hi."""
        C = env.size * env.size
        dist = dists[turn[0] % len(dists)]
        e = dist if rows is None else dist[rows.long()]
        match = (e >= lo) & (e <= hi)
        count = match.sum(dim=1)
        deepest = torch.where(e <= 252, e, torch.zeros_like(e)).amax(dim=1)
        j = (torch.rand(env.num_envs, device=dev) * count).long().clamp_(max=255)
        idx = (match.cumsum(dim=1) > j.unsqueeze(1)).to(torch.uint8).argmax(dim=1)
        placed = count > 0
        d = torch.where(placed, e.gather(1, idx.unsqueeze(1)).squeeze(1), torch.full_like(deepest, 255))
        for t in range(env.n_tiles):
            cell = ((idx // C ** t) % C).to(torch.uint8)
            env._pos[t] = torch.where(placed, cell, env._pos[t])
            env._init[t] = torch.where(placed, cell, env._init[t])
        env._step_count.masked_fill_(placed, 0)
        env._done.masked_fill_(placed, 0)
        return count, d, deepest

    big = 1 << (16 if args.quick else 20)
    say(f"{args.reps} launches a window ({max(2, args.reps // 5)} of the torch composition), median of 3 windows; 4x4 boards, two tiles, band [1, 252]")
    for label, n, levels, copies in ((f"{big} boards, their own table", big, big, 2), (f"{big} boards, rows= onto 1,024 rows", big, 1024, 1),
                                     ("4,096 boards, their own table", 4096, 4096, 1)):
        seeds = np.arange(n, dtype=np.int64) % levels
        env = VecTilerSliderEnv.from_seeds(seeds, size=4, num_tiles=2, num_obstacles=2, obs_dtype=None, device=dev, max_steps=16, auto_reset=True)
        env.reset()
        if levels == n:
            table, rows = env.build_table(), None
        else:
            small = VecTilerSliderEnv.from_seeds(np.arange(levels, dtype=np.int64), size=4, num_tiles=2, num_obstacles=2, obs_dtype=None, device=dev)
            table, rows = small.build_table(), torch.from_numpy(seeds.astype(np.int32)).to(dev)
        tables = [table] + [DistanceTable(table.dist.clone(), table.size, table.n_tiles, table.n_targets, table.multi_color, table.max_depth)
                            for _ in range(copies - 1)]
        d = sc.describe_starts_place(env._dims)
        turn = [0]

        def fused():
            turn[0] += 1
            return env.place_at_distance(tables[turn[0] % copies], 1, 252, rows=rows, seed=7, step_index=turn[0])

        def composed():
            turn[0] += 1
            return torch_place(env, [t.dist for t in tables], rows, 1, 252, turn)

        info = fused()
        placed = float(info.placed.float().mean())
        res = time_rows({"fused": (fused, args.reps), "torch": (composed, max(2, args.reps // 5))})
        nbytes = table.dist.shape[1] * (n if rows is None else n)      # the rows the boards read: every board reads its row once
        say(f"{label}: {d['name']}, {d['lanes_per_board']} lanes a board, {d['blocks']} blocks; {100 * placed:.0f} % of the boards are placed")
        say(f"    place_at_distance {res['fused']:10.1f} us     torch composition {res['torch']:10.1f} us     x{res['torch'] / res['fused']:.0f}")
        if rows is None:
            say(f"    rows read: {nbytes / 2 ** 20:.0f} MiB in {res['fused']:.1f} us = {nbytes / res['fused'] / 1e6:.2f} TB/s, beside {HBM_TBS} TB/s of HBM reads"
                + ("" if copies > 1 else " (one table, launch after launch: it stays in the caches)"))
        else:
            say(f"    rows read: {nbytes / 2 ** 20:.0f} MiB out of a table of {table.dist.numel() / 2 ** 10:.0f} KiB, which stays in the caches")
        del env, tables, table
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
