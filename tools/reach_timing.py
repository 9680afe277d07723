#!/usr/bin/env python3
"""Times ts_reach_solve (include/tiler_slider_reach.h) on one GPU: HIP events around 50 launches after warm-up.

    python tools/reach_timing.py [--log FILE] [--launches 50] [--boards 65536] [--quick]

Shapes ts_solve refuses, random levels from seeds, capacity 8192 in a workspace of 1 GiB: us per launch, what the launch was
(ts_describe_reach), how the boards ended and how many states they expanded.  Then 4x4 with four tiles, 8,192 boards, against
ts_solve on the same boards (moves and best compared first).  Beside each the CPU yardstick's time per board
(tests/reach_reference.py on a sample, compared with the kernel's answer).  profiles/reach_timing.log is a run of this script.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--boards", type=int, default=1 << 16)
    ap.add_argument("--quick", action="store_true", help="no CPU yardstick")
    args = ap.parse_args()
    import torch
    from oracle import binding as orc
    import reach_reference as ref
    from tiler_slider_amd import VecTilerSliderEnv
    from tiler_slider_amd import _reach_cabi as rc
    from tiler_slider_amd import _search_cabi as sc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def time_us(fn, launches):
        fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches

    def run(label, S, T, K, mc, n, capacity, against_solve=False):
        env = VecTilerSliderEnv.from_seeds(np.arange(n, dtype=np.int64), size=S, num_tiles=T, num_obstacles=K, multi_color=mc, obs_dtype=None, device=dev)
        moves, best, states = (torch.empty(n, dtype=dt, device=dev) for dt in (torch.int16, torch.uint8, torch.int32))
        d = rc.describe_reach(env._dims, 64, capacity, 1 << 30)
        ws = torch.empty(d["boards_in_flight"] * d["bytes_per_board"] // 8, dtype=torch.int64, device=dev)
        cfg = rc.ReachCfg(64, capacity, ws.data_ptr(), ws.numel() * 8)
        out = rc.ReachOut(moves.data_ptr(), best.data_ptr(), states.data_ptr())
        reach = lambda: rc.check(rc.lib().ts_reach_solve(C.byref(env._dims), C.byref(env._state), C.byref(cfg), C.byref(out), stream()), "ts_reach_solve")
        once = time_us(reach, 1)
        m = moves.cpu().numpy()
        st = states.cpu().numpy()
        say(f"{label}: {n} boards, capacity {capacity}; {d['name']}, {d['blocks']} blocks of {d['threads_per_block']}, {d['bytes_per_board']} B per board, "
            f"workspace {ws.numel() * 8 >> 20} MiB")
        say(f"    solvable {(m >= 1).sum()}, none {(m == ref.SOLVE_NONE).sum()}, depth {(m == ref.SOLVE_DEPTH).sum()}, full {(m == ref.SOLVE_FULL).sum()}; "
            f"states expanded: mean {st.mean():.0f}, most {st.max()}, {st.sum() / 1e6:.1f} M in all; one launch {once:.0f} us")
        launches = max(1, min(args.launches, int(20e6 / max(once, 1))))   # at most 20 s a shape
        us = time_us(reach, launches)
        say(f"    ts_reach_solve {us:12.1f} us per launch ({launches} launches), {us * 1e3 / n:10.1f} ns per board, {st.sum() / us:8.1f} states per us")
        if against_solve:
            m2, b2 = torch.empty_like(moves), torch.empty_like(best)
            solve = lambda: sc.check(sc.lib().ts_solve(C.byref(env._dims), C.byref(env._state), 64, m2.data_ptr(), b2.data_ptr(), stream()), "ts_solve")
            solve()
            assert torch.equal(m2, moves) and torch.equal(b2, best), "ts_solve disagrees"
            us2 = time_us(solve, args.launches)
            say(f"    ts_solve       {us2:12.1f} us per launch on the same boards ({sc.describe_solve(env._dims)['name']}): the hashed form takes {us / us2:.2f} times as long")
        if not args.quick:
            k = min(n, 256)
            blk, init, tgt = orc.generate_mt19937(S, T, T, K, np.arange(k, dtype=np.uint32))
            t0 = time.perf_counter()
            want = ref.solve(orc, S, mc, blk, tgt, init, 64, capacity)
            dt = time.perf_counter() - t0
            assert all(np.array_equal(w, g[:k].cpu().numpy()) for w, g in zip(want, (moves, best, states)))
            say(f"    CPU yardstick ({k} boards, equal to the kernel's): {dt * 1e6 / k:8.1f} us per board")

    n = args.boards
    run("5x5 / 4 tiles / 3 obstacles", 5, 4, 3, True, n, 8192)
    run("8x8 / 3 tiles / 10 obstacles", 8, 3, 10, False, n, 8192)
    run("6x6 / 4 tiles / 6 obstacles", 6, 4, 6, False, n, 8192)
    run("4x4 / 4 tiles / 2 obstacles", 4, 4, 2, True, min(n, 8192), 65536, against_solve=True)   # capacity = the index space: never FULL
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        open(args.log, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
