#!/usr/bin/env python3
"""Times ts_rtable_build and ts_rtable_lookup (include/tiler_slider_rtable.h) on one GPU: HIP events around 50 launches after warm-up.

    python tools/rtable_timing.py [--log FILE] [--launches 50] [--levels 16384] [--boards 1048576]

Shapes the dense tables refuse, the reference's random levels from seeds, capacity 4,096.  The build of all levels, beside
ts_reach_solve on the same levels with the same capacity and depth: the build does strictly more - it expands every reachable
state and not only those up to the first win, and then runs the rounds - and the log says how much.  Then the lookup at `boards`
boards that replicate the levels through rows= and stand three random moves from their root, beside ts_reach_solve on the same
boards: how the parent of this library answers that question.  Every figure is taken after the first 256 answers were compared
with the CPU yardstick (tests/rtable_reference.py).  profiles/rtable_timing.log is a run of this script.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--levels", type=int, default=1 << 14)
    ap.add_argument("--boards", type=int, default=1 << 20)
    args = ap.parse_args()
    import torch
    from oracle import binding as orc
    import rtable_reference as ref
    from tiler_slider_amd import ReachTable, VecTilerSliderEnv
    from tiler_slider_amd import _reach_cabi as rc
    from tiler_slider_amd import _rtable_cabi as xc

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

    def timed(fn):
        once = time_us(fn, 1)
        launches = max(1, min(args.launches, int(20e6 / max(once, 1))))   # at most 20 s a figure
        return time_us(fn, launches), launches

    def reach_call(env, capacity, max_depth):
        """(launch, moves, states): ts_reach_solve on the boards of env as they stand, in a workspace of 1 GiB at most."""
        n = env.num_envs
        moves, best, states = (torch.empty(n, dtype=dt, device=dev) for dt in (torch.int16, torch.uint8, torch.int32))
        d = rc.describe_reach(env._dims, max_depth, capacity, 1 << 30)
        ws = torch.empty(d["boards_in_flight"] * d["bytes_per_board"] // 8, dtype=torch.int64, device=dev)
        cfg = rc.ReachCfg(max_depth, capacity, ws.data_ptr(), ws.numel() * 8)
        out = rc.ReachOut(moves.data_ptr(), best.data_ptr(), states.data_ptr())
        keep = (ws, best)
        return (lambda: (keep, rc.check(rc.lib().ts_reach_solve(C.byref(env._dims), C.byref(env._state), C.byref(cfg), C.byref(out), stream()), "ts_reach_solve"))), moves, states

    def run(label, S, T, K, mc, capacity=4096, max_depth=252):
        L, n, k = args.levels, args.boards, min(args.levels, 256)
        env = VecTilerSliderEnv.from_seeds(np.arange(L, dtype=np.int64), size=S, num_tiles=T, num_obstacles=K, multi_color=mc, obs_dtype=None, device=dev)
        slots = xc.slots(capacity)
        table = torch.empty((L, slots), dtype=torch.int64, device=dev)
        count, root_moves, deepest = (torch.empty(L, dtype=dt, device=dev) for dt in (torch.int32, torch.int16, torch.int32))
        d = xc.describe_rtable_build(env._dims, max_depth, capacity, 1 << 30)
        ws = torch.empty(d["levels_in_flight"] * d["workspace_bytes"] // 8, dtype=torch.int64, device=dev)
        cfg = xc.RtableCfg(max_depth, capacity, xc.ROOT_INIT, ws.data_ptr(), ws.numel() * 8)
        out = xc.RtableOut(table.data_ptr(), count.data_ptr(), root_moves.data_ptr(), deepest.data_ptr())
        build = lambda: xc.check(xc.lib().ts_rtable_build(C.byref(env._dims), C.byref(env._state), C.byref(cfg), C.byref(out), stream()), "ts_rtable_build")
        build()
        # the first 256 levels against the yardstick, before any figure
        blk, init, tgt = orc.generate_mt19937(S, T, T, K, np.arange(k, dtype=np.uint32))
        want = ref.build(orc, S, mc, blk, tgt, init, max_depth, capacity)
        for name, g, w in (("count", count, want.count), ("root_moves", root_moves, want.root_moves), ("deepest", deepest, want.deepest)):
            assert np.array_equal(g[:k].cpu().numpy(), w), name
        rtab = ReachTable(table, count, root_moves, deepest, capacity, S, T, T, mc, max_depth, "init")
        for lv in range(k):
            keys, entries = rtab.entries(lv)
            assert np.array_equal(keys.cpu().numpy(), want.keys(lv)) and np.array_equal(entries.cpu().numpy(), want.entries(lv)), lv
        c = count.cpu().numpy().astype(np.int64)
        held = np.maximum(c, 0)
        say(f"{label}: {L} levels, capacity {capacity}, max_depth {max_depth}; {d['name']}, {d['blocks']} blocks of {d['threads_per_block']}, "
            f"{d['table_bytes']} B of table and {d['workspace_bytes']} B of workspace per level, table {table.numel() * 8 >> 20} MiB, workspace {ws.numel() * 8 >> 20} MiB")
        say(f"    full {(c == ref.SOLVE_FULL).sum()}, won as they stand {(c == 0).sum()}, roots that can be won {(root_moves >= 1).sum().item()}; "
            f"states held: mean {held.mean():.0f}, most {held.max()}, {held.sum() / 1e6:.1f} M in all; deepest entry {deepest.max().item()}")
        us, launches = timed(build)
        say(f"    ts_rtable_build  {us:12.1f} us per launch ({launches} launches), {us * 1e3 / L:10.1f} ns per level, {held.sum() / us:8.1f} states per us")
        solve, m, st = reach_call(env, capacity, max_depth)
        solve()
        assert bool(((m == root_moves) | (root_moves == ref.SOLVE_FULL)).all()), "ts_reach_solve disagrees with root_moves"   # (a search can end before its budget does)
        us2, launches = timed(solve)
        expanded = st.cpu().numpy().astype(np.int64).sum()
        say(f"    ts_reach_solve   {us2:12.1f} us per launch ({launches} launches) on the same levels, {expanded / 1e6:.1f} M states expanded: "
            f"the build holds {held.sum() / max(expanded, 1):.2f} times as many states and takes {us / us2:.2f} times as long")
        # the lookup: n boards that replicate the levels, three random moves from the root
        rows = (torch.arange(n, device=dev) % L).to(torch.int32)
        blk_d, init_d, tgt_d = (t[:, rows.long()].contiguous().cpu().numpy() for t in (env._blk.view(torch.int32), env._init, env._tgt))
        boards = VecTilerSliderEnv.from_arrays(S, blk_d.view(np.uint32), init_d, tgt_d, multi_color=mc, obs_dtype=None, device=dev, max_steps=1 << 30)
        boards.reset()
        boards.rollout(3, "random", seed=0x7AB1E, stats=False)
        moves, best, action = (torch.empty(n, dtype=dt, device=dev) for dt in (torch.int16, torch.uint8, torch.uint8))
        look = lambda: xc.check(xc.lib().ts_rtable_lookup(C.byref(boards._dims), C.byref(boards._state), table.data_ptr(), slots, count.data_ptr(), L,
                                                          rows.data_ptr(), moves.data_ptr(), best.data_ptr(), action.data_ptr(), stream()), "ts_rtable_lookup")
        look()
        first = rows[:k].cpu().numpy()
        assert (first < k).all()
        got = ref.lookup(orc, want, blk_d[:, :k].view(np.uint32), tgt_d[:, :k], boards._pos[:, :k].cpu().numpy(), rows=first)
        for name, g, w in zip(("moves", "best", "action"), (moves, best, action), got):
            assert np.array_equal(g[:k].cpu().numpy(), w), name
        mv = moves.cpu().numpy()
        say(f"    {n} boards three random moves from their root: won {(mv == 0).sum()}, a distance {(mv >= 1).sum()}, none {(mv == ref.SOLVE_NONE).sum()}, "
            f"full {(mv == ref.SOLVE_FULL).sum()}, absent {(mv == ref.SOLVE_ABSENT).sum()}")
        us3, launches = timed(look)
        say(f"    ts_rtable_lookup {us3:12.1f} us per launch ({launches} launches), {us3 * 1e3 / n:10.2f} ns per board (moves, best and action)")
        solve, m, st = reach_call(boards, capacity, max_depth)
        solve()
        assert bool(((m == moves) | (moves == ref.SOLVE_FULL)).all()), "ts_reach_solve disagrees with the lookup"
        us4, launches = timed(solve)
        say(f"    ts_reach_solve   {us4:12.1f} us per launch ({launches} launches) on the same boards: the lookup takes {us3 / us4:.5f} times as long "
            f"({us4 / us3:.0f} times faster); {us / max(us4 - us3, 1e-9):.2f} such calls pay for the build"
            if us4 > us3 else f"    ts_reach_solve   {us4:12.1f} us per launch on the same boards: THE LOOKUP IS NOT FASTER ({us3:.1f} us)")

    run("5x5 / 4 tiles / 3 obstacles", 5, 4, 3, True)
    run("8x8 / 3 tiles / 10 obstacles", 8, 3, 10, False)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        open(args.log, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
