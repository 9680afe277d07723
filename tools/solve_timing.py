#!/usr/bin/env python3
"""Times ts_solve (include/tiler_slider_search.h) on one GPU: HIP events around 50 launches after warm-up.

    python tools/solve_timing.py [--log FILE] [--launches 50] [--quick]

Per shape: the library's own launch form and, where both forms exist, the other one (ts_search_tuning moves the boundary),
with and without the `best` output; beside it one ts_is_won launch on the same batch (the floor of any launch that reads the
same state) and the CPU yardstick's time per board (tests/solver_reference.py on a sample).  The answers of every timed form
are compared with the library's default form before anything is timed.  profiles/solver_timing.log is a run of this script;
`rocprofv3 --kernel-trace --stats -- python tools/solve_timing.py --quick` adds kernel names, registers and LDS.
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
    ap.add_argument("--quick", action="store_true", help="default forms only, no CPU yardstick (for a profiler run)")
    args = ap.parse_args()
    import torch
    from oracle import binding as orc
    import solver_reference as ref
    from tiler_slider_amd import VecTilerSliderEnv, _cabi
    from tiler_slider_amd import _search_cabi as sc
    from tiler_slider_amd.levels import pack_levels

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    L, LS = _cabi.lib(), sc.lib()
    dev = torch.device("cuda", 0)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def time_us(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches

    def run(label, env, sample_levels, variants):
        n = env.num_envs
        moves = torch.empty(n, dtype=torch.int16, device=dev)
        best = torch.empty(n, dtype=torch.uint8, device=dev)
        won = torch.empty(n, dtype=torch.uint8, device=dev)
        solve = lambda b: sc.check(LS.ts_solve(C.byref(env._dims), C.byref(env._state), 64, moves.data_ptr(), b, stream()), "ts_solve")
        floor = time_us(lambda: _cabi.check(L.ts_is_won(C.byref(env._dims), C.byref(env._state), won.data_ptr(), stream()), "ts_is_won"))
        say(f"{label}: {n} boards; ts_is_won {floor:9.1f} us")
        base = None
        for name, states, wpl in variants:
            LS.ts_search_tuning(sc.TUNE_WAVE_MAX_STATES, states)
            LS.ts_search_tuning(sc.TUNE_WORDS_PER_LANE, wpl)
            d = sc.describe_solve(env._dims)
            solve(best.data_ptr())
            torch.cuda.synchronize()
            got = (moves.clone(), best.clone())
            if base is None:
                base = got
                solvable = int((got[0] >= 1).sum())
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), "forms disagree"
            with_best, without = time_us(lambda: solve(best.data_ptr())), time_us(lambda: solve(None))
            say(f"    {name:<22} {d['name']:<17} lanes/board {d['lanes_per_board']:>3}  LDS/block {d['lds_bytes_block']:>6} B  blocks {d['blocks']:>7}  "
                f"with best {with_best:10.1f} us ({with_best * 1e3 / n:8.2f} ns/board)  without {without:10.1f} us")
        LS.ts_search_tuning(sc.TUNE_WAVE_MAX_STATES, states0)
        LS.ts_search_tuning(sc.TUNE_WORDS_PER_LANE, wpl0)
        say(f"    solvable {solvable} of {n}, deepest optimum {int(base[0].max())}")
        if sample_levels is not None and not args.quick:
            S, mc, blk, init, tgt = sample_levels
            t0 = time.perf_counter()
            want = ref.solve(orc, S, mc, blk, tgt, init)
            dt = time.perf_counter() - t0
            k = blk.shape[1]
            assert np.array_equal(want[0], base[0][:k].cpu().numpy()) and np.array_equal(want[1], base[1][:k].cpu().numpy())
            say(f"    CPU yardstick (moves and best, {k} boards, equal to the kernel's): {dt * 1e6 / k:8.1f} us/board")

    states0, wpl0 = LS.ts_search_tuning(sc.TUNE_WAVE_MAX_STATES, -1), LS.ts_search_tuning(sc.TUNE_WORDS_PER_LANE, -1)
    DEFAULT = ("library policy", states0, wpl0)
    BLOCK, WAVE = ("block form forced", 0, 1), ("wave form forced", 65536, 1)
    shapes = [  # label, S, T, K, mc, boards, variants
        ("4x4 / 2 tiles (cfg1)", 4, 2, 2, False, 1 << 20, [DEFAULT, ("wave, 2 words/lane", 65536, 2), ("wave, 4 words/lane", 65536, 4), ("wave, 8 words/lane", 65536, 8), BLOCK]),
        ("5x5 / 3 tiles", 5, 3, 3, True, 1 << 18, [DEFAULT, WAVE, ("wave, 8 words/lane", 65536, 8)]),
        ("6x6 / 3 tiles", 6, 3, 6, False, 1 << 14, [DEFAULT, WAVE]),
    ]
    if not args.quick:  # the boundary between the forms: index spaces in between, both forms
        shapes += [("5x5 / 2 tiles (625 states)", 5, 2, 3, False, 1 << 18, [DEFAULT, ("wave, 2 words/lane", 65536, 2), ("wave, 4 words/lane", 65536, 4), BLOCK]),
                   ("6x6 / 2 tiles (1296 states)", 6, 2, 6, False, 1 << 17, [DEFAULT, ("wave, 2 words/lane", 65536, 2), BLOCK]),
                   ("4x4 / 3 tiles (4096 states)", 4, 3, 2, True, 1 << 17, [DEFAULT, ("wave, 2 words/lane", 65536, 2), BLOCK]),
                   ("3x3 / 4 tiles (6561 states)", 3, 4, 1, False, 1 << 17, [DEFAULT, BLOCK, ("wave, 2 words/lane", 65536, 2)]),
                   ("4x4 / 4 tiles (65536 states)", 4, 4, 2, True, 1 << 13, [DEFAULT, WAVE])]
    for label, S, T, K, mc, n, variants in shapes:
        seeds = np.arange(n, dtype=np.int64)
        env = VecTilerSliderEnv.from_seeds(seeds, size=S, num_tiles=T, num_obstacles=K, multi_color=mc, obs_dtype=None, device=dev)
        k = min(n, 2048)
        blk, init, tgt = orc.generate_mt19937(S, T, T, K, np.arange(k, dtype=np.uint32))
        run(label, env, (S, mc, blk, init, tgt), variants[:1] if args.quick else variants)
        del env
    for (S, T, mc), (ids, blk, init, tgt, want) in ref.fixture_groups(os.path.join(ROOT, "tests", "golden"), pack_levels).items():
        env = VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=mc, obs_dtype=None, device=dev)
        run(f"screenshot levels {S}x{S} / {T} tiles {'multi' if mc else 'single'}", env, (S, mc, blk, init, tgt), [DEFAULT])
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        open(args.log, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
