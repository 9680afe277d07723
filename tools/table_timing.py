#!/usr/bin/env python3
"""Times the distance-to-win tables (include/tiler_slider_table.h) on one GPU: HIP events around 50 launches after warm-up.

    python tools/table_timing.py [--log FILE] [--launches 50] [--quick]

Per shape of DESIGN.md section 11's table, in one process and one run: ts_table_build in the library's own launch form and,
in both forms forced (ts_table_tuning moves the boundaries; the wave form also with more placements per lane),
then on the same boards ts_table_lookup (moves and best; the action alone), ts_solve of the search library (what the lookup
replaces) and ts_valid_moves (the same four slides without the five byte reads), and the break-even number of lookups,
build / (solve - lookup).  The boards are looked up where they stand after eight random steps.  Then both forms on small
batches of small index spaces (where one wave per board stops filling the GPU), and the build on the 400 screenshot levels,
the deep case, as they are and in 64 copies each.  The tables of every timed form are compared with the library's default form, and the lookup
with ts_solve, before anything is timed.  A build slower than 40 ms is timed over fewer launches (the line says how many).
profiles/table_timing.log is a run of this script; run it under `timeout`.
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
    ap.add_argument("--quick", action="store_true", help="default forms only, a sixteenth of the boards (for a profiler run)")
    args = ap.parse_args()
    import torch
    from oracle import binding as orc
    import solver_reference as ref
    from tiler_slider_amd import VecTilerSliderEnv, _cabi
    from tiler_slider_amd import _search_cabi as sc
    from tiler_slider_amd import _table_cabi as tc
    from tiler_slider_amd.levels import pack_levels

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    L, LS, LT = _cabi.lib(), sc.lib(), tc.lib()
    dev = torch.device("cuda", 0)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def time_us(fn, launches=None, warm=5):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        k = launches or args.launches
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k

    def time_build(fn):
        """(us per launch, launches): one launch first; a slow build is timed over as many launches as fit two seconds (at least 3)."""
        once = time_us(fn, launches=1, warm=1)
        k = int(min(args.launches, max(3, 2e6 // max(once, 1.0))))
        return time_us(fn, launches=k, warm=1 if k < args.launches else 5), k

    states0, spl0 = LT.ts_table_tuning(tc.TUNE_WAVE_MAX_STATES, -1), LT.ts_table_tuning(tc.TUNE_STATES_PER_LANE, -1)
    below0 = LT.ts_table_tuning(tc.TUNE_BLOCK_BELOW_BOARDS, -1)

    def policy(wave_max, spl, below):
        LT.ts_table_tuning(tc.TUNE_WAVE_MAX_STATES, wave_max)
        LT.ts_table_tuning(tc.TUNE_STATES_PER_LANE, spl)
        LT.ts_table_tuning(tc.TUNE_BLOCK_BELOW_BOARDS, below)

    def run(label, env, variants, steps=8):
        n = env.num_envs
        states = tc.table_states(env._dims)
        dist = torch.empty((n, states), dtype=torch.uint8, device=dev)
        build = lambda: tc.check(LT.ts_table_build(C.byref(env._dims), C.byref(env._state), tc.TABLE_MAX_DEPTH, dist.data_ptr(), stream()), "ts_table_build")
        say(f"{label}: {n} boards x {states} placements = {n * states / 2**20:.1f} MiB of table")
        base, default_us = None, None
        for name, wave_max, spl, below in variants:
            policy(wave_max, spl, below)
            d = tc.describe_table_build(env._dims)
            dist.fill_(77)
            build()
            torch.cuda.synchronize()
            if base is None:
                base = dist.clone()
            assert torch.equal(dist, base), "forms disagree"
            us, k = time_build(build)
            default_us = us if default_us is None else default_us
            say(f"    build, {name:<28} {d['name']:<17} lanes/board {d['lanes_per_board']:>3}  LDS/block {d['lds_bytes_block']:>6} B  blocks {d['blocks']:>7}  "
                f"{us:11.1f} us ({us * 1e3 / n:9.2f} ns/board, {k} launches)")
        policy(states0, spl0, below0)
        finite = base <= tc.TABLE_MAX_DEPTH
        deepest = torch.where(finite, base, torch.zeros_like(base)).amax(dim=1)
        say(f"    rounds per board (deepest finite entry + 1, 1 where nothing is won): mean {float((deepest.float() + 1).mean()):.2f}, most {int(deepest.max()) + 1}; "
            f"valid placements {int((base != tc.TABLE_INVALID).sum()) * 100 / base.numel():.1f} %")
        if steps is None:
            return
        for step in range(steps):
            env.step(torch.from_numpy(orc.fill_actions(n, seed=0x7AB1E, step_index=step)))
        moves, best, action = (torch.empty(n, dtype=dt, device=dev) for dt in (torch.int16, torch.uint8, torch.uint8))
        smoves, sbest, valid = torch.empty(n, dtype=torch.int16, device=dev), torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        look = lambda m, b, a: tc.check(LT.ts_table_lookup(C.byref(env._dims), C.byref(env._state), base.data_ptr(), n, None, m, b, a, stream()), "ts_table_lookup")
        solve = lambda: sc.check(LS.ts_solve(C.byref(env._dims), C.byref(env._state), sc.SOLVE_MAX_DEPTH, smoves.data_ptr(), sbest.data_ptr(), stream()), "ts_solve")
        look(moves.data_ptr(), best.data_ptr(), action.data_ptr())
        solve()
        torch.cuda.synchronize()
        assert torch.equal(moves, smoves) and torch.equal(best, sbest), "lookup and ts_solve disagree"
        t_pair = time_us(lambda: look(moves.data_ptr(), best.data_ptr(), None))
        t_act = time_us(lambda: look(None, None, action.data_ptr()))
        t_solve = time_us(solve)
        t_valid = time_us(lambda: _cabi.check(L.ts_valid_moves(C.byref(env._dims), C.byref(env._state), valid.data_ptr(), stream()), "ts_valid_moves"))
        say(f"    after {steps} random steps ({int((moves >= 1).sum())} boards with a way to win, {int((moves == 0).sum())} won): "
            f"ts_table_lookup moves+best {t_pair:8.1f} us, action only {t_act:8.1f} us; ts_solve {t_solve:9.1f} us ({sc.describe_solve(env._dims)['name']}); "
            f"ts_valid_moves {t_valid:7.1f} us")
        say(f"    lookup / ts_solve = {t_pair / t_solve:.4f}; lookup / ts_valid_moves = {t_pair / t_valid:.2f}; "
            f"break-even = build / (solve - lookup) = {default_us / (t_solve - t_pair):.1f} lookups")

    DEFAULT = ("library policy", states0, spl0, below0)
    WAVE = lambda spl: (f"wave form, {spl} placement{'s' if spl > 1 else ''}/lane", 65536, spl, 0)
    BLOCK = ("block form", 0, 1, 0)
    shrink = 4 if args.quick else 0
    shapes = [  # label, S, T, K, mc, boards, variants: the shapes and batch sizes of the solver's table
        ("4x4 / 2 tiles (cfg1, 256 states)", 4, 2, 2, False, 1 << 20, [DEFAULT, WAVE(1), WAVE(4), WAVE(8), WAVE(32), BLOCK]),
        ("5x5 / 2 tiles (625 states)", 5, 2, 3, False, 1 << 18, [DEFAULT, WAVE(1), WAVE(16), BLOCK]),
        ("6x6 / 2 tiles (1296 states)", 6, 2, 6, False, 1 << 17, [DEFAULT, WAVE(1), BLOCK]),
        ("7x7 / 2 tiles (2401 states)", 7, 2, 8, False, 1 << 17, [DEFAULT, WAVE(1), BLOCK]),
        ("4x4 / 3 tiles (4096 states)", 4, 3, 2, True, 1 << 17, [DEFAULT, WAVE(1), BLOCK]),
        ("8x8 / 2 tiles (4096 states)", 8, 2, 10, True, 1 << 17, [DEFAULT, WAVE(1), BLOCK]),
        ("3x3 / 4 tiles (6561 states)", 3, 4, 1, False, 1 << 17, [DEFAULT, WAVE(1), BLOCK]),
        ("5x5 / 3 tiles (15625 states)", 5, 3, 3, True, 1 << 18, [DEFAULT, WAVE(1), BLOCK]),
        ("6x6 / 3 tiles (46656 states)", 6, 3, 6, False, 1 << 14, [DEFAULT, WAVE(1), BLOCK]),
        ("4x4 / 4 tiles (65536 states)", 4, 4, 2, True, 1 << 13, [DEFAULT, WAVE(1), BLOCK]),
    ]
    for label, S, T, K, mc, n, variants in shapes:
        n >>= shrink
        env = VecTilerSliderEnv.from_seeds(np.arange(n, dtype=np.int64), size=S, num_tiles=T, num_obstacles=K, multi_color=mc, obs_dtype=None, device=dev,
                                           max_steps=1000)
        env.reset()
        run(label, env, variants[:1] if args.quick else variants)
        del env
        torch.cuda.empty_cache()
    if not args.quick:  # the batch size below which one wave per board no longer fills the GPU: both forms, small index spaces
        for label, S, T, K, mc in (("4x4 / 2 tiles (256 states)", 4, 2, 2, False), ("5x5 / 2 tiles (625 states)", 5, 2, 3, False)):
            for n in (1 << 10, 1 << 12, 1 << 14, 1 << 15, 1 << 16):
                env = VecTilerSliderEnv.from_seeds(np.arange(n, dtype=np.int64), size=S, num_tiles=T, num_obstacles=K, multi_color=mc, obs_dtype=None, device=dev)
                run(f"batch sweep, {label}", env, [WAVE(1), BLOCK], steps=None)
    for (S, T, mc), (ids, blk, init, tgt, want) in ref.fixture_groups(os.path.join(ROOT, "tests", "golden"), pack_levels).items():
        for copies in (1, 64):
            tile = lambda a: np.ascontiguousarray(np.tile(a, (1, copies)))
            env = VecTilerSliderEnv.from_arrays(S, tile(blk), tile(init), tile(tgt), multi_color=mc, obs_dtype=None, device=dev, max_steps=1000)
            env.reset()
            forms = [DEFAULT] if args.quick else [DEFAULT, WAVE(1), BLOCK]
            run(f"screenshot levels {S}x{S} / {T} tiles {'multi' if mc else 'single'}" + (f", {copies} copies of each" if copies > 1 else ""), env, forms,
                steps=4 if copies == 1 else None)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        open(args.log, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
