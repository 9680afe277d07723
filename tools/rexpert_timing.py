#!/usr/bin/env python3
"""Times the reach-table experts (include/tiler_slider_rexpert.h) against the loops they replace, on one GPU: HIP events around the
launches after warm-up.

    python tools/rexpert_timing.py [--log FILE] [--launches 5] [--quick]

Per shape - 5x5 / 4 tiles / 3 obstacles and 8x8 / 3 tiles / 10 obstacles, multi colour - and per batch of 4,096, 65,536 and
1,048,576 boards, K = 100 steps, epsilon = 0.1, an observation-less auto-reset environment (max_steps 30).  The levels are 1,024
reference levels whose targets lie where ten random moves leave the tiles - they can be won; fewer than 1 % of random 5x5 levels
can -; the reach table is built on those distinct levels (capacity 4,096) and read through rows=.

    fused        one ts_rexpert_rollout: K steps, state written back, the last flags, no other output
    loop         what it replaces, K times: ts_fill_actions, ts_rtable_lookup (action only), the epsilon mix - torch.rand, a
                 comparison and two torch.where -, ts_step; every call of it code of the tree as it stood before this library
    loop, graph  the same K rounds captured once into a graph and replayed
    labels       one ts_rexpert_labels over the K * N samples of a logged rollout: moves, best and action
    lookups      K times: a copy of the logged cells into the boards and ts_rtable_lookup (moves and best): lookup_bits() K times

The loop is timed twice, before and after the fused call; the larger relative spread of a pair of its runs at a point is the
margin within which "fused is not slower than the loop" is read.  The explore bits of the fused call are bits of the draw that
ts_fill_actions does not return, so the loop draws its own: before anything is timed the two sides are compared byte for byte
with epsilon = 0, and the labels with the lookups.  profiles/rexpert_timing.log is where a run of this script belongs (DESIGN.md
section 27); run it under `timeout`.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="16 steps, the two smaller batches")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import VecTilerSliderEnv, _cabi
    from tiler_slider_amd import _rexpert_cabi as ec
    from tiler_slider_amd import _rtable_cabi as xc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.log:  # rewritten at every line: what was measured survives a run that ends early
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            open(args.log, "w").write("\n".join(lines) + "\n")

    L, LE, LX = _cabi.lib(), ec.lib(), xc.lib()
    dev = torch.device("cuda", 0)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def time_us(fn, launches, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches

    SEED, LEVELS, EPS, MAX_STEPS = 0x7131, 1024, 0.1, 30
    steps = 16 if args.quick else 100

    def levels_of(S, T, Ko):
        """(blk, init, tgt) of LEVELS reference levels with the targets where ten random moves leave the tiles."""
        walk = VecTilerSliderEnv.from_seeds(np.arange(LEVELS, dtype=np.int64), size=S, num_tiles=T, num_obstacles=Ko, multi_color=True, obs_dtype=None, device=dev)
        walk.reset()
        walk.rollout(10, "random", seed=0x3A1C, stats=False)
        return walk._blk.clone(), walk._init.clone(), walk.positions.clone()

    def run(label, S, T, Ko, n, level):
        blk, init, tgt = level
        small = VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=True, obs_dtype=None, device=dev)
        small.reset()
        rt = small.build_reach_table(capacity=4096)
        rows = (torch.arange(n, device=dev) % LEVELS).to(torch.int32)
        idx = rows.long()
        make = lambda: VecTilerSliderEnv.from_arrays(S, blk[:, idx].contiguous(), init[:, idx].contiguous(), tgt[:, idx].contiguous(), multi_color=True,
                                                     obs_dtype=None, device=dev, max_steps=MAX_STEPS, auto_reset=True)
        env, twin = make(), make()
        env.reset(), twin.reset()
        can_win = int((rt.root_moves >= 1).sum())
        say(f"{label}: {n} boards, {LEVELS} levels ({can_win} can be won, {int(rt.full.sum())} FULL), table {rt.table.numel() * 8 / 2**20:.1f} MiB")
        act, expert, chosen = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(3))
        u = torch.empty(n, dtype=torch.float32, device=dev)
        table, count, slots = rt.table.data_ptr(), rt.count.data_ptr(), rt.slots

        def fused(e, eps, logs=None):
            cfg = ec.RexpertCfg(steps, _cabi.MODE_AUTORESET, 1, 0, SEED, 0, 0, int(round(eps * 2**32)), table, slots, count, LEVELS, rows.data_ptr())
            got = {"flags": e._flags, **(logs or {})}
            out = ec.RolloutOut(*(got[f].data_ptr() if f in got else None for f in ec.OUT_FIELDS))
            return lambda: ec.check(LE.ts_rexpert_rollout(C.byref(e._dims), C.byref(e._state), C.byref(cfg), C.byref(out), stream()), "ts_rexpert_rollout")

        def loop(e, eps):
            out = _cabi.StepOut(e._flags.data_ptr(), None, None, None, None, None, None)

            def body():
                for k in range(steps):
                    _cabi.check(L.ts_fill_actions(n, SEED, 0, k, act.data_ptr(), stream()), "ts_fill_actions")
                    xc.check(LX.ts_rtable_lookup(C.byref(e._dims), C.byref(e._state), table, slots, count, LEVELS, rows.data_ptr(), None, None,
                                                 expert.data_ptr(), stream()), "ts_rtable_lookup")
                    if eps > 0.0:
                        u.uniform_()
                        torch.where(u < eps, act, expert, out=chosen)
                        torch.where(chosen == 255, act, chosen, out=chosen)
                    else:
                        torch.where(expert == 255, act, expert, out=chosen)
                    _cabi.check(L.ts_step(C.byref(e._dims), C.byref(e._state), chosen.data_ptr(), e._mode, C.byref(out), stream()), "ts_step")
            return body

        # the same bytes first, without exploration: both from a fresh reset
        fused(env, 0.0)()
        loop(twin, 0.0)()
        torch.cuda.synchronize()
        for name in ("_pos", "_step_count", "_done", "_flags"):
            assert torch.equal(getattr(env, name), getattr(twin, name)), (label, n, name)
        env.reset(), twin.reset()
        body = loop(twin, EPS)
        t_loop_a = time_us(body, args.launches)
        t_fused = time_us(fused(env, EPS), args.launches)
        t_loop_b = time_us(body, args.launches)
        torch.cuda.synchronize()
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                body()
        t_graph_a = time_us(graph.replay, args.launches)
        t_fused_2 = time_us(fused(env, EPS), args.launches)
        t_graph_b = time_us(graph.replay, args.launches)
        del graph
        spread = max(abs(t_loop_a - t_loop_b) / min(t_loop_a, t_loop_b), abs(t_graph_a - t_graph_b) / min(t_graph_a, t_graph_b))
        t_f, best_loop = max(t_fused, t_fused_2), min(t_loop_a, t_loop_b, t_graph_a, t_graph_b)
        d = ec.describe_rexpert_rollout(env._dims, ec.RexpertCfg(steps, 1, 1, 0, 0, 0, 0, 0, None, slots, None, LEVELS, None))
        say(f"    K {steps:>3} {d['name']:<20} fused {t_fused:10.1f} / {t_fused_2:10.1f} us   loop {t_loop_a:10.1f} / {t_loop_b:10.1f} us   "
            f"loop, graph {t_graph_a:10.1f} / {t_graph_b:10.1f} us   spread {100 * spread:4.1f} %   fastest loop / slowest fused {best_loop / t_f:6.2f}   "
            f"{'not slower' if t_f <= best_loop * (1 + spread) else 'SLOWER'}   ({t_f * 1e3 / (n * steps):.3f} ns per board-step fused)")

        # ---- labels: a logged rollout of the expert, then one launch against K lookups on restored boards
        env.reset()
        logs = {"pos_log": torch.zeros((steps, T, n), dtype=torch.uint8, device=dev)}
        first = env.positions.clone()
        fused(env, EPS, logs)()
        pos_log = logs["pos_log"]
        moves, best, action = (torch.empty((steps, n), dtype=dt, device=dev) for dt in (torch.int16, torch.uint8, torch.uint8))
        moves2, best2 = torch.empty_like(moves), torch.empty_like(best)
        tin = ec.RexpertLabelsIn(first.data_ptr(), pos_log.data_ptr(), table, count, rows.data_ptr(), slots, LEVELS, steps, 0)
        tout = ec.LabelsOut(moves.data_ptr(), best.data_ptr(), action.data_ptr())

        def labels():
            ec.check(LE.ts_rexpert_labels(C.byref(env._dims), C.byref(env._state), C.byref(tin), C.byref(tout), stream()), "ts_rexpert_labels")

        def lookups():
            for k in range(steps):
                twin._pos.copy_(first if k == 0 else pos_log[k - 1])
                xc.check(LX.ts_rtable_lookup(C.byref(twin._dims), C.byref(twin._state), table, slots, count, LEVELS, rows.data_ptr(), moves2[k].data_ptr(),
                                             best2[k].data_ptr(), None, stream()), "ts_rtable_lookup")

        labels(), lookups()
        torch.cuda.synchronize()
        assert torch.equal(moves, moves2) and torch.equal(best, best2), (label, n, "labels")
        t_look_a = time_us(lookups, args.launches)
        t_lab = time_us(labels, args.launches)
        t_look_b = time_us(lookups, args.launches)
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                lookups()
        t_lgraph = time_us(graph.replay, args.launches)
        del graph
        spread = abs(t_look_a - t_look_b) / min(t_look_a, t_look_b)
        best_look = min(t_look_a, t_look_b, t_lgraph)
        dl = ec.describe_rexpert_labels(env._dims, steps)
        say(f"    K {steps:>3} {dl['name']:<20} labels {t_lab:9.1f} us ({dl['waves']} waves)   lookups {t_look_a:10.1f} / {t_look_b:10.1f} us   lookups, graph {t_lgraph:10.1f} us   "
            f"spread {100 * spread:4.1f} %   fastest lookups / labels {best_look / t_lab:6.2f}   {'not slower' if t_lab <= best_look * (1 + spread) else 'SLOWER'}   "
            f"({t_lab * 1e3 / (n * steps):.3f} ns per sample; expert has a move on {100 * float((action != 255).float().mean()):.0f} %)")
        del env, twin, small, rt, logs, pos_log, moves, best, action, moves2, best2
        torch.cuda.empty_cache()

    for label, S, T, Ko in (("5x5 / 4 tiles / 3 obstacles", 5, 4, 3), ("8x8 / 3 tiles / 10 obstacles", 8, 3, 10)):
        level = levels_of(S, T, Ko)
        for n in ((4096, 65536) if args.quick else (4096, 65536, 1 << 20)):
            run(label, S, T, Ko, n, level)


if __name__ == "__main__":
    main()
