#!/usr/bin/env python3
"""Times the reach-table curricula (include/tiler_slider_rstarts.h) against the torch compositions they replace, on one GPU: HIP
events around the launches after warm-up.

    python tools/rstarts_timing.py [--log FILE] [--launches 5] [--quick]

Per shape - 5x5 / 4 tiles / 3 obstacles and 8x8 / 3 tiles / 10 obstacles, multi colour - 16,384 reference levels whose targets
lie where ten random moves leave the tiles (they can be won; fewer than 1 % of random levels of these shapes can), a reach table
at capacity 4,096 (1 GiB).

    index        one ts_rstarts_index over the 16,384 levels
    torch index  what the tree offered before this library: torch.sort(rt.table, dim=1), a slice of the first `capacity` words,
                 the entry bytes and torch.searchsorted for the 256 lower bounds
    place        one ts_rstarts_place of 4,096 and of 1,048,576 boards through rows=, band [1, 4], and the re-encode of the
                 float32 observation that place_at_distance() makes
    torch place  the same by gathers: the two bounds, the draw (torch.rand: the stream's draw is not offered to torch), the word,
                 the cells by division, torch.where writes of pos, init, step_count and done, and the same re-encode

Each composition is timed twice, before and after the fused call; the larger relative spread of its two runs is the margin
within which "the fused call is not slower" is read.  Before anything is timed the two sides are compared byte for byte: the
index as it is, the placement with the composition fed the fused call's own j.  profiles/rstarts_timing.log is where a run of
this script belongs; run it under `timeout`.
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
    ap.add_argument("--quick", action="store_true", help="2,048 levels")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import VecTilerSliderEnv
    from tiler_slider_amd import _rstarts_cabi as xs

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.log:  # rewritten at every line: what was measured survives a run that ends early
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            open(args.log, "w").write("\n".join(lines) + "\n")

    LX = xs.lib()
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

    LEVELS, CAPACITY, LO, HI = (2048 if args.quick else 16384), 4096, 1, 4
    KEY_MASK = (1 << 48) - 1

    def run(label, S, T, Ko):
        walk = VecTilerSliderEnv.from_seeds(np.arange(LEVELS, dtype=np.int64), size=S, num_tiles=T, num_obstacles=Ko, multi_color=True, obs_dtype=None, device=dev)
        walk.reset()
        walk.rollout(10, "random", seed=0x3A1C, stats=False)
        blk, init, tgt = walk._blk.clone(), walk._init.clone(), walk.positions.clone()
        small = VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=True, obs_dtype=None, device=dev)
        small.reset()
        rt = small.build_reach_table(capacity=CAPACITY)
        ridx = small.build_reach_index(rt)
        d = xs.describe_rstarts_index(LEVELS, rt.slots, CAPACITY)
        say(f"{label}: {LEVELS} levels ({int((rt.root_moves >= 1).sum())} can be won, {int(rt.full.sum())} FULL, {int(rt.count.clamp(min=0).sum())} states, "
            f"largest {int(rt.count.max())}), table {rt.table.numel() * 8 / 2**20:.0f} MiB, index {(ridx.sorted.numel() * 8 + ridx.first.numel() * 4) / 2**20:.0f} MiB")

        # ---- the index
        def fused_index():
            xs.check(LX.ts_rstarts_index(rt.table.data_ptr(), rt.slots, rt.count.data_ptr(), LEVELS, CAPACITY, ridx.sorted.data_ptr(), ridx.first.data_ptr(),
                                         stream()), "ts_rstarts_index")

        edges = torch.arange(256, device=dev).repeat(LEVELS, 1)
        held = {}

        def torch_index():
            srt = torch.sort(rt.table, dim=1).values[:, :CAPACITY]      # occupied words are negative: first, in their unsigned order
            srt = torch.where(srt < 0, srt, torch.zeros_like(srt))
            entry = torch.where(srt < 0, (srt >> 48) & 0xFF, torch.full_like(srt, 256))
            held["sorted"], held["first"] = srt, torch.searchsorted(entry, edges).to(torch.int32)

        fused_index(), torch_index()
        torch.cuda.synchronize()
        live = (rt.count >= 0).unsqueeze(1)
        assert torch.equal(ridx.sorted, torch.where(live, held["sorted"], torch.zeros_like(held["sorted"]))), (label, "sorted")
        assert torch.equal(ridx.first, torch.where(live, held["first"], torch.zeros_like(held["first"]))), (label, "first")
        t_a = time_us(torch_index, max(1, args.launches // 2), warm=1)
        t_f1 = time_us(fused_index, args.launches)
        t_b = time_us(torch_index, max(1, args.launches // 2), warm=1)
        t_f2 = time_us(fused_index, args.launches)
        held.clear()
        spread = abs(t_a - t_b) / min(t_a, t_b)
        t_f, best = max(t_f1, t_f2), min(t_a, t_b)
        say(f"    {d['name']:<24} index {t_f1:10.1f} / {t_f2:10.1f} us   torch.sort + searchsorted {t_a:10.1f} / {t_b:10.1f} us   spread {100 * spread:4.1f} %   "
            f"fastest torch / slowest fused {best / t_f:6.2f}   {'not slower' if t_f <= best * (1 + spread) else 'SLOWER'}   ({t_f * 1e3 / LEVELS:.1f} ns a level)")

        # ---- the placement
        for n in (4096, 1 << 20):
            rows = (torch.arange(n, device=dev) % LEVELS).to(torch.int32)
            idx = rows.long()
            make = lambda: VecTilerSliderEnv.from_arrays(S, blk[:, idx].contiguous(), init[:, idx].contiguous(), tgt[:, idx].contiguous(), multi_color=True,
                                                         obs_dtype="float32", device=dev)
            env, twin = make(), make()
            env.reset(), twin.reset()
            count, dist, deepest = (torch.empty(n, dtype=dt, device=dev) for dt in (torch.int32, torch.uint8, torch.uint8))
            cfg = xs.StartsCfg(LO, HI, None, xs.ALL, 1, 1, 0, 7, 0, 0)
            out = xs.StartsOut(count.data_ptr(), dist.data_ptr(), deepest.data_ptr())

            def fused_place():
                xs.check(LX.ts_rstarts_place(C.byref(env._dims), C.byref(env._state), ridx.sorted.data_ptr(), ridx.first.data_ptr(), CAPACITY, LEVELS,
                                             rows.data_ptr(), C.byref(cfg), C.byref(out), stream()), "ts_rstarts_place")
                env.encode(out=env._obs)

            weights = torch.tensor([(S * S) ** t for t in range(T)], dtype=torch.int64, device=dev).unsqueeze(1)
            got = {}

            def torch_place(j=None):
                a, b = ridx.first[idx, LO].long(), ridx.first[idx, HI + 1].long()
                c = (b - a).clamp_(min=0)
                finite = ridx.first[idx, 253].long()
                deep = torch.where(finite > 0, (ridx.sorted[idx, (finite - 1).clamp_(min=0)] >> 48) & 0xFF, torch.full_like(finite, 255)).to(torch.uint8)
                if j is None:
                    j = torch.minimum((torch.rand(n, device=dev, dtype=torch.float64) * c).long(), (c - 1).clamp_(min=0))
                placed = c > 0
                w = ridx.sorted[idx, torch.where(placed, a + j, torch.zeros_like(a))]
                cells = (((w & KEY_MASK).unsqueeze(0) // weights) % (S * S)).to(torch.uint8)
                twin._pos.copy_(torch.where(placed.unsqueeze(0), cells, twin._pos))
                twin._init.copy_(torch.where(placed.unsqueeze(0), cells, twin._init))
                twin._step_count.copy_(torch.where(placed, torch.zeros_like(twin._step_count), twin._step_count))
                twin._done.copy_(torch.where(placed, torch.zeros_like(twin._done), twin._done))
                got["count"], got["deepest"] = c.to(torch.int32), deep
                got["dist"] = torch.where(placed, (w >> 48) & 0xFF, torch.full_like(w, 255)).to(torch.uint8)
                twin.encode(out=twin._obs)

            # the same bytes first: the composition fed the j the fused call drew (recovered from where it put the boards)
            fused_place()
            if n <= 4096:
                a = ridx.first[idx, LO].long()
                keys = (env._pos.long() * weights).sum(0)
                words = ridx.sorted[idx]
                j = (((words & KEY_MASK) == keys.unsqueeze(1)) & (words < 0)).long().argmax(1) - a
                del words
                torch_place(torch.where(count > 0, j, torch.zeros_like(j)))
                torch.cuda.synchronize()
                for name in ("_pos", "_init", "_step_count", "_done", "_obs"):
                    assert torch.equal(getattr(env, name), getattr(twin, name)), (label, n, name)
                assert torch.equal(count, got["count"]) and torch.equal(dist, got["dist"]) and torch.equal(deepest, got["deepest"]), (label, n, "outputs")
            t_a = time_us(torch_place, args.launches)
            t_f1 = time_us(fused_place, args.launches)
            t_b = time_us(torch_place, args.launches)
            t_f2 = time_us(fused_place, args.launches)
            spread = abs(t_a - t_b) / min(t_a, t_b)
            t_f, best = max(t_f1, t_f2), min(t_a, t_b)
            name = xs.describe_rstarts_place(env._dims)["name"]
            say(f"    {name:<24} {n:>8} boards   place + encode {t_f1:9.1f} / {t_f2:9.1f} us   torch gathers + encode {t_a:9.1f} / {t_b:9.1f} us   spread {100 * spread:4.1f} %   "
                f"fastest torch / slowest fused {best / t_f:6.2f}   {'not slower' if t_f <= best * (1 + spread) else 'SLOWER'}   ({int((count > 0).sum())} placed)")
            del env, twin
            torch.cuda.empty_cache()
        del rt, ridx, small, walk
        torch.cuda.empty_cache()

    for label, S, T, Ko in (("5x5 / 4 tiles / 3 obstacles", 5, 4, 3), ("8x8 / 3 tiles / 10 obstacles", 8, 3, 10)):
        run(label, S, T, Ko)


if __name__ == "__main__":
    main()
