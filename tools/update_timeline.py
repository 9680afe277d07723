#!/usr/bin/env python3
"""The timeline of one launch of the in-place step: when its waves start, when their loads have returned, when they begin to
store the observation and when they are through (csrc/ts_update.hip, -DTS_UPDATE_TRACE; profiles/update_requests.md, section 6).

    timeout 300 python tools/update_timeline.py [--log profiles/update_timeline.log] [--shape cfg1_1m] [--steps 60] [--resident 8192]
                                                [--define NAME[=VALUE] ...]

One process, tools/update_pmc_target.py's environment (update_ab.py's levels and action buffers, multi colour, auto-reset,
obs_update="inplace"): a reset and --steps steps with the shipped library, with the -DTS_UPDATE_TRACE=1 build and with the
-DTS_UPDATE_TRACE=2 build (built into build/variants/ through the guarded build on first use, as update_ab.py --define builds a
variant), the last 50 steps of each between two HIP events.  A traced build has every wave stamp the 100 MHz clock four times
and its lane 0 write the stamps into an array of the code object; ts_update_trace_read copies the last launch's out.  TRACE=2
waits for the wave's stores to be acknowledged before the last stamp: its store stall less TRACE=1's is that wait.

--define NAME[=VALUE] adds a knob to the two traced builds (build/variants/libtiler_slider_update_trace<level>_<names>.so):
TS_UPDATE_PRIO_OFF gives the timeline without the priority schedule (profiles/update_timeline_prio_off.log), TS_UPDATE_PRIO_ALL
the timeline with it for a shape whose kernel does not ship it.

Waves are ranked by their entry stamp and cut into rounds of --resident (256 CUs x 4 SIMDs x 8 waves of 28 registers).  Per
round the median, the 10th and 90th percentile and the maximum of load wait, compute and store stall, then their means and the
mean residency (entry to end); then per us the waves that enter, begin to store and end in it, and the waves resident - in a
slot - at its start.  All times are us from the first wave's entry; a stamp is 10 ns, so medians of a few ticks are coarse.
Run it under `timeout`."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

TICK_US = 0.01  # wall_clock64(): 100 MHz
TRACE_WAVES = 16384  # kTraceWaves of csrc/ts_update.hip


def spread(xs):
    """median [10th .. 90th percentile] max, us"""
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(f * len(xs)))] * TICK_US  # noqa: E731
    return f"{statistics.median(xs) * TICK_US:6.2f} [{q(0.1):5.2f} .. {q(0.9):5.2f}] {xs[-1] * TICK_US:6.2f}"


def mean_us(xs):
    return statistics.fmean(xs) * TICK_US


def resident_at(rows, t0, n_bins):
    """Waves resident at t0 + b us, b = 0 .. n_bins - 1: entered at or before that tick and not yet ended."""
    ticks_per_us = round(1 / TICK_US)
    return [sum(1 for r in rows if r[0] <= t0 + b * ticks_per_us < r[3]) for b in range(n_bins)]


def report(say, rows, resident, us_step):
    """rows: (entry, loaded, store, end, xcc) per recorded wave, in ticks."""
    rows.sort()
    t0 = rows[0][0]
    end = max(r[3] for r in rows)
    first_end = min(r[3] for r in rows)
    say(f"  {len(rows)} waves; entered before the first wave ended: {sum(1 for r in rows if r[0] < first_end)}")
    say("  round  waves  entry, first .. last   load wait: median [p10 .. p90] max   compute                            store stall")
    for k in range(0, len(rows), resident):
        part = rows[k:k + resident]
        say(f"  {k // resident:>5} {len(part):>6}  {(part[0][0] - t0) * TICK_US:6.2f} .. {(part[-1][0] - t0) * TICK_US:6.2f}      "
            f"{spread([r[1] - r[0] for r in part])}   {spread([r[2] - r[1] for r in part])}   {spread([r[3] - r[2] for r in part])}")
    say("  round  mean: load wait  compute  store stall  residency (entry to end)")
    for k in range(0, len(rows), resident):
        part = rows[k:k + resident]
        say(f"  {k // resident:>5}        {mean_us([r[1] - r[0] for r in part]):9.2f} {mean_us([r[2] - r[1] for r in part]):8.2f} "
            f"{mean_us([r[3] - r[2] for r in part]):12.2f} {mean_us([r[3] - r[0] for r in part]):10.2f}")
    say(f"  mean residency of all waves, entry to end: {mean_us([r[3] - r[0] for r in rows]):.2f} us")
    say(f"  observation stores issue from {(min(r[2] for r in rows) - t0) * TICK_US:.2f} to {(max(r[2] for r in rows) - t0) * TICK_US:.2f} us; "
        f"waves end from {(first_end - t0) * TICK_US:.2f} to {(end - t0) * TICK_US:.2f} us")
    span = (end - t0) * TICK_US
    say(f"  first entry to last end {span:.2f} us; {us_step:.2f} us per step by HIP events; the rest, launch boundary and flush tail: {us_step - span:.2f} us")
    say("  us      " + " ".join(f"{b:>5}" for b in range(0, int(span) + 1)))
    for name, col in (("entries", 0), ("stores ", 2), ("ends   ", 3)):
        hist = [0] * (int(span) + 1)
        for r in rows:
            hist[min(len(hist) - 1, int((r[col] - t0) * TICK_US))] += 1
        say(f"  {name} " + " ".join(f"{h:>5}" for h in hist))
    say("  resident" + " ".join(f"{h:>5}" for h in resident_at(rows, t0, int(span) + 1)) + "   (waves in a slot at the start of each us)")
    by_xcc = {}
    for r in rows:
        by_xcc.setdefault(r[4], []).append(r)
    say("  XCC: waves, last end  " + "  ".join(f"{x}: {len(v)}, {(max(r[3] for r in v) - t0) * TICK_US:.2f}" for x, v in sorted(by_xcc.items())))


def main():
    import update_ab
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "update_timeline.log"))
    ap.add_argument("--shape", default="cfg1_1m", choices=sorted(update_ab.SHAPES))
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--resident", type=int, default=8192)
    ap.add_argument("--define", action="append", default=[], metavar="NAME[=VALUE]",
                    help="-D knob of csrc/ts_update.hip for the two traced builds (TS_UPDATE_PRIO_OFF: the timeline without the priority schedule); repeatable")
    args = ap.parse_args()
    if args.steps < 51:
        ap.error("--steps: at least 51 (the last 50 are timed)")
    import torch
    from tiler_slider_amd import VecTilerSliderEnv, _cabi, _update_cabi as uc

    shipped = uc.LIB_PATH
    libraries = [("shipped", shipped)]
    tag = "".join("_" + d.replace("TS_UPDATE_", "").replace("=", "").lower() for d in args.define)
    for level in (1, 2):
        variant = os.path.join(ROOT, "build", "variants", f"libtiler_slider_update_trace{level}{tag}.so")
        if not os.path.exists(variant) or os.path.getmtime(variant) < os.path.getmtime(uc.SRC):
            _cabi.compile_guarded(uc.SRC, variant, defines=(f"-DTS_UPDATE_TRACE={level}", *("-D" + d for d in args.define)),
                                  work=os.path.dirname(variant), min_kernels=uc.MIN_KERNELS)
        libraries.append((" ".join([f"TS_UPDATE_TRACE={level}", *args.define]), variant))

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        open(args.log, "w").write("\n".join(lines) + "\n")

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    S, T, K, n = update_ab.SHAPES[args.shape]
    stream = torch.cuda.current_stream(dev).cuda_stream
    ring = []
    for i in range(16):
        a = torch.empty(n, dtype=torch.uint8, device=dev)
        _cabi.check(_cabi.lib().ts_fill_actions(n, update_ab.ACTION_SEED, 0, i, a.data_ptr(), stream), "ts_fill_actions")
        ring.append(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    say(f"# tools/update_timeline.py --shape {args.shape} --steps {args.steps} --resident {args.resident}: {n} boards, "
        f"{-(-n // 64)} waves; {torch.cuda.get_device_name(dev)}")
    us = {}
    for name, path in libraries:
        uc.LIB_PATH, uc._lib = path, None  # a fresh environment binds the library named here
        env = VecTilerSliderEnv.random(n, size=S, num_tiles=T, num_obstacles=K, seed=update_ab.LEVEL_SEED, multi_color=True,
                                       max_steps=2**30, device=dev, auto_reset=True, obs_update="inplace")
        env.reset()
        for i in range(args.steps - 50):
            env.step_async(ring[i & 15])
        e0.record()
        for i in range(args.steps - 50, args.steps):
            env.step_async(ring[i & 15])
        e1.record()
        torch.cuda.synchronize(dev)
        us[name] = e0.elapsed_time(e1) * 1e3 / 50
        kernel = _cabi.describe_launch(env._dims, _cabi.OP_STEP, _cabi.OUT_OBS)["name"]
        say(f"{name}: {os.path.relpath(path, ROOT)}, {kernel}, {us[name]:.2f} us per step"
            + ("" if name == "shipped" else f" ({us[name] - us['shipped']:+.2f} us, {100 * (us[name] / us['shipped'] - 1):+.1f} %: the trace's own cost)"))
        if name != "shipped":
            L = uc.lib()
            L.ts_update_trace_read.argtypes, L.ts_update_trace_read.restype = [C.c_void_p, C.c_int64], C.c_int64
            words = 4 * min(TRACE_WAVES, -(-n // 64))
            buf = (C.c_uint64 * words)()
            got = L.ts_update_trace_read(buf, words)
            if got != words:
                raise SystemExit(f"ts_update_trace_read: {got}")
            rows = [(buf[i] & (1 << 56) - 1, buf[i + 1], buf[i + 2], buf[i + 3] & (1 << 56) - 1, buf[i + 3] >> 56) for i in range(0, words, 4)]
            rows = [r for r in rows if r[0]]
            report(say, rows, args.resident, us[name])
        del env
        torch.cuda.empty_cache()
    uc.LIB_PATH, uc._lib = shipped, None


if __name__ == "__main__":
    main()
