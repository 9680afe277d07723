#!/usr/bin/env python3
"""Times the in-place step (include/tiler_slider_update.h) against the full-write step on one GPU: where is
VecTilerSliderEnv(obs_update="auto") allowed to step in place?

    python tools/update_ab.py [--log FILE] [--rounds 3] [--store plain|sc1|lane] [--define NAME[=VALUE] ...] [--library FILE]
                              [--max-steps M] [--obs-dtype float32|uint8] [--only cfg1_1m]

Per shape two environments on the same levels (bench.py's LEVEL_SEED, multi colour, auto-reset, max_steps 2**30) and the same
sixteen action buffers (ACTION_SEED): obs_update="inplace" (ts_step_update whatever the size of the buffer) and obs_update="full"
(ts_step).  Each is timed with HIP events on the launch stream over 200 steps after a reset and 50 warm-up steps, --rounds times,
the two taking turns; the line gives every round, the medians and their ratio, and what "auto" chooses for the shape.  Before a
shape is timed the two environments are compared after 20 steps (observation, flags, cells): nothing is timed that computes
something else.

--store sc1 loads a build of the library whose scattered observation stores are agent-scope stores in every kernel
(-DTS_UPDATE_STORE_SC1, built into build/variants/ through the guarded build on first use) - the shipped build has them in the
two two-tile kernels whose board is 192 bytes of observation and plain stores in the others, and --define TS_UPDATE_STORE_PLAIN
builds plain stores everywhere; --store lane a build whose two-tile kernels store every board's cells from the board's own lane
(-DTS_UPDATE_LANE_PUT, plain stores) instead of from the four lanes of its quad.
--define NAME[=VALUE] (repeatable) does the same for any other build-time knob of csrc/ts_update.hip - the ablations of
profiles/update_requests.md are -DTS_UPDATE_NO_PUT (the observation stores compiled out) and -DTS_UPDATE_ARITH_TWICE (the slides
computed twice), the write-back variants of its section 6 -DTS_UPDATE_SC1_FIRST=K, -DTS_UPDATE_SC1_LAST=K, -DTS_UPDATE_NT,
-DTS_UPDATE_KICK=K and -DTS_UPDATE_STATE_ALWAYS, the priority schedule of its section 7 -DTS_UPDATE_PRIO_OFF (in no kernel: the
parent's code), -DTS_UPDATE_PRIO_ALL (in all 32; the shipped build has it in seven), -DTS_UPDATE_PRIO_LEVEL=1|2|3,
-DTS_UPDATE_PRIO_UNTIL=issued|loaded|store and the control -DTS_UPDATE_PRIO_STORES - into build/variants/libtiler_slider_update_<names>.so; --library FILE steps
with a build of the library made elsewhere (the parent commit's, say).  --max-steps 7 times episodes that end every seventh
step, so that most waves reset; --obs-dtype uint8 times both environments with the uint8 observation.
profiles/update_ab.log is where a run of this script belongs; run it under `timeout`.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVEL_SEED = 0x715311DE
ACTION_SEED = 0xAC710005
# name: (size, tiles, obstacles, boards)
SHAPES = {
    "cfg1_4k": (4, 2, 2, 4096),
    "cfg1_64k": (4, 2, 2, 65536),
    "cfg1_128k": (4, 2, 2, 1 << 17),
    "cfg1_256k": (4, 2, 2, 1 << 18),
    "cfg1_512k": (4, 2, 2, 1 << 19),
    "cfg1_768k": (4, 2, 2, 3 << 18),
    "cfg1_1m": (4, 2, 2, 1 << 20),
    "cfg1_4m": (4, 2, 2, 4 << 20),
    "cfg1_16m": (4, 2, 2, 16 << 20),
    "8x8_4_512k": (8, 4, 6, 524288),
    "8x8_2_512k": (8, 2, 6, 524288),
    "5x5_2_1m": (5, 2, 3, 1 << 20),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--store", choices=("plain", "sc1", "lane"), default="plain")
    ap.add_argument("--define", action="append", default=[], metavar="NAME[=VALUE]", help="-D knob of csrc/ts_update.hip; repeatable")
    ap.add_argument("--library", default=None, help="a build of libtiler_slider_update.so to step with instead of the shipped one")
    ap.add_argument("--max-steps", type=int, default=2**30)
    ap.add_argument("--obs-dtype", choices=("float32", "uint8"), default="float32")
    ap.add_argument("--check", choices=("all", "state"), default=None,
                    help="what the two environments must agree on before a shape is timed; state: flags and cells only, the default "
                         "with -DTS_UPDATE_NO_PUT, whose build leaves the observation alone")
    ap.add_argument("--only", default=None, help="comma-separated names of SHAPES")
    ap.add_argument("--clock-warmup-ms", type=float, default=300.0)
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import VecTilerSliderEnv, _cabi, _update_cabi

    store_define = {"sc1": "TS_UPDATE_STORE_SC1=1", "lane": "TS_UPDATE_LANE_PUT=1"}
    defines = ([store_define[args.store]] if args.store in store_define else []) + args.define
    if args.library and defines:
        ap.error("--library takes a finished build: no --store sc1 or --define with it")
    if args.library:
        _update_cabi.LIB_PATH = os.path.abspath(args.library)
    elif defines:
        tag = args.store if defines == [store_define.get(args.store)] else "_".join(d.replace("TS_UPDATE_", "").replace("=", "").lower() for d in defines)
        variant = os.path.join(ROOT, "build", "variants", f"libtiler_slider_update_{tag}.so")
        if not os.path.exists(variant) or os.path.getmtime(variant) < os.path.getmtime(_update_cabi.SRC):
            _cabi.compile_guarded(_update_cabi.SRC, variant, defines=tuple("-D" + d for d in defines), work=os.path.dirname(variant),
                                  min_kernels=_update_cabi.MIN_KERNELS)
        _update_cabi.LIB_PATH = variant  # before the first lib(): this process steps with the variant

    check = args.check or ("state" if any("NO_PUT" in d for d in defines) else "all")

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.log:  # rewritten at every line: what was measured survives a run that ends early
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            open(args.log, "w").write("\n".join(lines) + "\n")

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = _cabi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    say(f"# tools/update_ab.py --store {args.store}{''.join(' --define ' + d for d in args.define)}"
        f"{' --max-steps %d' % args.max_steps if args.max_steps != 2**30 else ''}{' --obs-dtype uint8' if args.obs_dtype == 'uint8' else ''}: {args.steps} timed steps after {args.warmup} warm-up steps, HIP events, us per step; "
        f"{torch.cuda.get_device_name(dev)}")
    say(f"# library: {os.path.relpath(_update_cabi.LIB_PATH, ROOT)}")
    say("# shape            boards  obs MiB  kernel (in place)              in place, rounds        full, rounds            in place  full    full / in place  auto")

    def timed(env, ring):
        for i in range(args.warmup):
            env.step_async(ring[i & 15])
        e0.record()
        for i in range(args.steps):
            env.step_async(ring[i & 15])
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3 / args.steps

    names = args.only.split(",") if args.only else list(SHAPES)
    for name in names:
        S, T, K, n = SHAPES[name]
        kw = dict(size=S, num_tiles=T, num_obstacles=K, seed=LEVEL_SEED, multi_color=True, max_steps=args.max_steps, device=dev, auto_reset=True,
                  obs_dtype=args.obs_dtype)
        inplace = VecTilerSliderEnv.random(n, obs_update="inplace", **kw)
        full = VecTilerSliderEnv.random(n, obs_update="full", **kw)
        auto_says = "in place" if VecTilerSliderEnv.in_place_pays(inplace._obs.numel() * inplace._obs.element_size(), n, T) else "full"
        ring = []
        for i in range(16):
            a = torch.empty(n, dtype=torch.uint8, device=dev)
            _cabi.check(L.ts_fill_actions(n, ACTION_SEED, 0, i, a.data_ptr(), stream), "ts_fill_actions")
            ring.append(a)
        inplace.reset(), full.reset()
        for i in range(20):
            inplace.step_async(ring[i & 15]), full.step_async(ring[i & 15])
        same = ((check == "state" or torch.equal(inplace._obs, full._obs)) and torch.equal(inplace._flags, full._flags)
                and torch.equal(inplace.positions, full.positions))
        if not same:
            say(f"{name}: the two environments DIFFER after 20 steps - not timed")
            continue
        t_w = time.perf_counter()  # clocks up before the first round
        while (time.perf_counter() - t_w) * 1e3 < args.clock_warmup_ms:
            for i in range(64):
                full.step_async(ring[i & 15])
            torch.cuda.synchronize(dev)
        us_in, us_full = [], []
        for _ in range(args.rounds):
            inplace.reset(), full.reset()
            us_in.append(timed(inplace, ring))
            us_full.append(timed(full, ring))
        m_in, m_full = statistics.median(us_in), statistics.median(us_full)
        kernel = _cabi.describe_launch(inplace._dims, _cabi.OP_STEP, _cabi.OUT_OBS_U8 if args.obs_dtype == "uint8" else _cabi.OUT_OBS)["name"]
        say(f"{name:<16} {n:>9} {inplace._obs.numel() * inplace._obs.element_size() / 2**20:>8.1f}  {kernel:<29}  {' '.join(f'{u:7.2f}' for u in us_in):<23} "
            f"{' '.join(f'{u:7.2f}' for u in us_full):<23} {m_in:7.2f} {m_full:7.2f}  {m_full / m_in:8.2f}x         {auto_says}")
        del inplace, full, ring
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
