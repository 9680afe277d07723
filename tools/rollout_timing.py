#!/usr/bin/env python3
"""Times the fused rollouts (include/tiler_slider_rollout.h) on one GPU: HIP events around 50 launches after warm-up.

    python tools/rollout_timing.py [--log FILE] [--launches 50] [--quick]

Per shape, K = 16 and 100 steps, the RANDOM and the TABLE policy (no exploration: the shipped entry points have no explore bits),
with and without the three per-step logs, in one process and one run, on an observation-less auto-reset actor:

    fused        one ts_rollout: state and last flags written once (+ act_log, flags_log, pos_log)
    fused+stats  the same with the five per-board reductions (the loop has no counterpart)
    loop         the shipped entry points producing the same bytes, K times: ts_fill_actions + ts_step for RANDOM; for TABLE
                 ts_fill_actions + ts_table_lookup + one torch.where (the no-expert fallback) + ts_step.  With logs the actions
                 and flags are written straight into their log rows and the cells copied there (one copy kernel per step).
    loop, graph  the same loop captured into one hipGraph and replayed

Before anything is timed the loop and the fused call are run from the same state and compared byte for byte.  The table holds
the distinct levels only (`levels` of them, boards replicate them through rows=), so that 5x5 / 3 tiles fits.
profiles/rollout_timing.log is a run of this script; run it under `timeout`.
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
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the boards, K = 16 only")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import VecTilerSliderEnv, _cabi
    from tiler_slider_amd import _rollout_cabi as rc
    from tiler_slider_amd import _table_cabi as tc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    L, LT, LR = _cabi.lib(), tc.lib(), rc.lib()
    dev = torch.device("cuda", 0)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def time_us(fn, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches

    SEED = 0x7131

    def make(S, T, K, mc, n, levels):
        env = VecTilerSliderEnv.from_seeds(np.arange(n, dtype=np.int64) % levels, size=S, num_tiles=T, num_obstacles=K, multi_color=mc, obs_dtype=None,
                                           device=dev, max_steps=20, auto_reset=True)
        env.reset()
        return env

    def run(label, S, T, K, mc, n, levels):
        env, twin = make(S, T, K, mc, n, levels), make(S, T, K, mc, n, levels)
        small = make(S, T, K, mc, levels, levels)
        table = small.build_table()
        rows = (torch.arange(n, device=dev) % levels).to(torch.int32)
        say(f"{label}: {n} boards, {levels} levels, table {table.dist.numel() / 2**20:.1f} MiB")
        act, expert, chosen = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(3))
        for steps in ((16,) if args.quick else (16, 100)):
            logs = {"act_log": torch.zeros((steps, n), dtype=torch.uint8, device=dev), "flags_log": torch.zeros((steps, n), dtype=torch.uint8, device=dev),
                    "pos_log": torch.zeros((steps, T, n), dtype=torch.uint8, device=dev)}
            twin_logs = {k: torch.zeros_like(v) for k, v in logs.items()}
            stats = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("wins", "finished", "first_win", "win_moves", "reward_sum")}
            for policy in (rc.RANDOM, rc.TABLE):
                cfg = rc.RolloutCfg(steps, _cabi.MODE_AUTORESET, policy, 1, None, SEED, 0, 0, 0, table.dist.data_ptr(), levels, rows.data_ptr())

                def fused(with_logs, with_stats=False):
                    got = {"flags": env._flags, **(logs if with_logs else {}), **(stats if with_stats else {})}
                    out = rc.RolloutOut(*(got[f].data_ptr() if f in got else None for f in rc.OUT_FIELDS))
                    return lambda: rc.check(LR.ts_rollout(C.byref(env._dims), C.byref(env._state), C.byref(cfg), C.byref(out), stream()), "ts_rollout")

                def loop(e, with_logs, lg):
                    outs = [_cabi.StepOut(lg["flags_log"][k].data_ptr() if with_logs else e._flags.data_ptr(), None, None, None, None, None, None) for k in range(steps)]
                    if with_logs:  # the last step's flags are also the environment's
                        outs[-1] = _cabi.StepOut(e._flags.data_ptr(), None, None, None, None, None, None)

                    def body():
                        for k in range(steps):
                            a = lg["act_log"][k] if with_logs else (chosen if policy == rc.TABLE else act)
                            draw = act if policy == rc.TABLE else a
                            _cabi.check(L.ts_fill_actions(n, SEED, 0, k, draw.data_ptr(), stream()), "ts_fill_actions")
                            if policy == rc.TABLE:
                                tc.check(LT.ts_table_lookup(C.byref(e._dims), C.byref(e._state), table.dist.data_ptr(), levels, rows.data_ptr(), None, None,
                                                            expert.data_ptr(), stream()), "ts_table_lookup")
                                torch.where(expert == 255, act, expert, out=a)
                            _cabi.check(L.ts_step(C.byref(e._dims), C.byref(e._state), a.data_ptr(), e._mode, C.byref(outs[k]), stream()), "ts_step")
                            if with_logs:
                                lg["pos_log"][k].copy_(e._pos)
                                if k == steps - 1:
                                    lg["flags_log"][k].copy_(e._flags)
                    return body

                for with_logs in (False, True):
                    # the same bytes first: both from a fresh reset
                    env.reset(), twin.reset()
                    fused(with_logs)()
                    loop(twin, with_logs, twin_logs)()
                    torch.cuda.synchronize()
                    for name in ("_pos", "_step_count", "_done", "_flags"):
                        assert torch.equal(getattr(env, name), getattr(twin, name)), (label, steps, policy, name)
                    if with_logs:
                        for name in logs:
                            assert torch.equal(logs[name], twin_logs[name]), (label, steps, policy, name)
                    t_fused = time_us(fused(with_logs))
                    t_stats = time_us(fused(with_logs, True))
                    body = loop(twin, with_logs, twin_logs)
                    t_loop = time_us(body)
                    torch.cuda.synchronize()
                    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
                    with torch.cuda.stream(side):
                        with torch.cuda.graph(graph, stream=side):
                            body()
                    t_graph = time_us(graph.replay)
                    d = rc.describe_rollout(env._dims, cfg, (rc.OUT_ACT_LOG | rc.OUT_FLAGS_LOG | rc.OUT_POS_LOG) if with_logs else 0)
                    say(f"    K {steps:>3} {'RANDOM' if policy == rc.RANDOM else 'TABLE ':<6} {'logs   ' if with_logs else 'no logs'} {d['name']:<16} "
                        f"fused {t_fused:9.1f} us  fused+stats {t_stats:9.1f} us  loop {t_loop:10.1f} us  loop, graph {t_graph:10.1f} us   "
                        f"loop / fused {t_loop / t_fused:6.2f}  graph / fused {t_graph / t_fused:6.2f}  ({t_fused * 1e3 / (n * steps):.3f} ns per board-step fused)")
                    del graph
        del env, twin, small, table
        torch.cuda.empty_cache()

    shrink = 4 if args.quick else 0
    for label, S, T, K, mc, n, levels in (("4x4 / 2 tiles (cfg1)", 4, 2, 2, False, 1 << 20, 1 << 16), ("4x4 / 2 tiles (cfg1), small batch", 4, 2, 2, False, 4096, 4096),
                                          ("5x5 / 3 tiles", 5, 3, 3, True, 1 << 18, 4096), ("8x8 / 2 tiles", 8, 2, 10, True, 1 << 17, 1 << 14)):
        n = max(n >> shrink, 4096)
        run(label, S, T, K, mc, n, min(levels, n))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        open(args.log, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
