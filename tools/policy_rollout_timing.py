#!/usr/bin/env python3
"""Times the neural-policy rollouts (include/tiler_slider_policy.h) on one GPU: HIP events around 50 launches after warm-up.

    python tools/policy_rollout_timing.py [--log FILE] [--launches 50] [--quick]

Per shape, H = 16 and 64 hidden units, K = 16 and 100 steps, both selects, in one process and one run, on an observation-less
auto-reset actor with Gaussian weights:

    fused        one ts_policy_rollout: state and last flags written once, no logs
    eager        the loop a user writes without it, K times: env.encode_onehot() + two torch matmuls (addmm, relu, addmm) +
                 argmax / softmax + multinomial + env.step()
    eager, graph the same loop captured into one graph and replayed, where capture works ("-" where it does not)
    random       ts_rollout's RANDOM policy at the same K: fused / random is what the network costs

Before a row is timed the two sides are compared, teacher-forced in the manner of tests/test_gpu_policy.py but more loosely (the
tests hold the rigorous bound and the sampling rule; this is a sanity check of what is about to be timed): the fused call runs with
its logs, a twin is stepped with the logged actions, and at every step torch's float32 logits on the twin's own one-hot planes
must agree with the logged logits to 1e-4 of their scale; a greedy action must be the first argmax of the logged logits, a
sampled one only be an action.  profiles/policy_rollout_timing.log is two runs of this script; run it under `timeout`.
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
    from tiler_slider_amd import MlpPolicy, VecTilerSliderEnv, _cabi
    from tiler_slider_amd import _policy_cabi as pc
    from tiler_slider_amd import _rollout_cabi as rc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    LP, LR = pc.lib(), rc.lib()
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
        D = env.onehot_channels * S * S
        planes = torch.empty((n, env.onehot_channels, S, S), dtype=torch.float32, device=dev)
        say(f"{label}: {n} boards, {D} features")
        for H in (16, 64):
            gen = torch.Generator(device="cpu").manual_seed(H)
            w1, b1, w2, b2 = (torch.randn(s, generator=gen).to(dev) for s in ((H, D), (H,), (4, H), (4,)))
            policy = MlpPolicy(w1, b1, w2, b2)
            mlp = policy._mlp(env)
            w1t, w2t = w1.t().contiguous(), w2.t().contiguous()

            def logits_of(e):
                x = e.encode_onehot(out=planes).flatten(1)
                return torch.addmm(b2, torch.relu(torch.addmm(b1, x, w1t)), w2t)

            for steps in ((16,) if args.quick else (16, 100)):
                for select in ("greedy", "sample"):
                    # a sanity check of the two sides: a twin teacher-forced with the logged actions
                    env.reset(), twin.reset()
                    got = env.rollout_policy(steps, policy, select=select, seed=SEED, log=("act", "logits"))
                    for k in range(steps):
                        z = logits_of(twin)
                        scale = float(z.abs().max())
                        assert float((z - got.logits_log[k]).abs().max()) <= 1e-4 * max(1.0, scale), (label, H, steps, select, k)
                        if select == "greedy":
                            first = (got.logits_log[k] == got.logits_log[k].max(dim=1, keepdim=True).values).to(torch.uint8).argmax(dim=1)
                            assert torch.equal(first.to(torch.uint8), got.act_log[k]), (label, H, steps, select, k)
                        assert int(got.act_log[k].max()) <= 3
                        twin.step(got.act_log[k])
                    for name in ("_pos", "_step_count", "_done", "_flags"):
                        assert torch.equal(getattr(env, name), getattr(twin, name)), (label, H, steps, select, name)
                    cfg = pc.PolicyCfg(steps, _cabi.MODE_AUTORESET, pc.SELECTS[select], 1, SEED, 0, 0, 0)
                    out = pc.PolicyOut(*(env._flags.data_ptr() if f == "flags" else None for f in pc.OUT_FIELDS))

                    def fused(lib):
                        return lambda: pc.check(lib.ts_policy_rollout(C.byref(env._dims), C.byref(env._state), C.byref(mlp), C.byref(cfg), C.byref(out),
                                                                      stream()), "ts_policy_rollout")

                    def eager():
                        for _ in range(steps):
                            z = logits_of(twin)
                            a = z.argmax(dim=1) if select == "greedy" else torch.multinomial(torch.softmax(z, dim=1), 1).squeeze(1)
                            twin.step(a.to(torch.uint8))

                    rcfg = rc.RolloutCfg(steps, _cabi.MODE_AUTORESET, rc.RANDOM, 1, None, SEED, 0, 0, 0, None, 0, None)
                    rout = rc.RolloutOut(*(env._flags.data_ptr() if f == "flags" else None for f in rc.OUT_FIELDS))
                    random = lambda: rc.check(LR.ts_rollout(C.byref(env._dims), C.byref(env._state), C.byref(rcfg), C.byref(rout), stream()), "ts_rollout")
                    t_fused, t_random, t_eager = time_us(fused(LP)), time_us(random), time_us(eager)
                    torch.cuda.synchronize()
                    t_graph = None
                    try:
                        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
                        with torch.cuda.stream(side):
                            with torch.cuda.graph(graph, stream=side):
                                eager()
                        t_graph = time_us(graph.replay)
                        del graph
                    except Exception as e:  # capture is not promised for this loop: report, do not work around
                        say(f"        (graph capture of the eager loop failed: {type(e).__name__})")
                        torch.cuda.synchronize()
                    d = pc.describe_policy_rollout(env._dims, H, cfg, 0)
                    say(f"    H {H:>2} K {steps:>3} {select:<6} {d['name']:<22} {d['threads_per_block']:>3} thr {d['lds_bytes']:>5} B LDS w{d['weights_in_lds']}  "
                        f"fused {t_fused:9.1f} us" +
                        f"  eager {t_eager:10.1f} us  eager, graph " + (f"{t_graph:10.1f} us" if t_graph is not None else "         -") +
                        f"  random {t_random:8.1f} us   eager / fused {t_eager / t_fused:6.2f}  " +
                        (f"graph / fused {t_graph / t_fused:6.2f}  " if t_graph is not None else "") +
                        f"fused / random {t_fused / t_random:5.2f}  ({t_fused / steps:.2f} us per step fused)")
        del env, twin, planes
        torch.cuda.empty_cache()

    shrink = 4 if args.quick else 0
    for label, S, T, K, mc, n, levels in (("4x4 / 2 tiles (cfg1)", 4, 2, 2, False, 1 << 20, 1 << 16), ("4x4 / 2 tiles (cfg1), small batch", 4, 2, 2, False, 4096, 4096),
                                          ("5x5 / 3 tiles, multi colour", 5, 3, 3, True, 1 << 18, 4096)):
        n = max(n >> shrink, 4096)
        run(label, S, T, K, mc, n, min(levels, n))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        open(args.log, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
