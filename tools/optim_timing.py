#!/usr/bin/env python3
"""Times the fused optimiser (include/tiler_slider_optim.h) against torch's own path on one GPU: HIP events on the launch stream
after warm-up, 50 repetitions a window, three windows a row with the rows of a shape taken in turn, one process.

    python tools/optim_timing.py [--log FILE] [--reps 50] [--quick]

Shapes: the six tensors of an ActorCriticNet for 4x4 / H = 32 (2,757 parameters) and for 8x8 / H = 64 (20,869), and one tensor of
4M elements.  Rows, each one optimiser step with the global-norm clip on:

    fused one / multi     FusedAdam.step(zero_grad=True), the one-block constant forced either way (one block only up to 128k elements)
    fused graph           the same step with the default constant, replayed from a captured graph
    foreach / fused=True  clip_grad_norm_ + torch.optim.AdamW(foreach=True | fused=True).step() + zero_grad(set_to_none=False)
    ... graph             the same three calls (capturable=True) replayed from a captured graph, where torch captures them

"us" is the window's device time over its repetitions - what the stream was busy or waiting for the host; "host us" the host's
wall time per call of the same window (the enqueue cost: what a launch-bound loop pays).  The row printed is the median window.
A sweep over one-tensor sizes in both forms follows: it is what the one-block constant (policy::kOneBlockMax) is set from.
Last, the optimiser's share of one actor-critic iteration (tools/actor_critic_demo.py --shared --fused-loss, 32 steps, H = 32) at
4,096 and at 1,048,576 boards: the iteration with torch.optim.Adam and with FusedAdam, and each optimiser's part alone.
profiles/optim_timing.log is where a run of this script belongs; run it under `timeout`.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--quick", action="store_true", help="64k elements instead of 4M, 65,536 boards instead of 1,048,576")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import ActorCriticNet, FusedAdam, RewardWeights, VecTilerSliderEnv
    from tiler_slider_amd import _optim_cabi as oc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.log:  # rewritten at every line: what was measured survives a run that ends early
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            open(args.log, "w").write("\n".join(lines) + "\n")

    dev = torch.device("cuda", 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, reps):
        """(device us, host us) per call of one window."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        host = (time.perf_counter() - t0) * 1e6 / reps
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps, host

    def time_rows(rows, reps, windows=3):
        """rows: {label: fn}; every fn warmed, then `windows` rounds over the rows in turn: {label: median (us, host us)}."""
        for fn in rows.values():
            for _ in range(5):
                fn()
        got = {k: [] for k in rows}
        for _ in range(windows):
            for k, fn in rows.items():
                got[k].append(window(fn, reps))
        return {k: sorted(v)[len(v) // 2] for k, v in got.items()}

    default = oc.tuning(oc.TUNE_ONE_BLOCK_MAX)
    say(f"one-block constant as built: {default}; {args.reps} repetitions a window, median of 3 windows")

    def params_of(shapes, seed=0):
        gen = torch.Generator(device=dev).manual_seed(seed)
        ps = [torch.randn(s, device=dev, generator=gen).requires_grad_(True) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device=dev, generator=gen)
        return ps

    def capture(fn):
        """fn captured on a side stream, one linear chain: graph.replay, or None with the reason where torch itself refuses to
        capture that optimiser (a RuntimeError).  Anything else, and any error the device reports afterwards, ends the script."""
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(dev)
        try:
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):
                    fn()
        except RuntimeError as e:
            torch.cuda.synchronize(dev)  # raises if the refusal left the device in error: nothing more is launched then
            return None, f"{type(e).__name__}: {str(e).splitlines()[0][:100]}"
        return graph, None

    def fused_step(shapes, knob):
        ps = params_of(shapes)
        opt = FusedAdam(ps, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
        opt.init_state()

        def fn():
            oc.tuning(oc.TUNE_ONE_BLOCK_MAX, knob)
            opt.step(zero_grad=True)
        return fn, opt, ps

    def torch_step(shapes, **kw):
        ps = params_of(shapes)
        opt = torch.optim.AdamW(ps, lr=1e-3, weight_decay=0.01, **kw)

        def fn():
            torch.nn.utils.clip_grad_norm_(ps, 1.0, foreach=True)
            opt.step()
            opt.zero_grad(set_to_none=False)
        return fn, opt, ps

    big = 1 << (16 if args.quick else 22)
    shape_sets = (("ActorCriticNet 4x4 / H = 32", ((80, 32), (32,), (32, 4), (4,), (32,), (1,))),
                  ("ActorCriticNet 8x8 / H = 64", ((320, 64), (64,), (64, 4), (4,), (64,), (1,))),
                  (f"one tensor of {big} elements", ((big,),)))
    for label, shapes in shape_sets:
        total = sum(int(np.prod(s)) for s in shapes)
        say(f"{label}: {total} elements in {len(shapes)} tensors")
        rows, keep, notes = {}, [], []
        if total <= (1 << 17):
            rows["fused one"] = fused_step(shapes, 1 << 40)[0]
        rows["fused multi"] = fused_step(shapes, 0)[0]
        fn, opt, ps = fused_step(shapes, default)
        graph, why = capture(fn)
        keep.append((graph, opt, ps))
        if graph is not None:
            rows["fused graph"] = graph.replay
        else:
            notes.append(f"fused graph: {why}")
        for name, kw in (("foreach", dict(foreach=True)), ("fused=True", dict(fused=True))):
            rows[name] = torch_step(shapes, **kw)[0]
            fn, opt, ps = torch_step(shapes, capturable=True, **kw)
            for _ in range(3):  # torch asks for warm-up steps before a capture: its state is created by the first
                fn()
            graph, why = capture(fn)
            keep.append((graph, opt, ps))
            if graph is not None:
                rows[name + " graph"] = graph.replay
            else:
                notes.append(f"{name} graph: not captured ({why})")
        res = time_rows(rows, args.reps)
        oc.tuning(oc.TUNE_ONE_BLOCK_MAX, default)
        for k, (us, host) in res.items():
            say(f"    {k:<18} {us:9.1f} us   host {host:8.1f} us")
        for n in notes:
            say(f"    {n}")
        del rows, keep
        torch.cuda.empty_cache()

    say("one tensor, the one-block form against the multi-block form (device us, clip on, zero_grad):")
    for n in (1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072):
        res = time_rows({"one": fused_step(((n,),), 1 << 40)[0], "multi": fused_step(((n,),), 0)[0]}, args.reps)
        oc.tuning(oc.TUNE_ONE_BLOCK_MAX, default)
        say(f"    {n:>7} elements   one {res['one'][0]:8.1f} us (host {res['one'][1]:6.1f})   multi {res['multi'][0]:8.1f} us (host {res['multi'][1]:6.1f})")

    # ---- the optimiser's share of one iteration of the shared-trunk actor-critic loop with the fused loss
    weights = RewardWeights(step=-0.01, win=1.0)
    for n in (4096, 1 << (16 if args.quick else 20)):
        env = VecTilerSliderEnv.from_seeds(np.arange(n, dtype=np.int64) % 4096, size=4, num_tiles=2, num_obstacles=2, obs_dtype=None, device=dev,
                                           max_steps=16, auto_reset=True)
        env.reset()
        D = env.onehot_channels * 16
        res = {}
        for which in ("torch.optim.Adam", "FusedAdam"):
            net = ActorCriticNet(D, 32, dev, generator=torch.Generator(device=dev).manual_seed(0))
            if which == "FusedAdam":
                opt = FusedAdam(net.parameters(), lr=1e-2)
                optim_part = lambda opt=opt: opt.step(zero_grad=True)
            else:
                opt = torch.optim.Adam(net.parameters(), lr=1e-2)

                def optim_part(opt=opt):
                    opt.step()
                    opt.zero_grad(set_to_none=False)
            it = [0]

            def iteration(net=net, optim_part=optim_part):
                out = env.rollout_policy(32, net.policy(), select="sample", seed=it[0], log=("start", "pos", "act", "flags"))
                it[0] += 1
                logits, v = env.trajectory_outputs(net, out)
                with torch.no_grad():
                    last = env.trajectory_outputs(net)[1][0]
                tr = env.trajectory_returns(out, 0.97, 0.9, values=v, last_value=last, reward=weights)
                info = env.trajectory_loss(logits, out, tr, values=v.contiguous(), value_coef=0.5, normalize_adv=True)
                info.loss.backward()
                optim_part()      # torch: zero_grad after the step instead of before the backward - the same launches

            iteration()
            reps = 20 if n <= 4096 else 5
            r = time_rows({"iteration": iteration, "optimiser": optim_part}, reps)
            res[which] = r
        say(f"{n} boards, 32 steps, H = 32, --shared --fused-loss (device us / host us):")
        for which, r in res.items():
            say(f"    {which:<17} iteration {r['iteration'][0]:10.1f} / {r['iteration'][1]:9.1f}   its optimiser alone {r['optimiser'][0]:8.1f} / {r['optimiser'][1]:7.1f}"
                f"   share {100 * r['optimiser'][0] / r['iteration'][0]:5.1f} %")
        del env
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
