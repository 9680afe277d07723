#!/usr/bin/env python3
"""Times the trainable policies (include/tiler_slider_train.h) on one GPU: HIP events around the launches after warm-up.

    python tools/train_timing.py [--log FILE] [--launches 50] [--baseline-launches 10] [--quick] [--no-graph]

Per shape, H = 16 and 64 hidden units, K = 16 and 100 logged steps, in one process and one run, on the trajectory of a
rollout_policy(K, ..., log=("start", "pos")) of an observation-less auto-reset actor with Gaussian weights and a Gaussian dz:

    fused fwd    one ts_train_forward over all K * N logged board-steps
    fused bwd    one ts_train_backward (the four gradient buffers zero-filled outside the timed region)
    dense fwd    the loop a user writes without the library, K times: the planes of step k - a twin's cells set from the log and
                 env.encode_onehot(), or a torch scatter of ones into zeroed planes, whichever is faster (both are timed once) -
                 then addmm / relu / addmm under torch.no_grad()
    dense f+b    the same loop with autograd: every step's logits.backward(dz[k]), the gradients accumulating in .grad
    graph f+b    the dense f+b loop captured into one graph and replayed ("-" with --no-graph).  Any failure of the capture or the
                 replay ENDS the run after the log is written - the error of a refused capture cannot be told from a GPU fault,
                 and nothing more may be launched after one: run again with --no-graph

dense bwd in the table is dense f+b minus dense fwd.  Before a row is timed the two sides are compared: the fused logits and
the four fused gradients against the dense loop's, to 1e-3 of their scale (a sanity check of what is about to be timed; the
tests hold the rigorous bound).  The backward's atomic bytes per launch are the plan's end-of-block flush (flush_bytes of
ts_describe_train_backward), shown against a chip-wide rate of 1.3 TB/s of added bytes.  profiles/train_timing.log is where two
runs of this script belong; run it under `timeout`.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ATOMIC_BYTES_PER_US = 1.3e6  # 1.3 TB/s of added bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--baseline-launches", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the boards, K = 16 only")
    ap.add_argument("--no-graph", action="store_true", help="do not capture the dense loop into a graph")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import PolicyNet, VecTilerSliderEnv
    from tiler_slider_amd import _train_cabi as tc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.log:  # rewritten at every line: what was measured survives a run that ends early
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            open(args.log, "w").write("\n".join(lines) + "\n")

    L = tc.lib()
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

    def make(S, T, K, mc, n, levels):
        env = VecTilerSliderEnv.from_seeds(np.arange(n, dtype=np.int64) % levels, size=S, num_tiles=T, num_obstacles=K, multi_color=mc, obs_dtype=None,
                                           device=dev, max_steps=20, auto_reset=True)
        env.reset()
        return env

    def run(label, S, T, Ko, mc, n, levels):
        env, twin = make(S, T, Ko, mc, n, levels), make(S, T, Ko, mc, n, levels)
        Cc, Ch = S * S, env.onehot_channels
        D = Ch * Cc
        planes = torch.empty((n, Ch, S, S), dtype=torch.float32, device=dev)
        say(f"{label}: {n} boards, {D} features")
        # the constant planes of the scatter baseline (obstacles, targets), built once; the tile planes are scattered per step
        twin.reset()
        const = twin.encode_onehot().flatten(1).clone()
        tile_lo, tile_hi = Cc, (1 + T) * Cc if mc else 2 * Cc
        const[:, tile_lo:tile_hi] = 0
        rows = torch.arange(n, device=dev)
        for H in (16, 64):
            gen = torch.Generator(device=dev)
            gen.manual_seed(H)
            net = PolicyNet(D, H, dev, generator=gen)
            with torch.no_grad():
                for p in net.parameters():
                    p.copy_(torch.randn(p.shape, device=dev, generator=gen))
            dense = [p.detach().clone().requires_grad_(True) for p in (net.w1, net.b1, net.w2, net.b2)]
            for steps in ((16,) if args.quick else (16, 100)):
                env.reset()
                out = env.rollout_policy(steps, net.policy(), select="sample", seed=0x7131, stats=False, log=("start", "pos"))
                cells = lambda k: out.start_pos if k == 0 else out.pos_log[k - 1]
                dz = torch.randn((steps, n, 4), device=dev, generator=gen)
                logits = torch.empty((steps, n, 4), dtype=torch.float32, device=dev)
                grads = [torch.zeros_like(p) for p in dense]
                mlp = net.policy()._mlp(env)
                tin = tc.TrainIn(out.start_pos.data_ptr(), out.pos_log.data_ptr(), steps, 0)
                grad = tc.MlpGrad(*(g.data_ptr() for g in grads))
                fwd = lambda: tc.check(L.ts_train_forward(C.byref(env._dims), C.byref(env._state), C.byref(mlp), C.byref(tin), logits.data_ptr(),
                                                          stream()), "ts_train_forward")
                bwd = lambda: tc.check(L.ts_train_backward(C.byref(env._dims), C.byref(env._state), C.byref(mlp), C.byref(tin), dz.data_ptr(),
                                                           C.byref(grad), stream()), "ts_train_backward")

                def planes_encode(k):
                    twin._pos.copy_(cells(k))
                    return twin.encode_onehot(out=planes).flatten(1)

                def planes_scatter(k):
                    x = const.clone()
                    c = cells(k).to(torch.int64).clamp_(max=Cc - 1)
                    for t in range(T):
                        x[rows, (Cc * (1 + t) if mc else Cc) + c[t]] = 1.0
                    return x

                t_enc = time_us(lambda: planes_encode(min(1, steps - 1)), args.baseline_launches)
                t_sca = time_us(lambda: planes_scatter(min(1, steps - 1)), args.baseline_launches)
                planes_of = planes_encode if t_enc <= t_sca else planes_scatter

                def net_of(x):
                    return torch.addmm(dense[3], torch.relu(torch.addmm(dense[1], x, dense[0])), dense[2])

                def dense_fwd():
                    with torch.no_grad():
                        for k in range(steps):
                            net_of(planes_of(k))

                def dense_both():
                    for k in range(steps):
                        net_of(planes_of(k)).backward(dz[k])

                # a sanity check of the two sides
                fwd()
                for g in grads:
                    g.zero_()
                bwd()
                for p in dense:
                    p.grad = None
                dense_both()
                with torch.no_grad():
                    for k in (0, steps - 1):
                        z = net_of(planes_of(k))
                        assert float((z - logits[k]).abs().max()) <= 1e-3 * max(1.0, float(z.abs().max())), (label, H, steps, k)
                for g, p in zip(grads, dense):
                    assert float((g - p.grad).abs().max()) <= 1e-3 * max(1.0, float(p.grad.abs().max())), (label, H, steps, tuple(p.shape))
                t_fwd, t_bwd = time_us(fwd, args.launches), time_us(bwd, args.launches)
                t_dfwd, t_dboth = time_us(dense_fwd, args.baseline_launches), time_us(dense_both, args.baseline_launches)
                torch.cuda.synchronize()
                t_graph = None
                if not args.no_graph:
                    try:
                        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
                        with torch.cuda.stream(side):
                            with torch.cuda.graph(graph, stream=side):
                                dense_both()
                        t_graph = time_us(graph.replay, args.baseline_launches)
                        del graph
                    except Exception as e:
                        say(f"        graph capture or replay of the dense loop failed ({type(e).__name__}: {e}); the run ends here: use --no-graph")
                        raise SystemExit(3)
                df, db = tc.describe_train_forward(env._dims, H, steps), tc.describe_train_backward(env._dims, H, steps)
                floor = db["flush_bytes"] / ATOMIC_BYTES_PER_US
                say(f"    H {H:>2} K {steps:>3} fwd {df['threads_per_block']:>3} thr {df['lds_bytes']:>5} B w{df['weights_in_lds']}; bwd {db['blocks']:>4} blocks "
                    f"{db['lds_bytes']:>5} B w{db['weights_in_lds']} g{db['grads_in_lds']}  planes by {'encode' if planes_of is planes_encode else 'scatter'} "
                    f"({t_enc:.0f} / {t_sca:.0f} us)  fused fwd {t_fwd:9.1f} us  fused bwd {t_bwd:9.1f} us  dense fwd {t_dfwd:10.1f} us  dense f+b {t_dboth:10.1f} us  "
                    f"graph f+b " + (f"{t_graph:10.1f} us" if t_graph is not None else "         -") +
                    f"  dense fwd / fused fwd {t_dfwd / t_fwd:6.2f}  dense bwd / fused bwd {(t_dboth - t_dfwd) / t_bwd:6.2f}  "
                    f"dense f+b / fused f+b {t_dboth / (t_fwd + t_bwd):6.2f}  " +
                    (f"graph f+b / fused f+b {t_graph / (t_fwd + t_bwd):6.2f}  " if t_graph is not None else "") +
                    f"flush atomics {db['flush_bytes']} B = {floor:.1f} us at 1.3 TB/s")
                del out, dz, logits
        del env, twin, planes, const
        torch.cuda.empty_cache()

    shrink = 4 if args.quick else 0
    for label, S, T, Ko, mc, n, levels in (("4x4 / 2 tiles (cfg1)", 4, 2, 2, False, 1 << 20, 1 << 16), ("4x4 / 2 tiles (cfg1), small batch", 4, 2, 2, False, 4096, 4096),
                                           ("5x5 / 3 tiles, multi colour", 5, 3, 3, True, 1 << 18, 4096)):
        n = max(n >> shrink, 4096)
        run(label, S, T, Ko, mc, n, min(levels, n))


if __name__ == "__main__":
    main()
