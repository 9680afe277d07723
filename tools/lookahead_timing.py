#!/usr/bin/env python3
"""Times the lookahead (include/tiler_slider_lookahead.h) against what the tree offered before it, on one GPU: HIP events around
the launches after warm-up.

    python tools/lookahead_timing.py [--log FILE] [--launches 50] [--quick] [--no-graph]

Per shape, H = 16 and 64 hidden units, depth 1 .. 3, leaf "value", gamma = 0.99, rewards -1 a move, +1 a win, -1 an invalid move,
Gaussian weights, boards of from_seeds as reset() leaves them, in one process, fused and baseline alternating, twice:

    fused        one ts_lookahead: q, value, best and win_in of every board
    loop         (a) the loop a user writes without it: a twin environment set to each node's cells and stepped with each of the
                 four constant actions (4 + ... + 4^d ts_step), trajectory_outputs(net) on each of the 4^d leaf sets, and the
                 backup in torch (where / maximum); q and value only
    graph        the same loop captured once with torch.cuda.graph and replayed, where the capture works ("-" where it does not)
    leaves       (b) 4^d times one trajectory_outputs(net) on the same boards: the leaf evaluations alone - how far the search is
                 from "the network, 4^d times"

Before a row is timed the fused q is compared with the loop's to 1e-4 of its scale (a sanity check of what is about to be timed;
the tests hold the rigorous bound).  profiles/lookahead_timing.log is where a run of this script belongs;
run it under `timeout`.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAMMA, W_STEP, W_WIN, W_INVALID = 0.99, -1.0, 1.0, -1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the boards")
    ap.add_argument("--no-graph", action="store_true", help="do not try to capture the loop")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import ActorCriticNet, RewardWeights, VecTilerSliderEnv
    from tiler_slider_amd import _cabi
    from tiler_slider_amd import _lookahead_cabi as lc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.log:  # rewritten at every line: what was measured survives a run that ends early
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            open(args.log, "w").write("\n".join(lines) + "\n")

    dev = torch.device("cuda", 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reward = RewardWeights(step=W_STEP, win=W_WIN, invalid=W_INVALID)

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

    def run(label, S, T, Ko, mc, n, levels):
        make = lambda: VecTilerSliderEnv.from_seeds(np.arange(n, dtype=np.int64) % levels, size=S, num_tiles=T, num_obstacles=Ko, multi_color=mc,
                                                    obs_dtype=None, device=dev, max_steps=1 << 20, strict=False)
        env, twin = make(), make()
        env.reset()
        twin.reset()
        D = env.onehot_channels * S * S
        say(f"{label}: {n} boards, {D} features")
        actions = [torch.full((n,), a, dtype=torch.uint8, device=dev) for a in range(4)]
        zero = torch.zeros(n, dtype=torch.float32, device=dev)
        for H in (16, 64):
            gen = torch.Generator(device=dev)
            gen.manual_seed(H)
            net = ActorCriticNet(D, H, dev, generator=gen)
            with torch.no_grad():
                for p in net.parameters():
                    p.copy_(torch.randn(p.shape, device=dev, generator=gen))
                    p.requires_grad_(False)

            def node(cells, plies):
                """[n, 4]: the backed-up values of the four actions on `cells`, the loop written by hand."""
                qs = []
                for a in range(4):
                    twin._pos.copy_(cells)
                    twin._done.zero_()
                    twin.step_async(actions[a])
                    won = (twin._flags & _cabi.FLAG_IS_WON) != 0
                    same = (twin._flags & _cabi.FLAG_INVALID_MOVE) != 0
                    r = W_STEP + W_WIN * won.float() + W_INVALID * same.float()
                    below = twin.trajectory_outputs(net)[1][0] if plies == 1 else node(twin._pos.clone(), plies - 1).max(dim=1).values
                    qs.append(r + GAMMA * torch.where(won, zero, below))
                return torch.stack(qs, dim=1)

            for depth in (1, 2, 3):
                start = env._pos.clone()
                held = {}

                def fused():
                    held["fused"] = env.lookahead(net, depth=depth, gamma=GAMMA, reward=reward)

                def loop():
                    q = node(start, depth)
                    held["loop"] = (q, q.max(dim=1).values)

                def leaves():
                    for _ in range(4 ** depth):
                        held["leaf"] = env.trajectory_outputs(net)

                fused()
                loop()
                torch.cuda.synchronize()
                alive = ~env.is_won()
                scale = float(held["loop"][0][alive].abs().max())
                diff = float((held["fused"].q[alive] - held["loop"][0][alive]).abs().max())
                assert diff <= 1e-4 * max(1.0, scale), (label, H, depth, diff, scale)
                replay = None
                if not args.no_graph:
                    try:
                        side = torch.cuda.Stream(device=dev)
                        side.wait_stream(torch.cuda.current_stream(dev))
                        with torch.cuda.stream(side):
                            loop()
                        torch.cuda.current_stream(dev).wait_stream(side)
                        torch.cuda.synchronize()
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            loop()
                        replay = g.replay
                    except Exception as e:  # the capture does not work here: say so in the row
                        say(f"    (capture failed: {type(e).__name__}: {str(e).splitlines()[0][:120]})")
                        torch.cuda.synchronize()
                runs = []
                for _ in range(2):
                    t_f = time_us(fused, args.launches)
                    t_l = time_us(loop, max(3, args.launches // (1 if depth == 1 else 5)))
                    t_g = time_us(replay, max(3, args.launches // (1 if depth == 1 else 5))) if replay else float("nan")
                    t_b = time_us(leaves, max(3, args.launches // (1 if depth == 1 else 5)))
                    runs.append((t_f, t_l, t_g, t_b))
                d = lc.describe_lookahead(env._dims, H, 1, depth, lc.LEAVES["value"])
                f = lambda i: " / ".join(f"{r[i]:10.1f}" for r in runs)
                best = [min(r[i] for r in runs) for i in range(4)]
                say(f"    H {H:>2} depth {depth} {d['name']:<18} {d['threads_per_block']:>3} thr {d['lds_bytes']:>5} B w{d['weights_in_lds']}  "
                    f"fused {f(0)} us  loop {f(1)} us  graph {f(2)} us  leaves {f(3)} us  "
                    f"loop / fused {best[1] / best[0]:6.1f}  graph / fused {best[2] / best[0]:6.1f}  fused / leaves {best[0] / best[3]:5.2f}")
                del replay
        del env, twin
        torch.cuda.empty_cache()

    shrink = 4 if args.quick else 0
    for label, S, T, Ko, mc, n, levels in (("4x4 / 2 tiles (cfg1)", 4, 2, 2, False, 1 << 20, 1 << 16), ("4x4 / 2 tiles (cfg1), small batch", 4, 2, 2, False, 4096, 4096),
                                           ("5x5 / 3 tiles, multi colour", 5, 3, 3, True, 1 << 18, 4096)):
        n = max(n >> shrink, 4096)
        run(label, S, T, Ko, mc, n, min(levels, n))


if __name__ == "__main__":
    main()
