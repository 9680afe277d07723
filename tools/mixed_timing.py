#!/usr/bin/env python3
"""Times the mixed rollouts (include/tiler_slider_mixed.h) against what they replace, on one GPU: HIP events around the calls after
warm-up, the sides of a comparison alternating inside this one command.

    python tools/mixed_timing.py [--log FILE] [--launches 3] [--quick]

Two shapes, observation-less auto-reset environments (max_steps 30), epsilon = 0.1, select "sample":
    dense   1,048,576 4x4 boards of two tiles and two obstacles, single colour, a DistanceTable row per board
    reach   65,536 5x5 boards of four tiles and three obstacles, multi colour, the ReachTable (capacity 4,096) of 16,384 levels -
            their targets lie where ten random moves leave the tiles, so they can be won - read through rows=
K = 32 and 100 steps, hidden widths 16 and 64, beta = 0, 0.5 and 1.

    fused            one rollout_policy(expert=, beta=): K steps, the state written back, the last flags, no other output
    fused + labels   the same with the three label logs (expert, moves, best) - at beta = 0 this is what reads the table
    (a) loop         what it replaces, K times: policy_logits, a torch softmax sample, expert_actions_from, a torch mix of the
                     two with a torch.rand draw for beta and one for epsilon, step; eager, and captured once and replayed
    (b) two launches rollout_policy(log=("start", "pos")) and trajectory_labels() of its log: the beta = 0 case with labels
    (c) policy       rollout_policy alone, the same logs as `fused`: what the lookups cost

The loop draws its own random numbers (the fused call's draws are bits the loop cannot see), so the two sides are not compared
byte for byte here: tests/test_gpu_mixed.py does that against the CPU yardstick.  Every side is timed twice around the other;
the larger relative spread of such a pair is the margin within which a ratio is read.  profiles/mixed_timing.log is where a run
of this script belongs; run it under `timeout`.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="K = 8, H = 16, a sixteenth of the boards")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import PolicyNet, VecTilerSliderEnv
    from tiler_slider_amd import _mixed_cabi as mc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.log:  # rewritten at every line: what was measured survives a run that ends early
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            open(args.log, "w").write("\n".join(lines) + "\n")

    dev = torch.device("cuda", 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def time_us(fn, launches, warm=1):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches

    EPS, MAX_STEPS, SEED = 0.1, 30, 0x313ED
    shrink = 16 if args.quick else 1

    def dense_case():
        n = (1 << 20) // shrink
        env = VecTilerSliderEnv.from_seeds(np.arange(n, dtype=np.int64), size=4, num_tiles=2, num_obstacles=2, multi_color=False, obs_dtype=None, device=dev,
                                           max_steps=MAX_STEPS, auto_reset=True)
        env.reset()
        table = env.build_table()
        return f"dense: {n} 4x4 boards of two tiles, a DistanceTable of {table.dist.numel() / 2**20:.0f} MiB", env, table, None

    def reach_case():
        n, levels = (1 << 16) // shrink, (1 << 14) // shrink
        walk = VecTilerSliderEnv.from_seeds(np.arange(levels, dtype=np.int64), size=5, num_tiles=4, num_obstacles=3, multi_color=True, obs_dtype=None, device=dev)
        walk.reset()
        walk.rollout(10, "random", seed=0x3A1C, stats=False)
        blk, init, tgt = walk._blk.clone(), walk._init.clone(), walk.positions.clone()
        small = VecTilerSliderEnv.from_arrays(5, blk, init, tgt, multi_color=True, obs_dtype=None, device=dev)
        small.reset()
        rt = small.build_reach_table(capacity=4096)
        rows = (torch.arange(n, device=dev) % levels).to(torch.int32)
        idx = rows.long()
        env = VecTilerSliderEnv.from_arrays(5, blk[:, idx].contiguous(), init[:, idx].contiguous(), tgt[:, idx].contiguous(), multi_color=True, obs_dtype=None,
                                            device=dev, max_steps=MAX_STEPS, auto_reset=True)
        env.reset()
        return (f"reach: {n} 5x5 boards of four tiles, a ReachTable of {levels} levels ({int((rt.root_moves >= 1).sum())} can be won, "
                f"{int(rt.full.sum())} FULL), {rt.table.numel() * 8 / 2**20:.0f} MiB"), env, rt, rows

    for make in (dense_case, reach_case):
        label, env, table, rows = make()
        say(label)
        n = env.num_envs
        kind = mc.REACH if rows is not None else mc.DENSE
        for H in ((16,) if args.quick else (16, 64)):
            net = PolicyNet(env.onehot_channels * env.size * env.size, H, env.device, generator=torch.Generator(device=dev).manual_seed(H))
            policy = net.policy()
            for K in ((8,) if args.quick else (32, 100)):
                u, v = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
                rnd = torch.empty(n, dtype=torch.uint8, device=dev)

                def fused(beta, log=()):
                    return lambda: env.rollout_policy(K, policy, select="sample", epsilon=EPS, seed=SEED, stats=False, log=log, expert=table, beta=beta, rows=rows)

                def loop(beta):
                    def body():
                        for _ in range(K):
                            z = env.policy_logits(policy)
                            a = torch.multinomial(torch.softmax(z, dim=1), 1).squeeze(1).to(torch.uint8)
                            if beta > 0.0:
                                x = env.expert_actions_from(table, rows=rows)
                                a = torch.where((u.uniform_() < beta) & (x != 255), x, a)
                            a = torch.where(v.uniform_() < EPS, rnd.random_(0, 4), a)
                            env.step(a)
                    return body

                plain = lambda log=(): (lambda: env.rollout_policy(K, policy, select="sample", epsilon=EPS, seed=SEED, stats=False, log=log))

                def two_launches():
                    out = env.rollout_policy(K, policy, select="sample", epsilon=EPS, seed=SEED, stats=False, log=("start", "pos"))
                    return env.trajectory_labels(out, table, rows=rows)

                cfg = mc.MixedCfg(K, 1, 1, 1, 0, 0, 0, 0, 1, kind, 0, None, None, 2 if rows is None else table.slots, None, 0, None)
                d = mc.describe_mixed_rollout(env._dims, H, cfg)
                say(f"  H {H:>2}  K {K:>3}  {d['name']}  {d['threads_per_block']} threads, {d['lds_bytes']} bytes of LDS, weights {'in LDS' if d['weights_in_lds'] else 'gathered'}")
                # (c) what the lookups cost, and (b) the two-launch form against the fused labels at beta = 0
                t_p1 = time_us(plain(), args.launches)
                t_f0 = time_us(fused(0.0), args.launches)
                t_p2 = time_us(plain(), args.launches)
                say(f"    beta 0    no table read: fused {t_f0:10.1f} us   (c) rollout_policy {t_p1:10.1f} / {t_p2:10.1f} us   fused / policy {t_f0 / min(t_p1, t_p2):5.2f}")
                labels = ("start", "pos", "expert", "moves", "best")
                t_b1 = time_us(two_launches, args.launches)
                t_fl = time_us(fused(0.0, labels), args.launches)
                t_b2 = time_us(two_launches, args.launches)
                spread = abs(t_b1 - t_b2) / min(t_b1, t_b2)
                say(f"    beta 0    with labels:   fused {t_fl:10.1f} us   (b) rollout_policy + trajectory_labels {t_b1:10.1f} / {t_b2:10.1f} us   spread {100 * spread:4.1f} %   "
                    f"two launches / fused {min(t_b1, t_b2) / t_fl:5.2f}   ({t_fl * 1e3 / (n * K):.3f} ns per board-step fused)")
                for beta in (0.5, 1.0):
                    body = loop(beta)
                    t_l1 = time_us(body, 1)
                    t_f = time_us(fused(beta), args.launches)
                    t_l2 = time_us(body, 1)
                    t_fl = time_us(fused(beta, labels[2:]), args.launches)
                    torch.cuda.synchronize()
                    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
                    with torch.cuda.stream(side):
                        with torch.cuda.graph(graph, stream=side):
                            body()
                    t_g1 = time_us(graph.replay, args.launches)
                    t_f2 = time_us(fused(beta), args.launches)
                    t_g2 = time_us(graph.replay, args.launches)
                    del graph
                    spread = max(abs(t_l1 - t_l2) / min(t_l1, t_l2), abs(t_g1 - t_g2) / min(t_g1, t_g2))
                    say(f"    beta {beta:<4}  fused {t_f:10.1f} / {t_f2:10.1f} us   with labels {t_fl:10.1f} us   (a) loop {t_l1:10.1f} / {t_l2:10.1f} us   loop, graph {t_g1:10.1f} / {t_g2:10.1f} us   "
                        f"spread {100 * spread:4.1f} %   fastest loop / slowest fused {min(t_l1, t_l2, t_g1, t_g2) / max(t_f, t_f2):6.2f}   "
                        f"fused / (c) policy {max(t_f, t_f2) / min(t_p1, t_p2):5.2f}   ({max(t_f, t_f2) * 1e3 / (n * K):.3f} ns per board-step fused)")
        del env, table
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
