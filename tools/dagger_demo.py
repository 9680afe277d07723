#!/usr/bin/env python3
"""DAgger on a reach shape, every step of the loop one launch of this tree.

    python tools/dagger_demo.py [--iterations 60] [--steps 24] [--hidden 32] [--levels 1024] [--log FILE]

1,024 levels of 5x5 boards with four tiles and three obstacles, multi colour - 390,625 placements a level, beyond the dense tables -
whose targets lie where ten random moves leave the tiles, so that they can be won.  Once: build_reach_table() solves every level
over the placements play can reach, build_reach_index() sorts them by distance.  Then per iteration:

    place_at_distance(ridx, 1, hi, only_done=True)       finished boards restart 1 .. hi moves from the win (the curriculum: hi
                                                         grows by one whenever the share of boards that won passes 0.5)
    rollout_policy(K, net, expert=rt, beta=beta_i,       the behaviour policy: the expert with probability beta_i = beta0 * decay^i,
                   log=("start", "pos", "expert"))       the learner otherwise - and the expert's move on every board visited, from
                                                         the same launch (include/tiler_slider_mixed.h)
    trajectory_logits(net, out)                          the learner's logits on the boards visited
    trajectory_loss(logits, out, labels=out.expert_log)  cross-entropy against the expert's moves; .backward() and FusedAdam

Progress is the network's greedy play from EVERY state the tables hold, exactly: build_policy_table(net, table=rt) and
score_policy() - the share of states it solves, solves optimally, and on which its move is one of the expert's.
profiles/dagger_demo.log is where a run of this script belongs.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--levels", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--beta", type=float, default=1.0, help="beta of iteration 0")
    ap.add_argument("--decay", type=float, default=0.9, help="beta_i = beta * decay ** i")
    ap.add_argument("--score-every", type=int, default=10)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import FusedAdam, PolicyNet, VecTilerSliderEnv

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.log:
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            open(args.log, "w").write("\n".join(lines) + "\n")

    dev = torch.device("cuda", 0)
    S, T, Ko, L, K = 5, 4, 3, args.levels, args.steps
    walk = VecTilerSliderEnv.from_seeds(np.arange(L, dtype=np.int64), size=S, num_tiles=T, num_obstacles=Ko, multi_color=True, obs_dtype=None, device=dev)
    walk.reset()
    walk.rollout(10, "random", seed=0x3A1C, stats=False)
    env = VecTilerSliderEnv.from_arrays(S, walk._blk.clone(), walk._init.clone(), walk.positions.clone(), multi_color=True, obs_dtype=None, device=dev,
                                        max_steps=30)
    env.reset()
    rt = env.build_reach_table(capacity=4096)
    ridx = env.build_reach_index(rt)
    net = PolicyNet(env.onehot_channels * S * S, args.hidden, dev, generator=torch.Generator(device=dev).manual_seed(0))
    opt = FusedAdam(net.parameters(), lr=args.lr)
    say(f"DAgger on {L} levels of {S}x{S} / {T} tiles / {Ko} obstacles, multi colour: {int((rt.root_moves >= 1).sum())} can be won from their root, "
        f"{int(rt.full.sum())} FULL, deepest entry {int(rt.deepest.max())}; K {K}, hidden {args.hidden}, lr {args.lr}, beta {args.beta} x {args.decay}^i")

    def score(it):
        s = env.score_policy(env.build_policy_table(net, table=rt), rt)    # three launches; no state is touched
        say(f"  [{it:>3}] greedy play over every state of the tables: solved {float(s.solved_share):.3f}, optimally {float(s.optimal_share):.3f}, "
            f"agreement with the expert {float(s.agreement):.3f}")

    score(0)
    hi = 1
    for it in range(args.iterations):
        beta = args.beta * args.decay ** it
        start = env.place_at_distance(ridx, 1, hi, seed=0xC0DE, step_index=it, only_done=it > 0)
        out = env.rollout_policy(K, net.policy(), select="sample", seed=0xDA66, step_index=it * K, log=("start", "pos", "expert", "who"), expert=rt, beta=beta)
        info = env.trajectory_loss(env.trajectory_logits(net, out), out, labels=out.expert_log)
        info.loss.backward()
        opt.step(zero_grad=True)
        won = float((out.wins > 0).float().mean())
        played = torch.bincount(out.who_log.flatten().long(), minlength=3).tolist()
        say(f"iteration {it:>3}: beta {beta:.3f}, starts 1..{hi} moves from the win ({int(start.placed.sum())} boards placed), loss {float(info.loss.detach()):.4f}, "
            f"labelled samples {int((out.expert_log != 255).sum())}, boards that won {won:.3f}, played by network / expert {played[0]} / {played[1]}")
        if won > 0.5 and hi < 24:
            hi += 1
        if args.score_every and (it + 1) % args.score_every == 0:
            score(it + 1)


if __name__ == "__main__":
    main()
