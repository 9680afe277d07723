#!/usr/bin/env python3
"""Times the reach policy tables (include/tiler_slider_rptable.h) against what they replace, on one GPU: HIP events around the
calls after warm-up.

    python tools/rptable_timing.py [--log FILE] [--launches 3] [--quick]

16,384 reference levels of 5x5 / 4 tiles / 3 obstacles, multi colour, whose targets lie where ten random moves leave the tiles, a
reach table at capacity 4,096 (1 GiB), and a Gaussian network of 64 hidden units.

    tables     build_policy_table(net, table=rt) - ts_rptable_actions and ts_rptable_walk - plus score_policy() - ts_rptable_score:
               the exact outcome of the network's greedy play from every state of every level
    rollouts   what the tree offered before this library for the same question: an environment of one board per live state
               standing on it (built once, outside the timing), then rollout_policy(252, select="greedy") from there; the
               boards that win are the states the policy solves, first_win their entries
    global     the walk alone on a table of the same levels at capacity 8,192: rows of 16,384 slots, walked in the output row

Before anything is timed the two sides are compared: first_win of the rollout is the entry of the policy table on every state
the table solves, and 0 on every other.  profiles/rptable_timing.log is where a run of this script belongs;
run it under `timeout`.
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
    ap.add_argument("--quick", action="store_true", help="1,024 levels")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import MlpPolicy, VecTilerSliderEnv
    from tiler_slider_amd import _rptable_cabi as xc

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

    S, T, Ko, H = 5, 4, 3, 64
    LEVELS, CAPACITY = (1024 if args.quick else 16384), 4096
    C_ = S * S
    walk = VecTilerSliderEnv.from_seeds(np.arange(LEVELS, dtype=np.int64), size=S, num_tiles=T, num_obstacles=Ko, multi_color=True, obs_dtype=None, device=dev)
    walk.reset()
    walk.rollout(10, "random", seed=0x3A1C, stats=False)
    blk, init, tgt = walk._blk.clone(), walk._init.clone(), walk.positions.clone()
    env = VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=True, obs_dtype=None, device=dev, max_steps=1000)
    env.reset()
    rt = env.build_reach_table(capacity=CAPACITY)
    g = torch.Generator(device="cpu").manual_seed(29)
    D = (1 + 2 * T) * C_
    policy = MlpPolicy(*(torch.randn(s, generator=g).to(dev) for s in ((H, D), (H,), (4, H), (4,))))
    names = [xc.describe_rptable_actions(env._dims, H, rt.slots), xc.describe_rptable_walk(env._dims, rt.slots), xc.describe_rptable_score(env._dims, rt.slots)]
    say(f"5x5 / 4 tiles / 3 obstacles: {LEVELS} levels ({int((rt.root_moves >= 1).sum())} can be won, {int(rt.full.sum())} FULL, "
        f"{int(rt.count.clamp(min=0).sum())} states), table {rt.table.numel() * 8 / 2**20:.0f} MiB, {H} hidden units")
    say("    " + ", ".join(f"{d['name']} ({d['blocks']} x {d['threads_per_block']}, {d['lds_bytes']} B LDS)" for d in names))

    held = {}

    def tables():
        held["pt"] = env.build_policy_table(policy, table=rt)
        held["score"] = env.score_policy(held["pt"], rt)

    tables()
    pt, score = held["pt"], held["score"]
    total = score.columns.sum(dim=0).tolist()
    say(f"    score over all levels: valid {total[0]}, solvable {total[1]}, solved {total[2]}, optimal {total[3]}, agree {total[4]}, excess {total[5]}, "
        f"deep {total[6]}; deepest policy entry {int(pt.deepest.max())}")

    # one board per live state, standing on it (in level and slot order)
    live = (pt.table < 0).nonzero()
    lv = live[:, 0]
    words = pt.table[live[:, 0], live[:, 1]]
    keys, entry = words & ((1 << 48) - 1), (words >> 48) & 0xFF
    weights = torch.tensor([C_ ** t for t in range(T)], dtype=torch.int64, device=dev).unsqueeze(1)
    cells = ((keys.unsqueeze(0) // weights) % C_).to(torch.uint8).contiguous()
    boards = VecTilerSliderEnv.from_arrays(S, blk[:, lv].contiguous(), cells, tgt[:, lv].contiguous(), multi_color=True, obs_dtype=None, device=dev, max_steps=1000)
    boards.reset()
    got = {}

    def rollouts():
        boards._pos.copy_(cells)
        boards._step_count.zero_()
        boards._done.zero_()
        got["out"] = boards.rollout_policy(252, policy, select="greedy")

    rollouts()
    torch.cuda.synchronize()
    solved = (entry >= 1) & (entry <= 252)
    first_win = got["out"].first_win.long()
    assert torch.equal(first_win[solved], entry[solved]) and not bool(first_win[~solved].any()), "the rollouts and the table disagree"
    say(f"    the rollouts' first_win is the table's entry on all {int(solved.sum())} solved states and 0 on the other {int((~solved).sum())}")

    t_a = time_us(rollouts, args.launches)
    t_f1 = time_us(tables, args.launches)
    t_b = time_us(rollouts, args.launches)
    t_f2 = time_us(tables, args.launches)
    say(f"    build_policy_table(table=rt) + score_policy {t_f1:10.1f} / {t_f2:10.1f} us   one board per state + rollout_policy(252, greedy) {t_a:10.1f} / {t_b:10.1f} us   "
        f"({boards.num_envs} boards; fastest rollouts / slowest tables {min(t_a, t_b) / max(t_f1, t_f2):6.2f})")
    for name, fn in (("actions", lambda: env.build_policy_table(policy, table=rt)), ("walk alone", lambda: env.walk_actions(pt.act, table=rt)),
                     ("score alone", lambda: env.score_policy(pt, rt))):
        say(f"    {name:<12} {time_us(fn, args.launches):10.1f} us" + ("   (actions + walk)" if name == "actions" else ""))

    # the same levels at capacity 8,192: rows of 16,384 slots, walked in the output row (the global form), every round over the row
    del boards, got, held, pt, score
    torch.cuda.empty_cache()
    wide = env.build_reach_table(capacity=2 * CAPACITY)
    d = xc.describe_rptable_walk(env._dims, wide.slots)
    wide_pt = env.build_policy_table(policy, table=wide)
    say(f"    capacity {2 * CAPACITY}: {d['name']} ({d['blocks']} x {d['threads_per_block']}), table {wide.table.numel() * 8 / 2**20:.0f} MiB, "
        f"deepest policy entry {int(wide_pt.deepest.max())}: walk alone {time_us(lambda: env.walk_actions(wide_pt.act, table=wide), args.launches):10.1f} us")


if __name__ == "__main__":
    main()
