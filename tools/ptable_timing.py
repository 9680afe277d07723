#!/usr/bin/env python3
"""Times the policy tables (include/tiler_slider_ptable.h) beside the composition they replace, on one GPU: HIP events on the
launch stream after warm-up, three windows a row with the rows of a shape taken in turn, the median window and the spread of the
three, one process.

    python tools/ptable_timing.py [--log FILE] [--reps 200] [--quick]

Shapes: 256 and 16,384 levels of 4x4 boards with two tiles (256 placements a level), networks of 16 and of 64 hidden units; 256
levels of 5x5 boards with two tiles (625 placements), 16 hidden units.

Rows: `build_policy_table` is VecTilerSliderEnv.build_policy_table(): ts_ptable_actions and ts_ptable_walk, timed together and
each on its own; `score_policy` the one launch of ts_ptable_score.  `rollout` is what a user writes without them for the same
answer: an environment of one board per VALID placement of every level (fewer boards than L x states: the comparison favours
it), reset() and rollout_policy(252, greedy, epsilon 0) in strict mode, whose first_win is the table's distance.  `policy_logits`
on that environment is the network once per board through the policy library: its time per board stands beside
ts_ptable_actions' time per placement.  profiles/ptable_timing.log is where a run of this script belongs;
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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="1,024 levels instead of 16,384")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import MlpPolicy, VecTilerSliderEnv
    from tiler_slider_amd import _ptable_cabi as xc

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
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    def time_rows(rows, windows=3):
        """rows: {label: (fn, reps)}; every fn warmed, then `windows` rounds over the rows in turn: {label: (median, spread) us}."""
        for fn, _ in rows.values():
            for _ in range(2):
                fn()
        got = {k: [] for k in rows}
        for _ in range(windows):
            for k, (fn, reps) in rows.items():
                got[k].append(window(fn, reps))
        return {k: (sorted(v)[len(v) // 2], max(v) - min(v)) for k, v in got.items()}

    many = 1024 if args.quick else 16384
    say(f"{args.reps} calls a window ({max(2, args.reps // 20)} of the rollout), median of 3 windows and their spread (max - min); greedy play, max_depth 252")
    for S, T, K, L, H in ((4, 2, 2, 256, 16), (4, 2, 2, 256, 64), (4, 2, 2, many, 16), (4, 2, 2, many, 64), (5, 2, 3, 256, 16)):
        C_ = S * S
        states = C_ ** T
        env = VecTilerSliderEnv.from_seeds(np.arange(L, dtype=np.int64), size=S, num_tiles=T, num_obstacles=K, obs_dtype=None, device=dev)
        D = env.onehot_channels * C_
        g = torch.Generator(device="cpu").manual_seed(1000 + H)
        policy = MlpPolicy(*(torch.randn(s, generator=g).to(dev) for s in ((H, D), (H,), (4, H), (4,))))
        table = env.build_table()
        pt = env.build_policy_table(policy)
        score = env.score_policy(pt, table)
        # one board per valid placement, standing on it
        level, idx = torch.nonzero(pt.act != 255, as_tuple=True)
        cells = torch.stack([(idx // C_ ** t) % C_ for t in range(T)]).to(torch.uint8)
        boards = VecTilerSliderEnv.from_arrays(S, env._blk[:, level].contiguous(), cells.contiguous(), env._tgt[:, level].contiguous(),
                                               multi_color=env.multi_color, max_steps=1 << 20, obs_dtype=None, device=dev)
        n = boards.num_envs

        def composed():
            boards.reset()
            return boards.rollout_policy(252, policy, select="greedy", epsilon=0.0, stats=("first_win",))

        first = composed().first_win
        d = pt.dist[level, idx].int()
        away = d != 0  # a board that starts on a won placement is not done: its first move may un-win it
        agree = bool(torch.where((d >= 1) & (d <= 252), d, torch.zeros_like(d))[away].eq(first[away]).all())
        lib = xc.lib()
        import ctypes as C
        st, dims = C.byref(env._state), C.byref(env._dims)
        mlp = policy._mlp(env)
        stream = torch.cuda.current_stream(dev).cuda_stream
        act, dist = pt.act, torch.empty_like(pt.dist)
        rows = {"build_policy_table": (lambda: env.build_policy_table(policy), args.reps),
                "ts_ptable_actions": (lambda: lib.ts_ptable_actions(dims, st, C.byref(mlp), act.data_ptr(), None, stream), args.reps),
                "ts_ptable_walk": (lambda: lib.ts_ptable_walk(dims, st, act.data_ptr(), 252, dist.data_ptr(), stream), args.reps),
                "score_policy": (lambda: env.score_policy(pt, table), args.reps),
                "policy_logits": (lambda: boards.policy_logits(policy), args.reps),
                "rollout": (composed, max(2, args.reps // 20))}
        res = time_rows(rows)
        da, dw, ds = xc.describe_ptable_actions(env._dims, H), xc.describe_ptable_walk(env._dims), xc.describe_ptable_score(env._dims)
        say(f"{L} levels of {S}x{S} / {T} tiles ({states} placements a level, {n} valid in all), H = {H}: {da['name']} {da['blocks']} blocks of "
            f"{da['threads_per_block']}, {dw['name']} {dw['blocks']} blocks, {ds['name']} {ds['lanes_per_level']} lanes a level")
        say(f"    solved {float(score.solved_share):.3f}  optimal {float(score.optimal_share):.3f}  agreement {float(score.agreement):.3f} of the solvable "
            f"placements; longest win {int(pt.dist[pt.dist <= 252].max())} moves; the rollout's first_win is the table's distance: {agree}")
        for k in ("build_policy_table", "ts_ptable_actions", "ts_ptable_walk", "score_policy", "policy_logits", "rollout"):
            say(f"    {k:20s} {res[k][0]:12.1f} us   (spread {res[k][1]:.1f})")
        new, old = res["build_policy_table"], res["rollout"]
        say(f"    the rollout over build_policy_table: x{old[0] / new[0]:.0f}; faster by more than the spreads: {old[0] - old[1] > new[0] + new[1]}")
        say(f"    per placement: ts_ptable_actions {1e3 * res['ts_ptable_actions'][0] / (L * states):.3f} ns (all {L * states}), policy_logits "
            f"{1e3 * res['policy_logits'][0] / n:.3f} ns per board ({n} boards); ts_ptable_walk reads {L * states} action bytes and writes as many: "
            f"{2 * L * states / res['ts_ptable_walk'][0] / 1e6:.3f} TB/s")
        del env, boards, pt, table
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
