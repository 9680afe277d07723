#!/usr/bin/env python3
"""Times the trajectory targets (include/tiler_slider_targets.h) on one GPU: HIP events around the launches after warm-up.

    python tools/targets_timing.py [--log FILE] [--launches 50] [--baseline-launches 5] [--quick] [--no-graph]

Per shape and K = 16 and 100 logged steps, in one process and one run, on the log of a table-policy rollout (epsilon 0.3,
auto-reset, max_steps 20, start, cells and flags logged) with Gaussian values:

    fused returns   one ts_traj_returns: every weight set (so the cells are read), values and last_value given, four outputs
    fused labels    one ts_traj_labels: three outputs
    loop returns    what a user writes without the library: K x (a twin's cells set from the log + env.reward()) and once more for
                    the start, the reward terms from the flag bits in torch, then the backward recursion as K rounds of
                    element-wise torch over [N]
    loop labels     K x (a twin's cells set from the log + lookup_bits + expert_actions_from)
    graph ...       each loop captured into one graph and replayed ("-" with --no-graph).  Any failure of a capture or a replay
                    ENDS the run after the log is written - the error of a refused capture cannot be told from a GPU fault, and
                    nothing more may be launched after one: run again with --no-graph

Before a row is timed the two sides are compared: labels byte for byte, returns to 1e-4 of their scale (a sanity check of what
is about to be timed; the tests hold the rigorous bound).  The fused calls' algorithmic bytes (bytes_read + bytes_written of the
describe calls) over their time are shown beside a sustainable HBM rate of 6.3 TB/s.  profiles/targets_timing.log is where a
run of this script belongs; run it under `timeout`.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_US = 6.3e6  # 6.3 TB/s: what a float4 copy achieves of the 8 TB/s peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--baseline-launches", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the boards, K = 16 only")
    ap.add_argument("--no-graph", action="store_true", help="do not capture the loops into graphs")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import RewardWeights, VecTilerSliderEnv, _cabi
    from tiler_slider_amd import _targets_cabi as gc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.log:  # rewritten at every line: what was measured survives a run that ends early
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            open(args.log, "w").write("\n".join(lines) + "\n")

    dev = torch.device("cuda", 0)
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

    def graphed(fn):
        """us per replay of fn captured into one graph; None with --no-graph; a failure ends the run."""
        if args.no_graph:
            return None
        try:
            torch.cuda.synchronize()
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):
                    fn()
            t = time_us(graph.replay, args.baseline_launches)
            del graph
            return t
        except Exception as e:
            say(f"        graph capture or replay of a loop failed ({type(e).__name__}: {e}); the run ends here: use --no-graph")
            raise SystemExit(3)

    def make(S, T, Ko, mc, seeds):
        env = VecTilerSliderEnv.from_seeds(seeds, size=S, num_tiles=T, num_obstacles=Ko, multi_color=mc, obs_dtype=None, device=dev, max_steps=20,
                                           auto_reset=True)
        env.reset()
        return env

    w = RewardWeights(step=-0.01, win=1.0, timeout=-0.5, invalid=-0.1, dist=0.05, progress=0.25)
    gamma, lam = 0.97, 0.9
    VOID = _cabi.FLAG_STEPPED_DONE | _cabi.FLAG_AUTORESET | _cabi.FLAG_BAD_ACTION
    END = _cabi.FLAG_SUCCESS | _cabi.FLAG_TIMEOUT

    def run(label, S, T, Ko, mc, n, levels):
        seeds = np.arange(n, dtype=np.int64) % levels
        env, twin = make(S, T, Ko, mc, seeds), make(S, T, Ko, mc, seeds)
        table = make(S, T, Ko, mc, np.arange(levels, dtype=np.int64)).build_table()
        rows = torch.from_numpy(seeds.astype(np.int32)).to(dev)
        say(f"{label}: {n} boards on {levels} levels")
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        for steps in ((16,) if args.quick else (16, 100)):
            env.reset()
            out = env.rollout(steps, "table", table=table, rows=rows, epsilon=0.3, seed=0x7A26, stats=False, log=("start", "pos", "flags"))
            V, VL = torch.randn((steps, n), device=dev, generator=gen), torch.randn(n, device=dev, generator=gen)
            cells = lambda k: out.start_pos if k == 0 else out.pos_log[k - 1]
            fused_returns = lambda: env.trajectory_returns(out, gamma, lam, V, VL, w)
            fused_labels = lambda: env.trajectory_labels(out, table, rows)
            m = torch.empty((steps + 1, n), dtype=torch.int32, device=dev)
            res = {}

            def loop_returns():
                for k in range(steps + 1):      # m(c[0]), then m(pos_log[k])
                    twin._pos.copy_(cells(k) if k < steps else out.pos_log[steps - 1])
                    twin.reward(out=m[k])
                f = out.flags_log
                mf = m.float()
                r = (w.step + w.win * ((f & _cabi.FLAG_SUCCESS) != 0) + w.timeout * ((f & _cabi.FLAG_TIMEOUT) != 0)
                     + w.invalid * ((f & _cabi.FLAG_INVALID_MOVE) != 0) + w.dist * mf[1:] + w.progress * (mf[1:] - mf[:-1]))
                void, end = (f & VOID) != 0, (f & END) != 0
                adv, carry = torch.zeros_like(r), torch.zeros(n, device=dev)
                for k in range(steps - 1, -1, -1):
                    vplus = torch.where(end[k], 0.0, VL if k == steps - 1 else V[k + 1])
                    a = r[k] + gamma * vplus - V[k] + torch.where(end[k], 0.0, gamma * lam * carry)
                    carry = torch.where(void[k], carry, a)
                    adv[k] = torch.where(void[k], 0.0, a)
                res["reward"], res["adv"], res["ret"], res["mask"] = torch.where(void, 0.0, r), adv, torch.where(void, 0.0, adv + V), ~void

            lm = torch.empty((steps, n), dtype=torch.int16, device=dev)
            lb, la = torch.empty((steps, n), dtype=torch.uint8, device=dev), torch.empty((steps, n), dtype=torch.uint8, device=dev)

            def loop_labels():
                for k in range(steps):
                    twin._pos.copy_(cells(k))
                    mv, bs = twin.lookup_bits(table, rows)
                    lm[k], lb[k], la[k] = mv, bs, twin.expert_actions_from(table, rows)

            # the two sides agree
            got, lab = fused_returns(), fused_labels()
            loop_returns()
            loop_labels()
            assert torch.equal(got.mask, res["mask"]), (label, steps, "mask")
            for key in ("reward", "adv", "ret"):
                a, b = getattr(got, key), res[key]
                assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max())), (label, steps, key)
            assert torch.equal(lab[0], lm) and torch.equal(lab[1], lb) and torch.equal(lab[2], la), (label, steps, "labels")
            what_r = 0xff
            dr, dl = gc.describe_traj_returns(env._dims, steps, what_r), gc.describe_traj_labels(env._dims, steps)
            t_r, t_l = time_us(fused_returns, args.launches), time_us(fused_labels, args.launches)
            t_lr, t_ll = time_us(loop_returns, args.baseline_launches), time_us(loop_labels, args.baseline_launches)
            t_gr, t_gl = graphed(loop_returns), graphed(loop_labels)
            us = lambda t: f"{t:10.1f} us" if t is not None else "         -"
            ratio = lambda t, f: f"{t / f:7.1f}" if t is not None else "      -"
            for name, d, t, tl, tg in (("returns", dr, t_r, t_lr, t_gr), ("labels ", dl, t_l, t_ll, t_gl)):
                nbytes = d["bytes_read"] + d["bytes_written"]
                say(f"    K {steps:>3} {name} {d['name']:<18} {d['blocks']:>5} blocks  fused {t:9.1f} us  loop {us(tl)}  graph {us(tg)}  "
                    f"loop / fused {ratio(tl, t)}  graph / fused {ratio(tg, t)}  {nbytes / 1e6:8.1f} MB = {nbytes / t / 1e6:5.2f} TB/s "
                    f"({100 * nbytes / t / HBM_BYTES_PER_US:4.1f} % of 6.3 TB/s; {nbytes / HBM_BYTES_PER_US:7.1f} us at that rate)")
            del out, V, VL, m, lm, lb, la, res
        del env, twin, table
        torch.cuda.empty_cache()

    shrink = 4 if args.quick else 0
    for label, S, T, Ko, mc, n, levels in (("4x4 / 2 tiles (cfg1)", 4, 2, 2, False, 1 << 20, 1 << 16), ("4x4 / 2 tiles (cfg1), small batch", 4, 2, 2, False, 4096, 4096),
                                           ("5x5 / 3 tiles, multi colour", 5, 3, 3, True, 1 << 18, 4096)):
        n = max(n >> shrink, 4096)
        run(label, S, T, Ko, mc, n, min(levels, n))


if __name__ == "__main__":
    main()
