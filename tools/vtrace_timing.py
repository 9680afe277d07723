#!/usr/bin/env python3
"""Times the V-trace targets (include/tiler_slider_vtrace.h) against what they replace, on one GPU: HIP events around the calls
after warm-up, every baseline timed before AND after the fused call inside this one command.

    python tools/vtrace_timing.py [--log FILE] [--launches 5] [--quick]

Shapes: 1,048,576 4x4 boards of two tiles, K = 32 and 100; 65,536 5x5 boards of two tiles, K = 32 and 100; 4,096 4x4 boards,
K = 100.  The logs are those of a real mixed rollout - rollout_policy(expert=table, beta=0.5, epsilon=0.1, select="sample",
log=("flags", "act", "logits", "expert")) of a 16-unit network in auto-reset mode, max_steps 30 -, the target policy's logits are
the logged ones plus N(0, 1/4), the values Gaussian.  gamma = 0.97, lambda = 0.9, both bars 1, the default reward (1 for a win:
no cells are read).

    fused            one trajectory_vtrace(): all six outputs
    fused, pi = mu   the same with logits=None: one logits row a step less to read
    (a) torch        what it replaces: two log_softmax, gather, the mix, the ratio, the clamps, and the K-step backward loop of
                     torch.where over [N]; eager, and - if the capture works - replayed from a torch.cuda.graph
    (b) returns      trajectory_returns() alone on the same log: the on-policy launch, which reads 5 bytes a sample where the
                     fused call reads 39 and writes 13 where it writes 21 - the floor

The describe call's algorithmic bytes over the fused call's time are set against 6.3 TB/s.  The larger relative spread of a
before / after pair is the margin within which a ratio is read.  profiles/vtrace_timing.log is where a run of this script belongs
(DESIGN.md section 32); run it under `timeout`.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAMMA, LAM, EPS, BETA, PEAK = 0.97, 0.9, 0.1, 0.5, 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the boards, K = 8")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import PolicyNet, VecTilerSliderEnv
    from tiler_slider_amd import _vtrace_cabi as vc

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

    def torch_vtrace(flags, act, expert, mu_logits, pi_logits, V, VL, out):
        """The torch code the fused call replaces; writes reward, adv, ret, weight, log_mu, mask into `out`."""
        K = flags.shape[0]
        a = act.clamp(max=3).long().unsqueeze(-1)
        lp_mu = torch.log_softmax(mu_logits, -1).gather(-1, a).squeeze(-1)
        lp_pi = torch.log_softmax(pi_logits, -1).gather(-1, a).squeeze(-1)
        pe = lp_mu.exp()
        inner = torch.where(expert != 255, BETA * (act == expert).float() + (1.0 - BETA) * pe, pe)
        mu = EPS / 4 + (1.0 - EPS) * inner
        w = lp_pi.exp() / mu
        rho, c = w.clamp(max=1.0), LAM * w.clamp(max=1.0)
        void, end = (flags & 0x70) != 0, (flags & 0x0c) != 0
        r = ((flags & 0x04) != 0).float()
        zero = torch.zeros_like(VL)
        carry, vnext = zero, VL
        for k in range(K - 1, -1, -1):
            vplus = torch.where(end[k], zero, vnext)
            delta = rho[k] * (r[k] + GAMMA * vplus - V[k])
            d = torch.where(end[k], delta, delta + GAMMA * c[k] * carry)
            adv = torch.where(end[k], delta, rho[k] * (r[k] + GAMMA * (vplus + carry) - V[k]))
            out["adv"][k] = torch.where(void[k], zero, adv)
            out["ret"][k] = torch.where(void[k], zero, V[k] + d)
            carry, vnext = torch.where(void[k], carry, d), V[k]
        live = ~void
        out["reward"].copy_(r * live)
        out["weight"].copy_(w * live)
        out["log_mu"].copy_(mu.log() * live)
        out["mask"].copy_(live)

    shrink = 16 if args.quick else 1
    shapes = (((1 << 20) // shrink, 4, (32, 100)), ((1 << 16) // shrink, 5, (32, 100)), (4096 // shrink, 4, (100,)))
    say(f"gamma {GAMMA}, lambda {LAM}, rho_bar = c_bar = 1, epsilon {EPS}, beta {BETA}, select sample; {args.launches} launches a timing; nothing here was known in advance")
    for n, S, Ks in shapes:
        env = VecTilerSliderEnv.from_seeds(np.arange(n, dtype=np.int64), size=S, num_tiles=2, num_obstacles=2, multi_color=False, obs_dtype=None, device=dev,
                                           max_steps=30, auto_reset=True)
        env.reset()
        table = env.build_table()
        net = PolicyNet(env.onehot_channels * S * S, 16, dev, generator=torch.Generator(device=dev).manual_seed(16))
        say(f"{n} {S}x{S} boards of two tiles")
        for K in ((8,) if args.quick else Ks):
            roll = env.rollout_policy(K, net.policy(), select="sample", epsilon=EPS, seed=0x57ACE, stats=False, log=("flags", "act", "logits", "expert"),
                                      expert=table, beta=BETA)
            gen = torch.Generator(device=dev).manual_seed(K)
            pi = roll.logits_log + 0.5 * torch.randn(roll.logits_log.shape, device=dev, generator=gen)
            V, VL = torch.randn((K, n), device=dev, generator=gen), torch.randn(n, device=dev, generator=gen)
            kw = dict(gamma=GAMMA, lam=LAM, select="sample", epsilon=EPS, beta=BETA)
            fused = lambda: env.trajectory_vtrace(roll, pi, V, VL, **kw)
            fused_mu = lambda: env.trajectory_vtrace(roll, None, V, VL, **kw)
            returns = lambda: env.trajectory_returns(roll, GAMMA, LAM, V, VL)
            out = {k: torch.empty((K, n), dtype=torch.float32, device=dev) for k in ("reward", "adv", "ret", "weight", "log_mu")}
            out["mask"] = torch.empty((K, n), dtype=torch.bool, device=dev)
            eager = lambda: torch_vtrace(roll.flags_log, roll.act_log, roll.expert_log, roll.logits_log, pi, V, VL, out)
            # the two sides compute the same thing
            vt = fused()
            eager()
            torch.cuda.synchronize()
            worst = max(float((getattr(vt, k) - out[k]).abs().max()) for k in ("reward", "adv", "ret", "weight", "log_mu"))
            assert torch.equal(vt.mask, out["mask"]) and worst < 1e-3, worst
            what = vc.OUT_ALL | vc.IN_VALUES | vc.IN_LAST_VALUE | vc.IN_EXPERT | vc.IN_PI
            d, d_mu = vc.describe_traj_vtrace(env._dims, K, what), vc.describe_traj_vtrace(env._dims, K, what & ~vc.IN_PI)
            say(f"  K {K:>3}  {d['name']}  {d['blocks']} blocks of {d['threads_per_block']}, chunk {d['chunk_steps']}; live {float(vt.mask.float().mean()):.2f}, "
                f"w > 1 on {float((vt.weight[vt.mask] > 1).float().mean()):.2f}; torch and fused differ by at most {worst:.1e}")
            t_e1 = time_us(eager, 1)
            t_r1 = time_us(returns, args.launches)
            t_f = time_us(fused, args.launches)
            t_m = time_us(fused_mu, args.launches)
            t_r2 = time_us(returns, args.launches)
            t_e2 = time_us(eager, 1)
            t_g1 = t_g2 = t_f2 = float("nan")
            try:
                torch.cuda.synchronize()
                graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
                with torch.cuda.stream(side):
                    with torch.cuda.graph(graph, stream=side):
                        eager()
                t_g1 = time_us(graph.replay, args.launches)
                t_f2 = time_us(fused, args.launches)
                t_g2 = time_us(graph.replay, args.launches)
                del graph
            except Exception as e:  # the capture is a convenience of the baseline, not a part of the measurement
                say(f"    (graph capture of the torch code failed: {type(e).__name__})")
            nan_min = lambda *t: min(x for x in t if x == x)
            nan_max = lambda *t: max(x for x in t if x == x)
            spread = max(abs(t_e1 - t_e2) / min(t_e1, t_e2), abs(t_r1 - t_r2) / min(t_r1, t_r2), abs(t_g1 - t_g2) / min(t_g1, t_g2) if t_g1 == t_g1 else 0.0)
            slow = nan_max(t_f, t_f2)
            algo = d["bytes_read"] + d["bytes_written"]
            say(f"    fused {t_f:9.1f} / {t_f2:9.1f} us   fused, pi = mu {t_m:9.1f} us   (a) torch eager {t_e1:10.1f} / {t_e2:10.1f} us   torch, graph {t_g1:10.1f} / {t_g2:10.1f} us   "
                f"(b) returns {t_r1:8.1f} / {t_r2:8.1f} us   spread {100 * spread:4.1f} %")
            say(f"    fastest torch / slowest fused {nan_min(t_e1, t_e2, t_g1, t_g2) / slow:6.2f}   slowest fused / (b) returns {slow / min(t_r1, t_r2):5.2f}   "
                f"{algo / 2**20:.0f} MiB algorithmic: {algo / (slow * 1e-6) / 1e12:.2f} TB/s, {100 * algo / (slow * 1e-6) / PEAK:.0f} % of 6.3 TB/s   "
                f"(pi = mu: {(d_mu['bytes_read'] + d_mu['bytes_written']) / (t_m * 1e-6) / 1e12:.2f} TB/s)   {slow * 1e3 / (n * K):.4f} ns per sample")
            del roll, pi, V, VL, out, vt
            torch.cuda.empty_cache()
        del env, table
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
