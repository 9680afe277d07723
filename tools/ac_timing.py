#!/usr/bin/env python3
"""Times the actor-critic network (include/tiler_slider_ac.h) against the two-network pair it replaces, on one GPU: HIP events
around the launches after warm-up.

    python tools/ac_timing.py [--log FILE] [--launches 20] [--quick]

Per shape, H = 16 and 64 hidden units, K = 16 and 100 logged steps, in one process and one run, on the trajectory of a
rollout_policy(K, ..., log=("start", "pos")) of an observation-less auto-reset actor with Gaussian weights, a Gaussian dz and a
Gaussian dv:

    ac fwd       one ts_ac_forward over all K * N logged board-steps: logits and values
    ac bwd       one ts_ac_backward taking dz and dv (the six gradient buffers are not zeroed inside the timed region)
    pair fwd     what an actor and a separate critic PolicyNet launch for the same outputs: ts_train_forward twice
    pair bwd     ts_train_backward twice, the critic's with a dz that is dv in column 0 and zero in the other three

The pair is the training library as it stands in the tree: the code under test is never its own baseline.  Before a row is
timed the two sides are compared: the logits bit for bit, the actor's four gradients with dv = 0 to 1e-3 of their scale (a sanity
check of what is about to be timed; the tests hold the rigorous bound).  Launches of K = 100 rows are a quarter of --launches.
profiles/ac_timing.log is where a run of this script belongs; run it under `timeout`.
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
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the boards, K = 16 only")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import ActorCriticNet, PolicyNet, VecTilerSliderEnv
    from tiler_slider_amd import _ac_cabi as ac
    from tiler_slider_amd import _train_cabi as tc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.log:  # rewritten at every line: what was measured survives a run that ends early
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            open(args.log, "w").write("\n".join(lines) + "\n")

    LA, LT = ac.lib(), tc.lib()
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

    def run(label, S, T, Ko, mc, n, levels):
        env = VecTilerSliderEnv.from_seeds(np.arange(n, dtype=np.int64) % levels, size=S, num_tiles=T, num_obstacles=Ko, multi_color=mc, obs_dtype=None,
                                           device=dev, max_steps=20, auto_reset=True)
        env.reset()
        D = env.onehot_channels * S * S
        say(f"{label}: {n} boards, {D} features")
        for H in (16, 64):
            gen = torch.Generator(device=dev)
            gen.manual_seed(H)
            net, critic = ActorCriticNet(D, H, dev, generator=gen), PolicyNet(D, H, dev, generator=gen)
            with torch.no_grad():
                for p in list(net.parameters()) + list(critic.parameters()):
                    p.copy_(torch.randn(p.shape, device=dev, generator=gen))
            for steps in ((16,) if args.quick else (16, 100)):
                launches = args.launches if steps <= 16 else max(3, args.launches // 4)
                env.reset()
                out = env.rollout_policy(steps, net.policy(), select="sample", seed=0x7131, stats=False, log=("start", "pos"))
                dz = torch.randn((steps, n, 4), device=dev, generator=gen)
                dv = torch.randn((steps, n), device=dev, generator=gen)
                dz_critic = torch.zeros_like(dz)
                dz_critic[..., 0] = dv
                logits, values = torch.empty_like(dz), torch.empty_like(dv)
                logits_a, logits_c = torch.empty_like(dz), torch.empty_like(dz)
                params = (net.w1, net.b1, net.w2, net.b2, net.wv, net.bv)
                g_ac = [torch.zeros_like(p) for p in params]
                g_actor, g_critic = [torch.zeros_like(p) for p in params[:4]], [torch.zeros_like(p) for p in params[:4]]
                mlp, mlp_c = net.policy()._mlp(env), critic.policy()._mlp(env)
                head = ac.ValueHead(net.wv.data_ptr(), net.bv.data_ptr())
                tin = tc.TrainIn(out.start_pos.data_ptr(), out.pos_log.data_ptr(), steps, 0)
                grad, hgrad = tc.MlpGrad(*(g.data_ptr() for g in g_ac[:4])), ac.ValueHeadGrad(g_ac[4].data_ptr(), g_ac[5].data_ptr())
                grad_a, grad_c = tc.MlpGrad(*(g.data_ptr() for g in g_actor)), tc.MlpGrad(*(g.data_ptr() for g in g_critic))
                d, st = C.byref(env._dims), C.byref(env._state)

                def ac_fwd():
                    ac.check(LA.ts_ac_forward(d, st, C.byref(mlp), C.byref(head), C.byref(tin), logits.data_ptr(), values.data_ptr(), stream()), "ts_ac_forward")

                def ac_bwd(dvalues=dv):
                    ac.check(LA.ts_ac_backward(d, st, C.byref(mlp), C.byref(head), C.byref(tin), dz.data_ptr(), dvalues.data_ptr(), C.byref(grad),
                                               C.byref(hgrad), stream()), "ts_ac_backward")

                def pair_fwd():
                    tc.check(LT.ts_train_forward(d, st, C.byref(mlp), C.byref(tin), logits_a.data_ptr(), stream()), "ts_train_forward")
                    tc.check(LT.ts_train_forward(d, st, C.byref(mlp_c), C.byref(tin), logits_c.data_ptr(), stream()), "ts_train_forward")

                def pair_bwd():
                    tc.check(LT.ts_train_backward(d, st, C.byref(mlp), C.byref(tin), dz.data_ptr(), C.byref(grad_a), stream()), "ts_train_backward")
                    tc.check(LT.ts_train_backward(d, st, C.byref(mlp_c), C.byref(tin), dz_critic.data_ptr(), C.byref(grad_c), stream()), "ts_train_backward")

                # a sanity check of the two sides: the actor part of the new calls is the training library's
                ac_fwd()
                pair_fwd()
                assert torch.equal(logits, logits_a), (label, H, steps, "logits")
                ac_bwd(torch.zeros_like(dv))
                tc.check(LT.ts_train_backward(d, st, C.byref(mlp), C.byref(tin), dz.data_ptr(), C.byref(grad_a), stream()), "ts_train_backward")
                for a, b in zip(g_ac[:4], g_actor):
                    assert float((a - b).abs().max()) <= 1e-3 * max(1.0, float(b.abs().max())), (label, H, steps, tuple(a.shape))
                assert not bool(g_ac[4].any()) and not bool(g_ac[5].any())
                t_af, t_ab = time_us(ac_fwd, launches), time_us(ac_bwd, launches)
                t_pf, t_pb = time_us(pair_fwd, launches), time_us(pair_bwd, launches)
                torch.cuda.synchronize()
                df, db = ac.describe_ac_forward(env._dims, H, steps), ac.describe_ac_backward(env._dims, H, steps)
                pb = tc.describe_train_backward(env._dims, H, steps)
                say(f"    H {H:>2} K {steps:>3} ac fwd {df['threads_per_block']:>3} thr {df['lds_bytes']:>5} B w{df['weights_in_lds']}; ac bwd {db['blocks']:>4} blocks "
                    f"{db['lds_bytes']:>5} B w{db['weights_in_lds']} g{db['grads_in_lds']} (train bwd {pb['blocks']:>4} blocks {pb['lds_bytes']:>5} B "
                    f"w{pb['weights_in_lds']} g{pb['grads_in_lds']})  ac fwd {t_af:9.1f} us  pair fwd {t_pf:9.1f} us  ratio {t_af / t_pf:5.2f}  "
                    f"ac bwd {t_ab:9.1f} us  pair bwd {t_pb:9.1f} us  ratio {t_ab / t_pb:5.2f}  "
                    f"ac f+b / pair f+b {(t_af + t_ab) / (t_pf + t_pb):5.2f}")
                del out, dz, dv, dz_critic, logits, values, logits_a, logits_c
        del env
        torch.cuda.empty_cache()

    shrink = 4 if args.quick else 0
    for label, S, T, Ko, mc, n, levels in (("4x4 / 2 tiles (cfg1)", 4, 2, 2, False, 1 << 20, 1 << 16), ("4x4 / 2 tiles (cfg1), small batch", 4, 2, 2, False, 4096, 4096),
                                           ("5x5 / 3 tiles, multi colour", 5, 3, 3, True, 1 << 18, 4096)):
        n = max(n >> shrink, 4096)
        run(label, S, T, Ko, mc, n, min(levels, n))


if __name__ == "__main__":
    main()
