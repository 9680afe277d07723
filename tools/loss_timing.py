#!/usr/bin/env python3
"""Times the fused actor-critic loss (include/tiler_slider_loss.h) against the plain-torch loss it offers to replace, on one GPU:
HIP events around 50 calls after 2 warm-up calls, one process.

    python tools/loss_timing.py [--log FILE] [--calls 50] [--quick]

Shapes: the samples of cfg1's logged trajectories, M = K * N for N = 1,048,576 and 4,096 boards and K = 16 and 100 steps - the
loss knows no board, so Gaussian logits, values, returns and advantages, uniform actions and a mask that voids a tenth of the
samples stand in for a rollout.  Modes: A2C (advantage, value term, entropy 0) and PPO (the same with the ratio to old logits
0.1 away, clip 0.2).  Compared, from `logits` and `values` to their gradients:

    fused        one ts_actor_critic_loss: four launches, the raw call (actor_critic_loss_grads' C call on preallocated buffers)
    torch eager  the README's loss - log_softmax, gather, the mask, the sums - and torch.autograd.grad of it; PPO's as a user
                 writes it (exp of the difference, clamp, minimum)
    torch graph  the same, captured once in a torch.cuda.CUDAGraph and replayed

The torch loss is the code of the README as it stood before the fused loss: the code under test is never its own baseline.
Before a row is timed the two sides are compared: the loss to 1e-4 of its size and dlogits to 1e-3 of the largest entry on all
but a millionth of the entries, or eight (PPO samples at the clip's edge may take the other side; the tests hold the rigorous
bound).
The last column sets ts_describe_loss' algorithmic bytes over the fused time beside the 6.3 TB/s the HBM is measured at.
profiles/loss_timing.log is where a run of this script belongs; run it under `timeout`.
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the large batch, K = 16 only")
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import _loss_cabi as lc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.log:  # rewritten at every line: what was measured survives a run that ends early
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            open(args.log, "w").write("\n".join(lines) + "\n")

    L = lc.lib()
    dev = torch.device("cuda", 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def time_us(fn, calls, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls

    say(f"fused actor-critic loss against the plain-torch loss: us per call, {args.calls} calls after 2 warm-up calls, HIP events")
    for n in ((1 << 16) if args.quick else (1 << 20), 4096):
        for K in ((16,) if args.quick else (16, 100)):
            M = K * n
            gen = torch.Generator(device=dev)
            gen.manual_seed(K)
            z = torch.randn((K, n, 4), device=dev, generator=gen)
            old = z + 0.1 * torch.randn((K, n, 4), device=dev, generator=gen)
            act = torch.randint(0, 4, (K, n), device=dev, generator=gen, dtype=torch.uint8)
            mask = torch.rand((K, n), device=dev, generator=gen) >= 0.1
            adv, v, ret = (torch.randn((K, n), device=dev, generator=gen) for _ in range(3))
            dz, dv = torch.empty_like(z), torch.empty_like(v)
            scalars = torch.empty(8, device=dev)
            ws = torch.empty(lc.workspace_bytes(M), dtype=torch.uint8, device=dev)
            mask8 = mask.view(torch.uint8)
            for mode in ("A2C", "PPO"):
                ppo = mode == "PPO"
                clip = 0.2 if ppo else 0.0
                lin = lc.LossIn(z.data_ptr(), old.data_ptr() if ppo else None, act.data_ptr(), mask8.data_ptr(), adv.data_ptr(), v.data_ptr(),
                                ret.data_ptr(), M, clip, 0.5, 0.0, 0)
                lout = lc.LossOut(dz.data_ptr(), dv.data_ptr(), scalars.data_ptr(), ws.data_ptr())

                def fused():
                    lc.check(L.ts_actor_critic_loss(C.byref(lin), C.byref(lout), torch.cuda.current_stream(dev).cuda_stream), "ts_actor_critic_loss")

                zt, vt = z.clone().requires_grad_(True), v.clone().requires_grad_(True)

                def torch_loss():
                    logp = torch.log_softmax(zt, dim=2).gather(2, act.clamp(max=3).long().unsqueeze(2)).squeeze(2)
                    live = mask.float()
                    if ppo:
                        logp_old = torch.log_softmax(old, dim=2).gather(2, act.clamp(max=3).long().unsqueeze(2)).squeeze(2)
                        r = (logp - logp_old).exp()
                        policy = -torch.minimum(r * adv, r.clamp(1 - clip, 1 + clip) * adv)
                    else:
                        policy = -adv * logp
                    loss = ((policy * live).sum() + 0.5 * (((vt - ret) ** 2) * live).sum()) / live.sum()
                    return (loss,) + torch.autograd.grad(loss, (zt, vt))

                # the two sides agree
                fused()
                loss_t, gz, gv = torch_loss()
                top = float(gz.abs().max())
                assert abs(float(scalars[0]) - float(loss_t.detach())) <= 1e-4 * max(1.0, abs(float(loss_t.detach()))), (mode, M)
                apart = int(((dz - gz).abs() > 1e-3 * top).sum())
                assert apart <= max(8, 1e-6 * dz.numel()) and float((dv - gv).abs().max()) <= 1e-3 * float(gv.abs().max()), (mode, M, apart)
                del loss_t, gz, gv
                calls = args.calls if M <= (1 << 25) else max(5, args.calls // 5)
                t_f = time_us(fused, calls)
                t_e = time_us(torch_loss, calls)
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for _ in range(3):
                        torch_loss()
                torch.cuda.current_stream(dev).wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    kept = torch_loss()
                t_g = time_us(graph.replay, calls)
                torch.cuda.synchronize()
                d = lc.describe_loss(M, lc.VALUES | lc.ADV | lc.MASK | (lc.OLD_LOGITS if ppo else 0))
                moved = d["bytes_read"] + d["bytes_written"]
                say(f"{n:>8} boards K {K:>3} {mode}: {M:>10} samples, {d['blocks']:>4} blocks, {moved / 1e6:8.1f} MB  fused {t_f:9.1f} us  "
                    f"torch eager {t_e:9.1f} us ({t_e / t_f:5.1f}x)  torch graph {t_g:9.1f} us ({t_g / t_f:5.1f}x)  "
                    f"fused {moved / t_f / 1e6:5.2f} TB/s of {HBM_TBS}")
                del graph, kept, zt, vt
            del z, old, act, mask, adv, v, ret, dz, dv
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
