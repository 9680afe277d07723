#!/usr/bin/env python3
"""Target of a counter-only `rocprofv3 --pmc` pass (or of a `--kernel-trace --stats` run of its own) over the in-place step:
tools/update_ab.py's environment of one shape - bench.py's LEVEL_SEED and ACTION_SEED, multi colour, auto-reset, max_steps 2**30,
obs_update="inplace" - a reset and 60 steps.  profiles/update_requests.md takes the mean over launches 20 to 60.

    rocprofv3 --pmc COUNTER [COUNTER ...] --output-format csv -d DIR -- python tools/update_pmc_target.py [--shape cfg1_1m] [--library FILE]

--library FILE steps with another build of libtiler_slider_update.so (the parent commit's, a -D variant of build/variants/)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import update_ab
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="cfg1_1m", choices=sorted(update_ab.SHAPES))
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--library", default=None)
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import VecTilerSliderEnv, _cabi, _update_cabi
    if args.library:
        _update_cabi.LIB_PATH = os.path.abspath(args.library)  # before the first lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    S, T, K, n = update_ab.SHAPES[args.shape]
    env = VecTilerSliderEnv.random(n, size=S, num_tiles=T, num_obstacles=K, seed=update_ab.LEVEL_SEED, multi_color=True,
                                   max_steps=2**30, device=dev, auto_reset=True, obs_update="inplace")
    stream = torch.cuda.current_stream(dev).cuda_stream
    ring = []
    for i in range(16):
        a = torch.empty(n, dtype=torch.uint8, device=dev)
        _cabi.check(_cabi.lib().ts_fill_actions(n, update_ab.ACTION_SEED, 0, i, a.data_ptr(), stream), "ts_fill_actions")
        ring.append(a)
    env.reset()
    for i in range(args.steps):
        env.step_async(ring[i & 15])
    torch.cuda.synchronize(dev)
    print(f"{args.shape}: {args.steps} steps of {_cabi.describe_launch(env._dims, _cabi.OP_STEP, _cabi.OUT_OBS)['name']} "
          f"with {os.path.relpath(_update_cabi.LIB_PATH, ROOT)}")


if __name__ == "__main__":
    main()
