"""bench.py --dump-outputs: what the timed path computed in its last step, the same in every run with the same arguments
(the clock warm-up, whose step count varies, is followed by a reset and a fixed number of steps) and equal to the CPU
oracle's replay of the run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench(out_dir, *args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(out_dir)] + list(args)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _replay(oracle, config, n, steps, warmup, settle):
    """The oracle twin of bench.py's run: reset, the settle steps after the clock warm-up, W warm-up steps, K timed steps
    (actions ring[i & 15] in each)."""
    import bench
    cfg = bench.CONFIGS[config]
    blk, init, tgt = oracle.generate(cfg["size"], cfg["tiles"], cfg["tiles"], cfg["obstacles"], n, seed=bench.LEVEL_SEED)
    ref = oracle.OracleBatch(cfg["size"], True, 2**30, blk, init, tgt)
    ref.reset()
    acts = [oracle.fill_actions(n, seed=bench.ACTION_SEED, step_index=i) for i in range(16)]
    for i in list(range(settle)) + list(range(warmup)) + list(range(steps - 1)):
        ref.step(acts[i & 15], mode=oracle.MODE_AUTORESET, obs=False)
    out = ref.step(acts[(steps - 1) & 15], mode=oracle.MODE_AUTORESET, reward=cfg["reward"], onehot=cfg["onehot"])
    want = {"obs": out["obs"], "flags": out["flags"], "done": ref.done != 0, "step_count": ref.step_count, "positions": ref.pos.T}
    if cfg["reward"]:
        want["reward"] = out["reward"]
    if cfg["onehot"]:
        want["onehot"] = out["onehot"]
    return want


def _check(oracle, d, line, config, n, steps, warmup):
    want = _replay(oracle, config, n, steps, warmup, line["config"]["clock_warmup"].get("settle_steps", 0))
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in list(want) + ["boards"])
    idx = np.load(os.path.join(d, "boards.npy"))
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and idx[-1] < n
    idx = idx.astype(np.int64)
    for k, w in want.items():
        got = np.load(os.path.join(d, k + ".npy"))
        assert got.dtype in (np.float32, np.float64), k
        got = got.T if k == "positions" else got
        np.testing.assert_array_equal(got, w[idx].astype(got.dtype), err_msg=k)
    return len(idx)


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_and_match_the_oracle(oracle, tmp_path):
    args = ["--config", "cfg2", "--boards", "3000", "--steps", "7", "--warmup", "2", "--clock-warmup-ms", "30"]
    line = _bench(tmp_path / "a", *args)
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["config"]["boards_per_gpu"] == 3000
    assert "other_configs" not in line and "cpu_baseline" not in line  # a plain run: the headline figure alone
    _bench(tmp_path / "b", *args)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    for f in names:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f), err_msg=f)
    assert line["config"]["clock_warmup"]["settle_steps"] > 0
    assert _check(oracle, tmp_path / "a", line, "cfg2", 3000, 7, 2) == 3000  # every board: below the size budget


@pytest.mark.gpu
def test_bench_dump_outputs_sample_a_large_batch(oracle, tmp_path):
    """The BASELINE batch of cfg1 (1,048,576 boards): a fixed, seeded sample within the size budget."""
    import bench
    line = _bench(tmp_path, "--steps", "3", "--warmup", "1", "--clock-warmup-ms", "0")
    k = _check(oracle, tmp_path, line, "cfg1", 1 << 20, 3, 1)
    assert 0 < k < 1 << 20
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= bench.DUMP_BUDGET_BYTES + 4096 * 8
