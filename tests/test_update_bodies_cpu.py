"""The two bodies of the in-place step's kernels without a GPU: which boards take the straight-line one, what the code object of
k_step_update<4, 2, false> holds of each, how its rows are addressed, and the census tool behind profiles/update_requests.md."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from cabi_harness import _assert_build_goes_through_the_guard, _dims
from conftest import ROOT

FLAGSHIP = "k_step_update<4, 2, false>"


@pytest.fixture(scope="module")
def disassembly():
    """kernel name -> its instructions (mnemonic and operands), from the shipped code object."""
    from tiler_slider_amd import _update_cabi as uc
    from tiler_slider_amd import _vgpr_guard as guard
    with tempfile.TemporaryDirectory() as wd:
        co = guard.unbundle(uc.LIB_PATH, wd)
        dis = subprocess.run([f"{guard.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--demangle", co], check=True,
                             capture_output=True, text=True).stdout
    kernels, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = re.sub(r"^.*(k_step_update<[^>]*>).*$", r"\1", m.group(1)).replace("(anonymous namespace)::", "")
            kernels[name] = []
        elif name and line.strip() and not line.strip().startswith("//"):
            kernels[name].append(line.split("//")[0].strip())
    return kernels


def test_full_body_is_chosen_as_documented():
    """_update_cabi.full_body mirrors the kernel's uniform condition: T == Tt == 2 on a board of at least two cells, whatever the
    colour mode, the step mode, the reward and the observation type; never in an eight-tile kernel."""
    from tiler_slider_amd import _cabi, _update_cabi as uc
    for S in range(1, 9):
        for T in range(1, min(S * S, 8) + 1):
            for Tt in range(0, 9):
                for mc in (0, 1):
                    d = _dims(S, T, mc, 257, Tt=Tt)
                    name = uc.describe_step_update(d, _cabi.OUT_OBS)["name"]
                    assert uc.full_body(d) == (T == 2 and Tt == 2), (S, T, Tt)
                    if uc.full_body(d):
                        assert name == f"k_step_update<{S}, 2, false>", (S, T, Tt, name)
    src = open(uc.SRC).read()
    assert "if constexpr (TMAX == 2 && S * S >= TMAX)" in src and "if (a.T == TMAX && a.Tt == TMAX) return step_update_body<S, TMAX, U8, true>(a);" in src
    assert "step_update_body<S, TMAX, U8, false>(a);" in src


def test_the_flagship_kernel_holds_both_bodies(disassembly):
    """A body loads its board once: the obstacle word, the step counter, the done latch and the action, and per tile row the
    cell, the shown cell, the initial cell and the target.  That is 12 vector loads with two rows and 36 with eight; the
    two-tile kernels hold two bodies - 24 loads, four of them dwords - and the eight-tile kernels one."""
    loads = lambda k, what="global_load_": sum(1 for i in disassembly[k] if i.startswith(what))
    for u8 in ("false", "true"):
        assert loads(f"k_step_update<4, 2, {u8}>") == 2 * (4 + 4 * 2), u8
        assert loads(f"k_step_update<4, 2, {u8}>", "global_load_dword") == 2 * 2, u8
        assert loads(f"k_step_update<4, 8, {u8}>") == 4 + 4 * 8, u8
        assert loads(f"k_step_update<4, 8, {u8}>", "global_load_dword") == 2, u8


def test_rows_are_addressed_from_scalar_bases(disassembly):
    """No 64-bit vector multiply-add and no 64-bit vector add builds an address in either body of k_step_update<4, 2, false>:
    every load and store takes its base from a scalar register pair and a 32-bit offset from the lane."""
    text = disassembly[FLAGSHIP]
    assert not [i for i in text if "v_mad_u64_u32" in i]
    assert not [i for i in text if "v_lshl_add_u64" in i]
    memory = [i for i in text if i.startswith(("global_load_", "global_store_"))]
    assert len(memory) >= 40
    assert all(re.search(r"\bs\[\d+:\d+\]", i) and not re.search(r", off\b", i) for i in memory), [i for i in memory if re.search(r", off\b", i)][:4]
    # and in no kernel of the library is there a 64-bit multiply-add left
    assert not [k for k, t in disassembly.items() if any("v_mad_u64_u32" in i for i in t)]


def test_the_library_still_goes_through_the_guarded_build(monkeypatch):
    from tiler_slider_amd import _update_cabi as uc
    _assert_build_goes_through_the_guard(uc, monkeypatch)
    tool = open(os.path.join(ROOT, "tools", "update_ab.py")).read()
    assert "_cabi.compile_guarded(_update_cabi.SRC, variant" in tool and "--define" in tool and 'build", "variants"' in tool


def test_census_tool_against_a_direct_count(oracle):
    """tools/obs_delta_census.py at 4,096 boards, 64 settle steps, 8 steps, against a count made here from the oracle's own
    float32 observations: floats that differ between consecutive observations, the distinct 32 / 64 / 128-byte blocks of the
    buffer they lie in, boards with a difference, boards whose flags carry AUTORESET."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import obs_delta_census as census
    N, settle, steps = 4096, 64, 8
    got = census.census(oracle, 4, 2, 2, N, settle, steps)
    blk, init, tgt = oracle.generate(4, 2, 2, 2, N, seed=census.LEVEL_SEED)
    ref = oracle.OracleBatch(4, True, 2**30, blk, init, tgt)
    before = ref.reset()
    want = dict.fromkeys(census.QUANTITIES, 0)
    for k in range(settle + steps):
        out = ref.step(oracle.fill_actions(N, seed=census.ACTION_SEED, step_index=k & 15), mode=oracle.MODE_AUTORESET)
        after = out["obs"]
        if k >= settle:
            assert np.array_equal(after[..., 0], before[..., 0]) and np.array_equal(after[..., 2], before[..., 2])  # channel 1 alone moves
            where = np.flatnonzero(after.reshape(-1) != before.reshape(-1)).astype(np.int64) * 4
            want["floats"] += where.size
            want["sectors_32"] += len(set((where // 32).tolist()))
            want["pieces_64"] += len(set((where // 64).tolist()))
            want["lines_128"] += len(set((where // 128).tolist()))
            want["boards_changed"] += len(set((where // (4 * 48)).tolist()))
            want["boards_autoreset"] += int(((out["flags"] & 0x20) != 0).sum())
        before = after
    for q in census.QUANTITIES:
        assert got[q] == want[q] / (N * steps), (q, got[q], want[q] / (N * steps))
    assert 1.0 < got["floats"] < 2.5 and got["lines_128"] < got["pieces_64"] < got["sectors_32"] < got["floats"]
    # the command line prints the same table
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "obs_delta_census.py"), "--boards", str(N), "--settle", str(settle),
                          "--steps", str(steps)], check=True, capture_output=True, text=True).stdout
    assert f"| distinct 64-byte pieces | {got['pieces_64']:.3f} |" in run
