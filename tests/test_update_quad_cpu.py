"""The quad store of the in-place step's two-tile kernels without a GPU: the descriptor arithmetic of csrc/ts_quad.h on the host
under AddressSanitizer and UBSan, and what the shipped code object holds of it."""
import os
import re
import subprocess
import tempfile

import pytest

from cabi_harness import _kernel_metadata
from conftest import ROOT

FLAGSHIP = "k_step_update<4, 2, false>"


def test_the_descriptor_arithmetic_on_the_host(tmp_path):
    """csrc/ts_quad.h compiled for the host with the toolchain's clang++ and run over every cell, value, presence and position of
    a slot, the kernel's words for every S <= 8 and both tile counts, and the four passes of a quad against the per-lane loop
    (tests/native/quad_pack_check.cpp), under AddressSanitizer and UBSan: a stand-alone program, no GPU."""
    from tiler_slider_amd import _cabi
    src = os.path.join(ROOT, "tests", "native", "quad_pack_check.cpp")
    exe = str(tmp_path / "quad_pack_check")
    subprocess.run([f"{_cabi._LLVM_BIN}/clang++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), (out.returncode, out.stdout, out.stderr)


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


def _quad_moves(text):
    """The j of every `v_mov_b32_dpp ... quad_perm:[j,j,j,j]` with all rows and banks enabled, in program order."""
    found = []
    for i in text:
        m = re.match(r"v_mov_b32_dpp .*quad_perm:\[(\d),(\d),(\d),(\d)\] row_mask:0xf bank_mask:0xf", i)
        if m:
            assert len(set(m.groups())) == 1, i
            found.append(int(m.group(1)))
    return found


def test_both_bodies_of_the_two_tile_kernels_broadcast_by_quad(disassembly):
    """Each body of a two-tile kernel holds the four passes: a quad-broadcast DPP move of lane 0, 1, 2, 3 of the quad, in that
    order, each followed by one observation store before the next - eight moves in a kernel of two bodies.  The stores are
    dwords in float32 and bytes in uint8.  <1, 2, *> holds the general body alone (a board of one cell cannot hold two tiles)."""
    for S in range(1, 9):
        for u8, store in (("false", "global_store_dword"), ("true", "global_store_byte")):
            text = disassembly[f"k_step_update<{S}, 2, {u8}>"]
            moves = _quad_moves(text)
            bodies = 1 if S == 1 else 2
            assert moves == [0, 1, 2, 3] * bodies, (S, u8, moves)
            assert sum(1 for i in text if "_dpp" in i) == len(moves), (S, u8, "another DPP instruction")
            # between one move and the next (after the last: within the next 16 instructions) exactly one store of the type
            at = [n for n, i in enumerate(text) if i.startswith("v_mov_b32_dpp")]
            for a, b in zip(at, at[1:] + [None]):
                if b is None or _quad_moves(text[b:b + 1]) == [0]:  # the last pass of a body
                    b = a + 16
                stores = [i for i in text[a:b] if i.startswith("global_store_")]
                assert len(stores) == 1 and stores[0].startswith(store + " "), (S, u8, a, stores)
    # the eight-tile kernels keep the per-lane stores
    for S in range(1, 9):
        for u8 in ("false", "true"):
            assert not [i for i in disassembly[f"k_step_update<{S}, 8, {u8}>"] if "_dpp" in i], (S, u8)


def test_the_flagship_kernel_stays_in_registers_at_eight_waves(disassembly):
    """k_step_update<4, 2, false>: no LDS, no scratch, no ds_ instruction, at most 64 VGPRs (eight waves per SIMD), and the
    observation stores keep the `offset register, scalar base` form."""
    from tiler_slider_amd import _update_cabi as uc
    meta = [k for k in _kernel_metadata(uc.LIB_PATH) if "k_step_updateILi4ELi2ELb0E" in k["name"]]  # the mangled <4, 2, false>
    assert len(meta) == 1, [k["name"] for k in _kernel_metadata(uc.LIB_PATH)][:4]
    k = meta[0]
    assert k["group_segment_fixed_size"] == 0 and k["private_segment_fixed_size"] == 0 and not k["uses_dynamic_stack"], k
    assert 0 < k["vgpr_count"] <= 64, k
    text = disassembly[FLAGSHIP]
    assert not [i for i in text if re.match(r"(ds_|scratch_|s_barrier)", i)]
    stores = [i for i in text if i.startswith("global_store_dword ")]
    assert len(stores) >= 8 and all(re.search(r"\bs\[\d+:\d+\]", i) and not re.search(r", off\b", i) for i in stores), stores


def test_the_per_lane_stores_stay_behind_one_knob():
    """-DTS_UPDATE_LANE_PUT is the only way to the parent's stores, it is not defined by the shipped build, and
    tools/update_ab.py names it."""
    from tiler_slider_amd import _update_cabi as uc
    src = open(uc.SRC).read()
    assert src.count("#if defined(TS_UPDATE_LANE_PUT)") == 1 and "#define TS_UPDATE_LANE_PUT" not in src
    assert "constexpr bool kQuadStore = TMAX == 2;" in src
    assert os.path.join(ROOT, "tiler_slider_amd", "csrc", "ts_quad.h") in uc.HEADERS
    tool = open(os.path.join(ROOT, "tools", "update_ab.py")).read()
    assert '"lane": "TS_UPDATE_LANE_PUT=1"' in tool and 'choices=("plain", "sc1", "lane")' in tool
