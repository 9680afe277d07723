"""The in-place step's write-back knobs without a GPU (csrc/ts_update.hip: TS_UPDATE_TRACE, TS_UPDATE_SC1_FIRST / _LAST,
TS_UPDATE_NT, TS_UPDATE_KICK, TS_UPDATE_STATE_ALWAYS; profiles/update_requests.md, section 6): none of them is in the shipped
build but the written-through store of the two-tile kernels; its launch record and exports are what they were."""
import os
import re

from cabi_harness import _dims, _exported, _instruction_counts, _kernel_metadata, _kernel_names
from conftest import ROOT

KNOBS = ("TS_UPDATE_TRACE", "TS_UPDATE_STORE_PLAIN", "TS_UPDATE_STORE_SC1", "TS_UPDATE_SC1_FIRST", "TS_UPDATE_SC1_LAST", "TS_UPDATE_NT", "TS_UPDATE_KICK",
         "TS_UPDATE_STATE_ALWAYS")


def test_the_default_code_object_keeps_its_shape():
    """32 kernels, none with LDS, scratch, a barrier or a ds_ instruction; k_step_update<4, 2, false> between 28 and 64 VGPRs
    (eight waves per SIMD); no write-back instruction, no clock read and no nontemporal store in any kernel.  The two two-tile
    kernels whose board is 192 bytes of observation, <4, 2, false> and <8, 2, true>, write it through - four agent-scope stores
    a body, the state rows plain - and the other thirty store plain."""
    from tiler_slider_amd import _update_cabi as uc
    assert len(_kernel_names(uc.LIB_PATH)) == uc.MIN_KERNELS == 32
    kernels = _kernel_metadata(uc.LIB_PATH)
    assert len(kernels) == 32 and all("k_step_update" in k["name"] for k in kernels)
    assert not any(k["group_segment_fixed_size"] or k["private_segment_fixed_size"] or k["uses_dynamic_stack"] for k in kernels), kernels
    flagship = [k for k in kernels if "k_step_updateILi4ELi2ELb0E" in k["name"]]
    assert len(flagship) == 1 and 28 <= flagship[0]["vgpr_count"] <= 64, flagship
    counts = _instruction_counts(uc.LIB_PATH, (r"\b(s_barrier|ds_\w+|scratch_\w+)\b", r"\bbuffer_wbl2\b", r"\bs_mem(real)?time\b",
                                               r"\bglobal_store_\w+ .*\b(sc0|nt)\b", r"\bglobal_store_\w+ .*\bsc1\b", r"\bglobal_store_"))
    mine = {k: v for k, v in counts.items() if "k_step_update" in k}
    assert len(mine) == 32
    for k, (lds, wbl2, clock, other, through, stores) in mine.items():
        assert (lds, wbl2, clock, other) == (0, 0, 0, 0), (k, lds, wbl2, clock, other)
        size, tmax, u8 = (int(x) for x in re.search(r"k_step_updateILi(\d)ELi(\d)ELb(\d)E", k).groups())
        shipped = tmax == 2 and size * size * 3 * (1 if u8 else 4) == 192
        assert through == (8 if shipped else 0) and stores > through, (k, through, stores)  # two bodies, four passes each


def test_the_store_flavour_stays_behind_its_knobs():
    """The written-through store is the default where the quad stores a board of 192 bytes; -DTS_UPDATE_STORE_PLAIN and -DTS_UPDATE_STORE_SC1
    are the two ways round it, neither defined by the source, and tools/update_ab.py names both."""
    from tiler_slider_amd import _update_cabi as uc
    src = open(uc.SRC).read()
    assert "constexpr bool kThrough = kQuadStore<TMAX> && S * S * 3 * (U8 ? 1 : 4) == 192;" in src
    for knob in ("TS_UPDATE_STORE_PLAIN", "TS_UPDATE_STORE_SC1"):
        assert src.count(f"defined({knob})") == 1 and f"#define {knob}" not in src, knob
    tool = open(os.path.join(ROOT, "tools", "update_ab.py")).read()
    assert "TS_UPDATE_STORE_PLAIN" in tool and '"sc1": "TS_UPDATE_STORE_SC1=1"' in tool


def test_describe_step_update_is_unchanged():
    """The launch record over the shapes of tests/test_update_cpu.py: ceil(N / 256) blocks of four waves, one board per lane,
    the same 32 names."""
    from tiler_slider_amd import _cabi, _update_cabi as uc
    named = set()
    for S in range(1, 9):
        for T in range(1, min(S * S, 8) + 1):
            for Tt in (0, 1, 2, 3, 8):
                for n in (1, 257, 1 << 20):
                    for outputs, u8 in ((_cabi.OUT_OBS, False), (_cabi.OUT_OBS_U8 | _cabi.OUT_REWARD, True)):
                        d = uc.describe_step_update(_dims(S, T, 1, n, Tt=Tt), outputs)
                        tmax = 2 if T <= 2 and Tt <= 2 else 8
                        assert d["name"] == f"k_step_update<{S}, {tmax}, {'true' if u8 else 'false'}>"
                        assert (d["kernel"], d["boards_per_wave"], d["boards_per_lane"], d["lanes_per_board"], d["tiles_per_lane"]) == (6, 64, 1, 1, tmax)
                        assert (d["waves_per_block"], d["blocks"], d["lds_bytes_block"], d["lds_bytes_used"]) == (4, -(-n // 256), 0, 0)
                        assert (d["cached_every"], d["emit_edges"], d["xcd_piece"], d["blocks_per_cu"]) == (0, 0, -1, 0)
                        assert d["extras"] == int(bool(outputs & _cabi.OUT_REWARD))
                        assert d["output_bytes"] == d["resident_bytes"] == (3 if u8 else 12) * S * S * n
                        assert d["out_of_cache"] == int(d["output_bytes"] > 256 << 20)
                        named.add(d["name"])
    assert sorted(named) == _kernel_names(uc.LIB_PATH)


def test_the_trace_export_is_not_in_the_shipped_library():
    """ts_update_trace_read exists only under -DTS_UPDATE_TRACE: the shipped library exports its five entry points and no
    other, the public header does not declare it, and no knob is defined by the source itself."""
    from tiler_slider_amd import _update_cabi as uc
    assert _exported(uc.LIB_PATH) == sorted(uc.EXPORTS) and "ts_update_trace_read" not in _exported(uc.LIB_PATH)
    assert not hasattr(uc.lib(), "ts_update_trace_read")
    assert "trace" not in open(os.path.join(ROOT, "include", "tiler_slider_update.h")).read().lower()
    src = open(uc.SRC).read()
    assert "ts_update_trace_read" in src
    for knob in KNOBS:
        assert re.search(rf"defined\({knob}\)", src), knob
        assert not re.search(rf"#\s*define\s+{knob}\b", src), knob
    tool = open(os.path.join(ROOT, "tools", "update_timeline.py")).read()
    assert "compile_guarded" in tool and "-DTS_UPDATE_TRACE=" in tool
