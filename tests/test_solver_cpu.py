"""The on-device solver without a GPU: the search library's C-ABI (include/tiler_slider_search.h), its launch plan, its code
object, and the CPU yardstick (tests/solver_reference.py) against the optimal move counts already in git."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cabi_harness import _assert_build_goes_through_the_guard, _dims, _instruction_counts, _kernel_names
from conftest import GOLDEN_DIR, ROOT


def test_search_library_exports_what_its_header_declares():
    from tiler_slider_amd import _search_cabi
    header = open(os.path.join(ROOT, "include", "tiler_slider_search.h")).read()
    for name, value in (("TS_SOLVE_NONE", _search_cabi.SOLVE_NONE),
                        ("TS_SOLVE_DEPTH", _search_cabi.SOLVE_DEPTH), ("TS_SOLVE_MAX_STATES", _search_cabi.SOLVE_MAX_STATES),
                        ("TS_SOLVE_MAX_SIZE", _search_cabi.SOLVE_MAX_SIZE), ("TS_SOLVE_MAX_DEPTH", _search_cabi.SOLVE_MAX_DEPTH)):
        assert int(re.search(rf"#define {name} \(?(-?\d+)\)?", header).group(1)) == value, name
    import tiler_slider_amd
    assert (tiler_slider_amd.SOLVE_NONE, tiler_slider_amd.SOLVE_DEPTH) == (-1, -2)


def test_solve_states():
    from tiler_slider_amd import _cabi, _search_cabi
    L = _search_cabi.lib()
    for (S, T), want in (((4, 2), 256), ((5, 3), 15625), ((6, 3), 46656), ((4, 4), 65536), ((8, 2), 4096), ((5, 4), 0), ((8, 3), 0),
                         ((9, 1), 0), ((3, 5), 59049), ((3, 6), 0), ((1, 1), 1), ((7, 0), 1), ((32, 1), 0)):
        for mc in (0, 1):
            assert L.ts_solve_states(C.byref(_dims(S, T, mc))) == want, (S, T)
    assert L.ts_solve_states(None) == _cabi.ERR_NULL
    for bad, want in ((_dims(0, 1), _cabi.ERR_DIMS), (_dims(4, -1), _cabi.ERR_DIMS), (_dims(4, 17), _cabi.ERR_DIMS), (_dims(33, 1), _cabi.ERR_LIMIT),
                      (_dims(4, 2, 2), _cabi.ERR_DIMS), (_dims(4, 2, 0, -1), _cabi.ERR_DIMS), (_dims(4, 2, 0, 8, 256), _cabi.ERR_LIMIT)):
        assert L.ts_solve_states(C.byref(bad)) == want
    assert _search_cabi.solve_states(_dims(4, 2)) == 256
    with pytest.raises(_cabi.TilerSliderLibraryError):
        _search_cabi.solve_states(_dims(0, 1))


def test_argument_validation_precedes_any_launch():
    """Every refusal below returns its own status: a HIP call on this GPU-less box would have answered TS_ERR_HIP."""
    from tiler_slider_amd import _cabi, _search_cabi
    L = _search_cabi.lib()
    ok = _dims(4, 2)
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    full = _cabi.State(p, p, p, p, p, p)
    assert L.ts_solve(None, C.byref(full), 8, p, p, None) == _cabi.ERR_NULL
    assert L.ts_solve(C.byref(ok), None, 8, p, p, None) == _cabi.ERR_NULL
    assert L.ts_solve(C.byref(ok), C.byref(full), 8, None, p, None) == _cabi.ERR_NULL          # moves is required
    for missing in ("pos", "tgt", "blk"):
        st = _cabi.State(p, p, p, p, p, p)
        setattr(st, missing, None)
        assert L.ts_solve(C.byref(ok), C.byref(st), 8, p, p, None) == _cabi.ERR_NULL, missing
    for S, T in ((5, 4), (8, 3), (9, 1), (16, 2)):
        assert L.ts_solve(C.byref(_dims(S, T)), C.byref(full), 8, p, p, None) == _cabi.ERR_LIMIT
        assert L.ts_describe_solve(C.byref(_dims(S, T)), C.byref(_search_cabi.SolveDesc())) == _cabi.ERR_LIMIT
    assert L.ts_solve(C.byref(_dims(0, 2)), C.byref(full), 8, p, p, None) == _cabi.ERR_DIMS
    for depth in (-1, 32768, 2**31 - 1):
        assert L.ts_solve(C.byref(ok), C.byref(full), depth, p, p, None) == _cabi.ERR_ARG
    # an empty batch: TS_OK, nothing launched, with or without buffers; best = NULL passes validation like any other call
    empty = _dims(4, 2, 0, 0)
    assert L.ts_solve(C.byref(empty), None, 8, None, None, None) == _cabi.OK
    assert L.ts_solve(C.byref(empty), C.byref(full), 0, p, None, None) == _cabi.OK
    assert L.ts_solve(C.byref(empty), C.byref(full), -1, p, None, None) == _cabi.ERR_ARG
    assert L.ts_search_last_hip_error() == 0
    assert L.ts_describe_solve(None, C.byref(_search_cabi.SolveDesc())) == _cabi.ERR_NULL
    assert L.ts_describe_solve(C.byref(ok), None) == _cabi.ERR_NULL
    d = _search_cabi.describe_solve(empty)
    assert (d["form"], d["blocks"], d["name"], d["states"]) == (_search_cabi.FORM_NONE, 0, "", 256)


def _supported_shapes():
    from tiler_slider_amd import _search_cabi
    for S in range(1, 9):
        for T in range(0, S * S + 1):
            if _search_cabi.lib().ts_solve_states(C.byref(_dims(S, T))) <= 0:
                break
            for mc in (0, 1):
                yield S, T, mc


def test_describe_solve_names_exactly_the_compiled_kernels():
    """Every kernel of the search library's code object is what some supported shape launches under the library's own policy,
    and every launch names a kernel that exists: no compiled form that no call reaches, none missing."""
    from tiler_slider_amd import _search_cabi as sc
    compiled = _kernel_names(sc.LIB_PATH)
    assert len(compiled) >= sc.MIN_KERNELS
    assert sc.lib().ts_search_tuning(sc.TUNE_WAVE_MAX_STATES, -1) == 8192 and sc.lib().ts_search_tuning(sc.TUNE_WORDS_PER_LANE, -1) == 1
    named = {}
    for S, T, mc in _supported_shapes():
        for n in (1, 7, 4096, 1 << 20):
            d = sc.describe_solve(_dims(S, T, mc, n))
            named.setdefault(d["name"], []).append((S, T))
            words = -(-d["states"] // 32)
            assert d["states"] == (S * S) ** T and d["bitmap_words"] == words and d["lds_bytes_board"] == 4 * (7 * words + 3)
            assert d["lds_bytes_block"] == d["boards_per_block"] * d["lds_bytes_board"] <= 64 * 1024
            assert d["blocks"] == -(-n // d["boards_per_block"])
            if d["form"] == sc.FORM_WAVE:
                assert d["name"] == f"k_solve_wave<{S}>" and d["threads_per_block"] == 64 and d["states"] <= 8192
                assert d["lanes_per_board"] == min(64, 1 << (words - 1).bit_length()) and d["boards_per_block"] * d["lanes_per_board"] == 64
            else:
                assert d["form"] == sc.FORM_BLOCK and d["name"] == f"k_solve_block<{S}>" and d["states"] > 8192
                assert (d["threads_per_block"], d["lanes_per_board"], d["boards_per_block"]) == (256, 256, 1)
    assert sorted(named) == compiled
    # the issue's shapes: cfg1's 224 bytes of bitmaps per board, eight lanes; 6x6 / 3 tiles 40 KiB in the block form
    assert sc.describe_solve(_dims(4, 2))["lds_bytes_board"] == 224 + 12 and sc.describe_solve(_dims(4, 2))["lanes_per_board"] == 8
    assert sc.describe_solve(_dims(6, 3))["lds_bytes_board"] == 7 * 1458 * 4 + 12 and sc.describe_solve(_dims(6, 3))["form"] == sc.FORM_BLOCK


def test_search_tuning_knobs_choose_between_forms_only_where_both_exist():
    from tiler_slider_amd import _search_cabi as sc
    L = sc.lib()
    assert L.ts_search_tuning(99, 1) == -1 and L.ts_search_tuning(-1, -1) == -1
    try:
        assert L.ts_search_tuning(sc.TUNE_WAVE_MAX_STATES, 0) == 8192
        assert sc.describe_solve(_dims(4, 2))["name"] == "k_solve_block<4>"     # forced: cfg1's shape, one board per block
        assert sc.describe_solve(_dims(8, 2))["name"] == "k_solve_wave<8>"      # no block form is compiled for 8x8
        L.ts_search_tuning(sc.TUNE_WAVE_MAX_STATES, 65536)
        d = sc.describe_solve(_dims(4, 4))
        assert (d["name"], d["lanes_per_board"], d["boards_per_block"], d["lds_bytes_block"]) == ("k_solve_wave<4>", 64, 1, 7 * 8192 + 12)
        L.ts_search_tuning(sc.TUNE_WAVE_MAX_STATES, 8192)
        assert L.ts_search_tuning(sc.TUNE_WORDS_PER_LANE, 2) == 1
        assert sc.describe_solve(_dims(4, 2))["lanes_per_board"] == 4 and sc.describe_solve(_dims(5, 2))["lanes_per_board"] == 16
    finally:
        L.ts_search_tuning(sc.TUNE_WAVE_MAX_STATES, 8192)
        L.ts_search_tuning(sc.TUNE_WORDS_PER_LANE, 1)


def test_wave_form_has_no_block_barrier():
    """k_solve_wave runs in one-wave blocks so that its __syncthreads() costs no s_barrier: checked in the shipped code object."""
    from tiler_slider_amd import _search_cabi as sc
    barriers = {k: v[0] for k, v in _instruction_counts(sc.LIB_PATH, (r"\bs_barrier\b",)).items()}
    wave = {k: v for k, v in barriers.items() if "k_solve_wave" in k}
    block = {k: v for k, v in barriers.items() if "k_solve_block" in k}
    assert len(wave) == 8 and not any(wave.values()), wave
    assert len(block) == 4 and all(block.values()), block


def test_compile_guarded_tells_a_small_library_from_a_parse_failure(monkeypatch):
    """compile_guarded's last check takes "no kernel fills its register allocation" for unparsed metadata - right for the step
    library's hundreds of kernels, wrong for a handful.  With min_kernels the check counts parsed kernels instead; the step
    library's call (min_kernels=None) is what it was."""
    import inspect
    from tiler_slider_amd import _cabi, _search_cabi
    sig = inspect.signature(_cabi.compile_guarded)
    assert sig.parameters["min_kernels"].default is None
    assert _cabi.MIN_KERNELS is None and _search_cabi.MIN_KERNELS == 12
    _assert_build_goes_through_the_guard(_cabi, monkeypatch)
    _assert_build_goes_through_the_guard(_search_cabi, monkeypatch)


def test_yardstick_reproduces_the_recorded_optimum_of_the_400_screenshot_levels(oracle):
    """tests/solver_reference.py against numbers already in git: min_moves of tests/golden/levels_from_screenshots.npz (1 .. 15,
    every level solvable), and the `best` mask against its definition replayed by hand - stepping by a best move leaves
    min_moves - 1, stepping by any other does not."""
    import solver_reference as ref
    from tiler_slider_amd.levels import pack_levels
    total = 0
    for (S, T, mc), (ids, blk, init, tgt, want) in ref.fixture_groups(GOLDEN_DIR, pack_levels).items():
        moves, best = ref.solve(oracle, S, mc, blk, tgt, init)
        np.testing.assert_array_equal(moves, want, err_msg=str((S, T, mc)))
        assert moves.min() >= 1 and (best != 0).all() and (best < 16).all()
        # shallower searches: exactly the boards within reach keep their optimum, the others report SOLVE_DEPTH
        for depth in (0, 3, 7):
            np.testing.assert_array_equal(ref.optimum(oracle, S, mc, blk, tgt, init, depth), np.where(want <= depth, want, ref.SOLVE_DEPTH))
        for a in range(4):
            b = oracle.OracleBatch(S, mc, 2**30, blk, init, tgt)
            b.step(np.full(len(ids), a, np.uint8), obs=False)
            after = ref.optimum(oracle, S, mc, blk, tgt, b.pos)
            np.testing.assert_array_equal(after == want - 1, (best >> a) & 1 != 0)
        total += len(ids)
    assert total == 400
