"""The distance-to-win tables without a GPU: the table library's C-ABI (include/tiler_slider_table.h), its launch plan, its code
object, and the CPU yardstick (tests/table_reference.py) against the optimal move counts already in git."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cabi_harness import _dims, _instruction_counts, _kernel_names
from conftest import GOLDEN_DIR, ROOT


def test_table_library_exports_what_its_header_declares():
    from tiler_slider_amd import _table_cabi
    header = open(os.path.join(ROOT, "include", "tiler_slider_table.h")).read()
    for name, value in (("TS_TABLE_MAX_DEPTH", _table_cabi.TABLE_MAX_DEPTH),
                        ("TS_TABLE_INVALID", _table_cabi.TABLE_INVALID), ("TS_TABLE_DEEP", _table_cabi.TABLE_DEEP),
                        ("TS_TABLE_NONE", _table_cabi.TABLE_NONE), ("TS_TABLE_FORM_NONE", _table_cabi.FORM_NONE),
                        ("TS_TABLE_FORM_WAVE", _table_cabi.FORM_WAVE), ("TS_TABLE_FORM_BLOCK", _table_cabi.FORM_BLOCK),
                        ("TS_TABLE_TUNE_WAVE_MAX_STATES", _table_cabi.TUNE_WAVE_MAX_STATES),
                        ("TS_TABLE_TUNE_STATES_PER_LANE", _table_cabi.TUNE_STATES_PER_LANE),
                        ("TS_TABLE_TUNE_BLOCK_BELOW_BOARDS", _table_cabi.TUNE_BLOCK_BELOW_BOARDS)):
        assert int(re.search(rf"#define {name} \(?(-?\d+)\)?", header).group(1)) == value, name
    assert (_table_cabi.TABLE_MAX_DEPTH, _table_cabi.TABLE_INVALID, _table_cabi.TABLE_DEEP, _table_cabi.TABLE_NONE) == (252, 253, 254, 255)
    import tiler_slider_amd
    assert (tiler_slider_amd.TABLE_MAX_DEPTH, tiler_slider_amd.TABLE_INVALID, tiler_slider_amd.TABLE_DEEP, tiler_slider_amd.TABLE_NONE) == (252, 253, 254, 255)
    assert tiler_slider_amd.DistanceTable is not None and callable(tiler_slider_amd.build_table_library)


def test_table_states_are_the_solvers():
    from tiler_slider_amd import _cabi, _search_cabi, _table_cabi
    L, LS = _table_cabi.lib(), _search_cabi.lib()
    for S in range(0, 11):
        for T in range(-1, 8):
            for mc in (0, 1, 2):
                d = _dims(S, T, mc)
                assert L.ts_table_states(C.byref(d)) == LS.ts_solve_states(C.byref(d)), (S, T, mc)
    assert L.ts_table_states(None) == _cabi.ERR_NULL
    assert _table_cabi.table_states(_dims(4, 2)) == 256 and _table_cabi.table_states(_dims(5, 4)) == 0
    with pytest.raises(_cabi.TilerSliderLibraryError):
        _table_cabi.table_states(_dims(0, 1))


def test_argument_validation_precedes_any_launch():
    """Every refusal below returns its own status: a HIP call on this GPU-less box would have answered TS_ERR_HIP."""
    from tiler_slider_amd import _cabi, _table_cabi
    L = _table_cabi.lib()
    ok = _dims(4, 2)
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    full = _cabi.State(p, p, p, p, p, p)
    # ts_table_build
    assert L.ts_table_build(None, C.byref(full), 8, p, None) == _cabi.ERR_NULL
    assert L.ts_table_build(C.byref(ok), None, 8, p, None) == _cabi.ERR_NULL
    assert L.ts_table_build(C.byref(ok), C.byref(full), 8, None, None) == _cabi.ERR_NULL          # the table is required
    for missing in ("tgt", "blk"):
        st = _cabi.State(p, p, p, p, p, p)
        setattr(st, missing, None)
        assert L.ts_table_build(C.byref(ok), C.byref(st), 8, p, None) == _cabi.ERR_NULL, missing
    for S, T in ((5, 4), (8, 3), (9, 1), (16, 2)):
        assert L.ts_table_build(C.byref(_dims(S, T)), C.byref(full), 8, p, None) == _cabi.ERR_LIMIT
        assert L.ts_describe_table_build(C.byref(_dims(S, T)), C.byref(_table_cabi.TableDesc())) == _cabi.ERR_LIMIT
        assert L.ts_table_lookup(C.byref(_dims(S, T)), C.byref(full), p, 8, None, p, p, p, None) == _cabi.ERR_LIMIT
    assert L.ts_table_build(C.byref(_dims(0, 2)), C.byref(full), 8, p, None) == _cabi.ERR_DIMS
    assert L.ts_table_lookup(C.byref(_dims(0, 2)), C.byref(full), p, 8, None, p, p, p, None) == _cabi.ERR_DIMS
    for depth in (-1, 253, 32767, 2**31 - 1):
        assert L.ts_table_build(C.byref(ok), C.byref(full), depth, p, None) == _cabi.ERR_ARG
    # an unsupported shape is refused before a bad max_depth, a bad max_depth before a missing pointer: ts_solve's order
    assert L.ts_table_build(C.byref(_dims(5, 4)), None, -1, None, None) == _cabi.ERR_LIMIT
    assert L.ts_table_build(C.byref(ok), None, -1, None, None) == _cabi.ERR_ARG
    # an empty batch: TS_OK, nothing launched, with or without buffers
    empty = _dims(4, 2, 0, 0)
    assert L.ts_table_build(C.byref(empty), None, 8, None, None) == _cabi.OK
    assert L.ts_table_build(C.byref(empty), C.byref(full), 0, p, None) == _cabi.OK
    assert L.ts_table_build(C.byref(empty), C.byref(full), 253, p, None) == _cabi.ERR_ARG
    # ts_table_lookup
    assert L.ts_table_lookup(None, C.byref(full), p, 8, None, p, p, p, None) == _cabi.ERR_NULL
    assert L.ts_table_lookup(C.byref(ok), None, p, 8, None, p, p, p, None) == _cabi.ERR_NULL
    assert L.ts_table_lookup(C.byref(ok), C.byref(full), None, 8, None, p, p, p, None) == _cabi.ERR_NULL      # a table of 8 rows
    assert L.ts_table_lookup(C.byref(ok), C.byref(full), p, 8, None, None, None, None, None) == _cabi.ERR_NULL  # no output at all
    for missing in ("pos", "blk"):
        st = _cabi.State(p, p, p, p, p, p)
        setattr(st, missing, None)
        assert L.ts_table_lookup(C.byref(ok), C.byref(st), p, 8, None, p, p, p, None) == _cabi.ERR_NULL, missing
    assert L.ts_table_lookup(C.byref(ok), C.byref(full), p, -1, None, p, p, p, None) == _cabi.ERR_ARG
    assert L.ts_table_lookup(C.byref(empty), None, None, 0, None, None, None, None, None) == _cabi.OK
    assert L.ts_table_lookup(C.byref(empty), C.byref(full), p, -1, None, p, p, p, None) == _cabi.ERR_ARG
    assert L.ts_table_last_hip_error() == 0
    assert L.ts_describe_table_build(None, C.byref(_table_cabi.TableDesc())) == _cabi.ERR_NULL
    assert L.ts_describe_table_build(C.byref(ok), None) == _cabi.ERR_NULL
    d = _table_cabi.describe_table_build(empty)
    assert (d["form"], d["blocks"], d["name"], d["states"], d["table_bytes"]) == (_table_cabi.FORM_NONE, 0, "", 256, 0)


def _supported_shapes():
    from tiler_slider_amd import _table_cabi
    for S in range(1, 9):
        for T in range(0, S * S + 1):
            if _table_cabi.lib().ts_table_states(C.byref(_dims(S, T))) <= 0:
                break
            for mc in (0, 1):
                yield S, T, mc


def test_describe_table_build_names_exactly_the_compiled_kernels():
    """Every build kernel of the table library's code object is what some supported shape launches under the library's own
    policy, every launch names a kernel that exists, and beside them there is one lookup kernel per supported board size: no
    compiled form that no call reaches, none missing.  Every plan stays within the LDS bound it declares."""
    from tiler_slider_amd import _table_cabi as tc
    compiled = _kernel_names(tc.LIB_PATH)
    assert len(compiled) == tc.MIN_KERNELS
    wave_max = tc.lib().ts_table_tuning(tc.TUNE_WAVE_MAX_STATES, -1)
    spl = tc.lib().ts_table_tuning(tc.TUNE_STATES_PER_LANE, -1)
    below = tc.lib().ts_table_tuning(tc.TUNE_BLOCK_BELOW_BOARDS, -1)
    assert wave_max > 0 and spl >= 1 and below >= 0
    named, sizes = {}, set()
    for S, T, mc in _supported_shapes():
        sizes.add(S)
        for n in (1, 7, 4096, 1 << 20):
            d = tc.describe_table_build(_dims(S, T, mc, n))
            named.setdefault(d["name"], []).append((S, T))
            words = -(-d["states"] // 32)
            assert d["states"] == (S * S) ** T and d["bitmap_words"] == words and d["lds_bytes_board"] == 4 * (3 * words + 2)
            assert d["lds_bytes_block"] == d["boards_per_block"] * d["lds_bytes_board"] <= d["lds_bytes_max"] == 64 * 1024
            assert d["blocks"] == -(-n // d["boards_per_block"]) and d["table_bytes"] == n * d["states"]
            # a block per board for large index spaces and for small batches, where a block form is compiled (every size but 1x1)
            block = S >= 2 and (d["states"] > wave_max or (d["states"] >= 256 and n < below))
            assert d["form"] == (tc.FORM_BLOCK if block else tc.FORM_WAVE)
            if d["form"] == tc.FORM_WAVE:
                assert d["name"] == f"k_table_wave<{S}>" and d["threads_per_block"] == 64
                want = -(-d["states"] // spl)
                assert d["lanes_per_board"] == min(64, 1 << (want - 1).bit_length()) and d["boards_per_block"] * d["lanes_per_board"] == 64
            else:
                assert d["name"] == f"k_table_block<{S}>"
                assert (d["threads_per_block"], d["lanes_per_board"], d["boards_per_block"]) == (256, 256, 1)
    assert sorted(list(named) + [f"k_table_lookup<{S}>" for S in sizes]) == compiled
    # the issue's figures: three bitmaps are 96 B at 4x4 / 2 tiles and 24 KiB at the cap
    assert tc.describe_table_build(_dims(4, 2))["lds_bytes_board"] == 96 + 8
    assert tc.describe_table_build(_dims(4, 2, n=1 << 20))["form"] == tc.FORM_WAVE and tc.describe_table_build(_dims(2, 4, n=7))["name"] == "k_table_block<2>"
    assert tc.describe_table_build(_dims(4, 4))["lds_bytes_board"] == 24 * 1024 + 8 and tc.describe_table_build(_dims(4, 4, n=1 << 20))["form"] == tc.FORM_BLOCK


def test_table_tuning_knobs_choose_between_forms_only_where_both_exist():
    from tiler_slider_amd import _table_cabi as tc
    L = tc.lib()
    assert L.ts_table_tuning(99, 1) == -1 and L.ts_table_tuning(-1, -1) == -1
    keys = (tc.TUNE_WAVE_MAX_STATES, tc.TUNE_STATES_PER_LANE, tc.TUNE_BLOCK_BELOW_BOARDS)
    wave_max, spl, below = (L.ts_table_tuning(k, -1) for k in keys)
    big = 1 << 20
    try:
        assert L.ts_table_tuning(tc.TUNE_WAVE_MAX_STATES, 0) == wave_max
        assert tc.describe_table_build(_dims(4, 2, n=big))["name"] == "k_table_block<4>"   # forced: one board per block
        assert tc.describe_table_build(_dims(8, 2, n=big))["name"] == "k_table_block<8>"
        assert tc.describe_table_build(_dims(1, 1, n=big))["name"] == "k_table_wave<1>"    # no block form is compiled for 1x1
        L.ts_table_tuning(tc.TUNE_WAVE_MAX_STATES, 65536)
        assert L.ts_table_tuning(tc.TUNE_BLOCK_BELOW_BOARDS, 0) == below
        d = tc.describe_table_build(_dims(4, 4, n=3))
        assert (d["name"], d["lanes_per_board"], d["boards_per_block"], d["lds_bytes_block"]) == ("k_table_wave<4>", 64, 1, 3 * 8192 + 8)
        # the small-batch rule: fewer boards than the knob, and at least a placement per thread of the block
        L.ts_table_tuning(tc.TUNE_BLOCK_BELOW_BOARDS, 100)
        assert tc.describe_table_build(_dims(4, 2, n=99))["name"] == "k_table_block<4>" and tc.describe_table_build(_dims(4, 2, n=100))["name"] == "k_table_wave<4>"
        assert tc.describe_table_build(_dims(3, 2, n=99))["name"] == "k_table_wave<3>"     # 81 placements
        assert L.ts_table_tuning(tc.TUNE_STATES_PER_LANE, 32) == spl
        assert tc.describe_table_build(_dims(4, 2, n=big))["lanes_per_board"] == 8 and tc.describe_table_build(_dims(5, 2, n=big))["lanes_per_board"] == 32
        assert tc.describe_table_build(_dims(4, 2, n=big))["lds_bytes_block"] == 8 * 104
    finally:
        for k, v in zip(keys, (wave_max, spl, below)):
            L.ts_table_tuning(k, v)


def test_wave_form_has_no_block_barrier_and_the_lookup_no_lds():
    from tiler_slider_amd import _table_cabi as tc
    counts = _instruction_counts(tc.LIB_PATH, (r"\bs_barrier\b", r"\bds_"))
    barriers, lds = {k: v[0] for k, v in counts.items()}, {k: v[1] for k, v in counts.items()}
    wave = {k: v for k, v in barriers.items() if "k_table_wave" in k}
    block = {k: v for k, v in barriers.items() if "k_table_block" in k}
    look = {k: v for k, v in lds.items() if "k_table_lookup" in k}
    assert len(wave) == 8 and not any(wave.values()), wave
    assert len(block) == 7 and all(block.values()), block
    assert len(look) == 8 and not any(look.values()), look


def _start_entries(S, tab, init):
    import table_reference as tref
    return tab[np.arange(tab.shape[0]), tref.index_of(S, init)]


def test_yardstick_reproduces_the_recorded_optimum_of_the_400_screenshot_levels(oracle):
    """tests/table_reference.py against numbers already in git: the entry at each level's start cells is min_moves of
    tests/golden/levels_from_screenshots.npz; every table holds all three kinds of entry beside the finite ones or says so."""
    import solver_reference as ref
    import table_reference as tref
    from tiler_slider_amd.levels import pack_levels
    total = 0
    for (S, T, mc), (ids, blk, init, tgt, want) in ref.fixture_groups(GOLDEN_DIR, pack_levels).items():
        dist = tref.exact(oracle, S, mc, blk, tgt, T)
        tab = tref.cut(dist)
        np.testing.assert_array_equal(_start_entries(S, tab, init), want, err_msg=str((S, T, mc)))
        assert ((tab == 0).sum(axis=1) >= 1).all() and (tab == tref.DEEP).sum() == 0
        print(f"{S}x{S} T={T} mc={mc}: {len(ids)} levels, deepest entry {tab[tab <= tref.MAX_DEPTH].max()}, "
              f"{(tab == tref.NONE).sum()} NONE, {(tab == tref.INVALID).sum()} INVALID of {tab.size}")
        # shallower tables: what lies within reach keeps its entry
        for depth in (0, 3, 7):
            shallow = tref.cut(dist, depth)
            np.testing.assert_array_equal(_start_entries(S, shallow, init), np.where(want <= depth, want, tref.DEEP))
        total += len(ids)
    assert total == 400


@pytest.mark.parametrize("S,T,K,mc,n", ((4, 2, 2, False, 400), (4, 2, 2, True, 400), (5, 2, 3, False, 200), (5, 3, 3, True, 60), (6, 3, 6, False, 20),
                                        (8, 2, 10, True, 100), (3, 4, 1, False, 100), (4, 4, 2, True, 12)))
def test_yardstick_start_entries_equal_the_solver_yardstick_on_seeded_levels(oracle, S, T, K, mc, n):
    import solver_reference as ref
    import table_reference as tref
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    dist = tref.exact(oracle, S, mc, blk, tgt, T)
    tab = tref.cut(dist)
    want = ref.optimum(oracle, S, mc, blk, tgt, init, max_depth=32767)
    np.testing.assert_array_equal(tref.to_moves(_start_entries(S, tab, init)), want)
    # a cut table: DEEP exactly on the boards whose R(depth) is not empty, NONE on the others
    for depth in (0, 2):
        shallow = tref.cut(dist, depth)
        deep_board = (dist == depth).any(axis=1)
        unresolved = (dist > depth)
        np.testing.assert_array_equal(shallow[unresolved], np.broadcast_to(np.where(deep_board[:, None], tref.DEEP, tref.NONE), dist.shape)[unresolved])
        np.testing.assert_array_equal(shallow[~unresolved], tab[~unresolved])


def test_yardstick_lookup_at_the_start_of_the_400_screenshot_levels_is_the_recorded_optimum(oracle):
    """table_reference.lookup against numbers already in git: from each level's start cells it reports the fixture's min_moves,
    a best mask that is not empty, and its lowest bit as the action."""
    import solver_reference as ref
    import table_reference as tref
    from tiler_slider_amd.levels import pack_levels
    total = 0
    for (S, T, mc), (ids, blk, init, tgt, want) in ref.fixture_groups(GOLDEN_DIR, pack_levels).items():
        tab = tref.table(oracle, S, mc, blk, tgt, T)
        moves, best, action = tref.lookup(oracle, S, blk, init, tab)
        assert moves.dtype == np.int16 and best.dtype == np.uint8 and action.dtype == np.uint8
        np.testing.assert_array_equal(moves, want, err_msg=str((S, T, mc)))
        assert (best >= 1).all() and (best <= 15).all()
        np.testing.assert_array_equal(action, [(int(b) & -int(b)).bit_length() - 1 for b in best])
        # the same boards through rows=, in reverse order, and a row outside the table
        back = np.arange(len(ids))[::-1]
        again = tref.lookup(oracle, S, blk[:, back], init[:, back], tab, rows=back)
        np.testing.assert_array_equal(again[0], want[back])
        np.testing.assert_array_equal(again[1], best[back])
        out = tref.lookup(oracle, S, blk, init, tab, rows=np.full(len(ids), len(ids)))
        assert (out[0] == -1).all() and (out[1] == 0).all() and (out[2] == 255).all()
        total += len(ids)
    assert total == 400


@pytest.mark.parametrize("S,T,K,mc,n", ((4, 2, 2, False, 40), (5, 2, 3, True, 12)))
def test_yardstick_lookup_over_every_valid_placement_is_the_solver_yardstick(oracle, S, T, K, mc, n):
    """Two yardsticks that share no method: the lookup over the relaxed table, and a breadth-first search (solver_reference.solve)
    from the same cells - every valid placement of every level, moves and best."""
    import solver_reference as ref
    import table_reference as tref
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    tab = tref.table(oracle, S, mc, blk, tgt, T)
    level, state = np.nonzero(tab != tref.INVALID)
    C = S * S
    pos = np.stack([(state // C ** t) % C for t in range(T)]).astype(np.uint8)
    moves, best, action = tref.lookup(oracle, S, blk[:, level], pos, tab, rows=level)
    want = ref.solve(oracle, S, mc, blk[:, level], tgt[:, level], pos, max_depth=32767)
    kinds = ((want[0] >= 1).sum(), (want[0] == 0).sum(), (want[0] == -1).sum())
    print(f"{S}x{S} T={T} K={K} mc={mc}: {len(level)} placements, moves >= 1 / 0 / -1: {kinds}, deepest {want[0].max()}")
    assert min(kinds) >= 3
    np.testing.assert_array_equal(moves, want[0])
    np.testing.assert_array_equal(best, want[1])
    np.testing.assert_array_equal(action[best == 0], 255)
    assert ((best[best != 0] >> action[best != 0]) & 1).all() and ((best[best != 0] & ((1 << action[best != 0]) - 1)) == 0).all()
    # an invalid placement - the first tile on the second one's cell - is answered without the oracle
    twice = pos.copy()
    twice[0] = twice[1]
    out = tref.lookup(oracle, S, blk[:, level], twice, tab, rows=level)
    assert (out[0] == -1).all() and (out[1] == 0).all() and (out[2] == 255).all()


def test_occupancy_cases_name_exactly_the_compiled_table_kernels():
    """tests/test_gpu_table.py runs one case per kernel at 4,096 waves: its case table (tests/table_harness.py) is the code
    object's list, no kernel without a case and no case without a kernel; the knobs of each build case really select the kernel
    it is named after."""
    import table_harness as th
    from tiler_slider_amd import _table_cabi as tc
    assert sorted(th.OCCUPANCY_CASES) == _kernel_names(tc.LIB_PATH)
    assert len(th.OCCUPANCY_CASES) == tc.MIN_KERNELS == 23
    before = [tc.lib().ts_table_tuning(k, -1) for k in (0, 1, 2)]
    for name, (S, T, K, knobs) in th.OCCUPANCY_CASES.items():
        assert f"<{S}>" in name and (S * S) ** T <= 65536
        if "lookup" in name:
            assert not knobs
            continue
        with th.knobs(knobs):
            for n in (1021, 4349):
                assert tc.describe_table_build(_dims(S, T, 0, n))["name"] == name
    S, T, K, knobs = th.SUB_WAVE_CASE
    with th.knobs(knobs):
        d = tc.describe_table_build(_dims(S, T, 0, 4349))
        assert (d["name"], d["boards_per_block"], d["lanes_per_board"]) == ("k_table_wave<4>", 8, 8)
    assert [tc.lib().ts_table_tuning(k, -1) for k in (0, 1, 2)] == before
