"""The hashed solver without a GPU: the reach library's C-ABI (include/tiler_slider_reach.h), its launch plan, its code object,
and its CPU yardstick (tests/reach_reference.py) against the dense one (tests/solver_reference.py) wherever both apply."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cabi_harness import _dims, _instruction_counts, _kernel_metadata, _kernel_names, _struct_fields
from conftest import GOLDEN_DIR, ROOT

# size, tiles, obstacles, multi colour: the rows of DESIGN.md section 11 (tests/test_gpu_solver.py: ROWS)
ROWS = ((4, 2, 2, False), (4, 2, 2, True), (5, 2, 3, False), (5, 3, 3, True), (6, 3, 6, False), (8, 2, 10, True), (3, 4, 1, False), (4, 4, 2, True))
# 3x3 with five tiles, 59,049 placements: more than four tiles, C4 = 81^2 no power of two, and the dense yardstick still takes it
LONG_ROWS = ((3, 5, 1, False), (3, 5, 1, True))


def test_abi_version_and_constants_are_the_headers():
    import tiler_slider_amd
    from tiler_slider_amd import _reach_cabi as rc
    header = open(os.path.join(ROOT, "include", "tiler_slider_reach.h")).read()
    assert rc.lib().ts_reach_abi_version() == rc.ABI_VERSION == 1
    for name, value in (("TS_REACH_ABI_VERSION", 1), ("TS_REACH_FULL", rc.SOLVE_FULL), ("TS_REACH_MAX_SIZE", rc.REACH_MAX_SIZE),
                        ("TS_REACH_MAX_TILES", rc.REACH_MAX_TILES), ("TS_REACH_MAX_DEPTH", rc.REACH_MAX_DEPTH),
                        ("TS_REACH_MAX_CAPACITY", rc.REACH_MAX_CAPACITY)):
        assert int(re.search(rf"#define {name} \(?(-?\d+)\)?", header).group(1)) == value, name
    assert tiler_slider_amd.SOLVE_FULL == -3 and tiler_slider_amd.build_reach_library is rc.build_library
    assert rc.MIN_KERNELS == 8 and rc in tiler_slider_amd._libraries.ADDED
    # a board has pow2ceil(2 * capacity) slots and the log holds their numbers in 32 bits
    assert 2 * rc.REACH_MAX_CAPACITY <= 1 << 31


def test_struct_layouts():
    from tiler_slider_amd import _reach_cabi as rc
    header = open(os.path.join(ROOT, "include", "tiler_slider_reach.h")).read()
    for struct, cls, size in (("ts_reach_cfg", rc.ReachCfg, 24), ("ts_reach_out", rc.ReachOut, 24), ("ts_reach_desc", rc.ReachDesc, 8 + 7 * 8 + 64)):
        assert _struct_fields(header, struct) == [f for f, _ in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    assert rc.ReachCfg.workspace.offset == 8 and rc.ReachCfg.workspace_bytes.offset == 16 and rc.ReachDesc.name.offset == 64


def test_supported_over_the_grid():
    from tiler_slider_amd import _cabi, _reach_cabi as rc
    L = rc.lib()
    for S in range(1, 12):
        for T in range(0, 12):
            for mc in (0, 1):
                want = _cabi.ERR_DIMS if T > S * S else 1 if S <= 8 and T <= 8 else 0
                assert L.ts_reach_supported(C.byref(_dims(S, T, mc))) == want, (S, T)
    assert L.ts_reach_supported(C.byref(_dims(8, 8, 0, 8, 255))) == 1          # any valid number of targets
    assert L.ts_reach_supported(None) == _cabi.ERR_NULL
    for bad, want in ((_dims(0, 1), _cabi.ERR_DIMS), (_dims(4, -1), _cabi.ERR_DIMS), (_dims(33, 1), _cabi.ERR_LIMIT), (_dims(4, 2, 2), _cabi.ERR_DIMS),
                      (_dims(4, 2, 0, -1), _cabi.ERR_DIMS), (_dims(4, 2, 0, 8, 256), _cabi.ERR_LIMIT)):
        assert L.ts_reach_supported(C.byref(bad)) == want
    assert rc.reach_supported(_dims(5, 4)) and not rc.reach_supported(_dims(9, 1)) and not rc.reach_supported(_dims(4, 9))
    with pytest.raises(_cabi.TilerSliderLibraryError):
        rc.reach_supported(_dims(0, 1))


def test_every_refusal_has_its_own_status_in_the_stated_order():
    """dims (NULL, DIMS), shape (LIMIT), argument (ARG), pointer (NULL): each call below breaks one rule and every later one, and
    gets the status of the first.  A HIP call on a box without a GPU would have answered TS_ERR_HIP."""
    from tiler_slider_amd import _cabi, _reach_cabi as rc
    L = rc.lib()
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    full = _cabi.State(p, p, p, p, p, p)
    ok = _dims(5, 4)
    need = rc.workspace_bytes(ok, 16, 1)
    good = rc.ReachCfg(8, 16, p, need)
    out = rc.ReachOut(p, p, p)
    solve = lambda d, st, cfg, o: L.ts_reach_solve(None if d is None else C.byref(d), None if st is None else C.byref(st),
                                                   None if cfg is None else C.byref(cfg), None if o is None else C.byref(o), None)
    bad_arg, no_ptr = rc.ReachCfg(-1, 16, None, need), rc.ReachOut(None, None, None)
    assert solve(None, None, bad_arg, no_ptr) == _cabi.ERR_NULL                       # 1. dims
    assert solve(_dims(0, 2), None, bad_arg, no_ptr) == _cabi.ERR_DIMS
    assert solve(_dims(4, 17), None, bad_arg, no_ptr) == _cabi.ERR_DIMS
    for S, T in ((9, 1), (16, 2), (4, 9), (8, 12)):                                    # 2. the shape
        assert solve(_dims(S, T), None, bad_arg, no_ptr) == _cabi.ERR_LIMIT, (S, T)
        assert L.ts_describe_reach(C.byref(_dims(S, T)), C.byref(good), C.byref(rc.ReachDesc())) == _cabi.ERR_LIMIT
        assert L.ts_reach_workspace_bytes(C.byref(_dims(S, T)), 0, 0) == _cabi.ERR_LIMIT
    for depth, cap in ((-1, 16), (32768, 16), (8, 0), (8, -5), (8, rc.REACH_MAX_CAPACITY + 1)):   # 3. an argument
        assert solve(ok, None, rc.ReachCfg(depth, cap, None, 1 << 40), no_ptr) == _cabi.ERR_ARG, (depth, cap)
        assert solve(_dims(5, 4, 0, 0), None, rc.ReachCfg(depth, cap, None, 1 << 40), no_ptr) == _cabi.ERR_ARG   # also for an empty batch
    assert solve(ok, None, rc.ReachCfg(8, 16, None, need - 1), no_ptr) == _cabi.ERR_ARG   # a workspace too small for ONE board
    assert solve(ok, None, rc.ReachCfg(8, 16, None, -1), no_ptr) == _cabi.ERR_ARG
    assert solve(ok, None, rc.ReachCfg(8, 16, None, need), no_ptr) == _cabi.ERR_NULL       # 4. pointers
    assert solve(ok, full, None, out) == _cabi.ERR_NULL
    assert solve(ok, None, good, out) == _cabi.ERR_NULL
    assert solve(ok, full, good, None) == _cabi.ERR_NULL
    assert solve(ok, full, good, rc.ReachOut(None, p, p)) == _cabi.ERR_NULL               # moves is required
    assert solve(ok, full, rc.ReachCfg(8, 16, None, need), out) == _cabi.ERR_NULL         # the workspace
    for missing in ("pos", "tgt", "blk"):
        st = _cabi.State(p, p, p, p, p, p)
        setattr(st, missing, None)
        assert solve(ok, st, good, out) == _cabi.ERR_NULL, missing
    # an empty batch: TS_OK, nothing launched, no pointer and no workspace looked at
    empty = _dims(5, 4, 0, 0)
    assert solve(empty, None, rc.ReachCfg(8, 16, None, 0), None) == _cabi.OK
    assert L.ts_reach_last_hip_error() == 0
    d = rc.describe_reach(empty, 8, 16, 0)
    assert (d["blocks"], d["boards_in_flight"], d["name"], d["slots_per_board"]) == (0, 0, "", 32)
    assert L.ts_describe_reach(None, C.byref(good), C.byref(rc.ReachDesc())) == _cabi.ERR_NULL
    assert L.ts_describe_reach(C.byref(ok), None, C.byref(rc.ReachDesc())) == _cabi.ERR_NULL
    assert L.ts_describe_reach(C.byref(ok), C.byref(good), None) == _cabi.ERR_NULL
    assert L.ts_reach_workspace_bytes(None, 16, 1) == _cabi.ERR_NULL
    for cap, flight in ((0, 1), (16, 0), (rc.REACH_MAX_CAPACITY + 1, 1), (rc.REACH_MAX_CAPACITY, 1 << 40)):
        assert L.ts_reach_workspace_bytes(C.byref(ok), cap, flight) == _cabi.ERR_ARG, (cap, flight)


def test_workspace_bytes_are_the_sum_of_what_describe_reports():
    from tiler_slider_amd import _reach_cabi as rc
    for cap in (1, 2, 3, 5, 1023, 1024, 1025, 4096, 8192, 100000, rc.REACH_MAX_CAPACITY):
        slots = 1 << max(1, (2 * cap - 1).bit_length())
        for S, T, n in ((5, 4, 1), (8, 8, 257), (1, 1, 70000), (4, 0, 3)):
            one = rc.workspace_bytes(_dims(S, T), cap, 1)
            for flight in (1, 3, 1024):
                assert rc.workspace_bytes(_dims(S, T), cap, flight) == flight * one
            d = rc.describe_reach(_dims(S, T, 0, n), 64, cap, 7 * one + 5)
            assert (d["slots_per_board"], d["table_bytes"], d["frontier_bytes"], d["log_bytes"]) == (slots, 8 * slots, 8 * cap, 8 * ((cap + 1) // 2))
            assert slots > cap and d["log_bytes"] >= 4 * cap
            assert d["table_bytes"] + d["frontier_bytes"] + d["log_bytes"] == d["bytes_per_board"] == one
            assert d["boards_in_flight"] == d["blocks"] == min(n, 7) and d["threads_per_block"] == 256
    # at most 1,024 boards in flight however large the workspace, and never more than there are boards
    assert rc.describe_reach(_dims(5, 4, 0, 5000), 64, 16, 1 << 40)["blocks"] == 1024
    assert rc.describe_reach(_dims(5, 4, 0, 9), 64, 16, 1 << 40)["blocks"] == 9


def test_describe_reach_names_exactly_the_compiled_kernels():
    from tiler_slider_amd import _reach_cabi as rc
    compiled = _kernel_names(rc.LIB_PATH)
    named = {rc.describe_reach(_dims(S, min(T, S * S), mc))["name"] for S in range(1, 9) for T in (0, 1, 4, 8) for mc in (0, 1)}
    assert sorted(named) == compiled == [f"k_reach<{S}>" for S in range(1, 9)]


def test_the_kernels_use_no_scratch_no_float_and_plain_vector_memory_only():
    from tiler_slider_amd import _reach_cabi as rc
    meta = _kernel_metadata(rc.LIB_PATH)
    assert len(meta) == 8
    for k in meta:
        assert k["private_segment_fixed_size"] == 0 and not k["uses_dynamic_stack"] and k["agpr_count"] == 0, k
        assert k["group_segment_fixed_size"] == 12, k                      # the three control words
    counts = _instruction_counts(rc.LIB_PATH, (r"\bv_\w+_f(16|32|64)\b", r"\bscratch_", r"\bs_barrier\b", r"\bglobal_atomic_cmpswap_x2\b"))
    kernels = {k: v for k, v in counts.items() if "k_reach" in k}
    assert len(kernels) == 8
    for k, (floats, scratch, barriers, cas) in kernels.items():
        assert floats == 0 and scratch == 0 and barriers > 0 and cas > 0, (k, floats, scratch, barriers, cas)


def test_occupancy_cases_name_exactly_the_compiled_reach_kernels():
    """tests/test_gpu_reach_occupancy.py runs one case per kernel on a full grid: its case table (tests/reach_cases.py) is the code
    object's list, no kernel without a case and no case without a kernel; the library names that kernel for the case's dims and
    plans the grid the GPU test relies on - 1,024 blocks, a slice each, for a batch of 1,024 + 61 boards."""
    import reach_cases as cases
    from tiler_slider_amd import _reach_cabi as rc
    assert sorted(cases.REACH_CASES) == _kernel_names(rc.LIB_PATH)
    assert len(cases.REACH_CASES) == rc.MIN_KERNELS == 8
    for name, (S, T, K) in cases.REACH_CASES.items():
        assert name == f"k_reach<{S}>" and (T, K) == cases.SHAPES[S][:2] and T + K <= S * S and (T > 4 or S * S <= 4)
        for mc in (0, 1):
            for depth in (64, 3):
                d = rc.describe_reach(_dims(S, T, mc, cases.N_BUILD), depth, cases.CAPACITY)
                assert (d["name"], d["blocks"], d["boards_in_flight"], d["threads_per_block"]) == (name, cases.GRID, cases.GRID, 256), d
    assert cases.N_BUILD > cases.GRID and cases.N_BUILD % cases.GRID == 61


@pytest.mark.parametrize("S", range(1, 9))
def test_occupancy_cases_are_not_degenerate(oracle, S):
    """The conditions tests/reach_cases.py sets on the yardstick's answer hold for the levels it draws: boards that can be won,
    boards that cannot and boards that run out of their budget in every case from 3x3 up, in both colour modes."""
    import reach_cases as cases
    import reach_reference as reach
    seen = set()
    for mc in (False, True):
        blk, init, tgt = cases.levels(oracle, S, mc)
        assert blk.shape[1] == init.shape[1] == tgt.shape[1] == cases.DISTINCT and init.shape[0] == cases.SHAPES[S][0]
        s = cases.check_reach(S, reach.solve(oracle, S, mc, blk, tgt, init, 64, cases.CAPACITY))
        seen |= {k for k in ("won", "solved", "none") if s[k]}
        assert S == 1 or (s["won"] and s["solved"] + s["none"]), s
    assert "won" in seen and seen & {"solved", "none"}


@pytest.mark.parametrize("S,T,K,mc", ROWS + LONG_ROWS)
def test_yardstick_equals_the_dense_one_where_the_budget_is_the_index_space(oracle, S, T, K, mc):
    """capacity = (S * S) ** T can never be exceeded: moves and best of tests/solver_reference.py, at full depth and cut short."""
    import reach_reference as reach
    import solver_reference as dense
    if (S, T, K, mc) in LONG_ROWS:
        import reach_cases as cases
        assert (T, K) == cases.SHAPES[S][:2]
        blk, init, tgt = (np.ascontiguousarray(a[:, :64]) for a in cases.levels(oracle, S, mc))
    else:
        blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(64, dtype=np.uint32))
    space = (S * S) ** T
    for depth in (64, 3, 0):
        want = dense.solve(oracle, S, mc, blk, tgt, init, depth)
        moves, best, states = reach.solve(oracle, S, mc, blk, tgt, init, depth, space)
        np.testing.assert_array_equal(moves, want[0], err_msg=str((S, T, mc, depth)))
        np.testing.assert_array_equal(best, want[1], err_msg=str((S, T, mc, depth)))
        assert (moves != reach.SOLVE_FULL).all() and (states <= space).all() and ((states == 0) == ((moves == 0) | (depth == 0))).all()
    # the budget: a board that expanded R states in all is FULL at every capacity below what it reached, with fewer states expanded
    full_moves, full_states = reach.search(oracle, S, mc, blk, tgt, init, 64, 3)
    m64, s64 = reach.search(oracle, S, mc, blk, tgt, init, 64, space)
    assert ((full_moves == reach.SOLVE_FULL) | (full_moves == m64)).all() and (full_states <= s64).all()
    assert (full_moves[m64 == reach.SOLVE_NONE][s64[m64 == reach.SOLVE_NONE] > 3] == reach.SOLVE_FULL).all()
    assert (full_moves[s64 <= 3] == m64[s64 <= 3]).all()


def test_yardstick_reproduces_the_recorded_optimum_of_the_400_screenshot_levels(oracle):
    import reach_reference as reach
    import solver_reference as dense
    from tiler_slider_amd.levels import pack_levels
    total = 0
    for (S, T, mc), (ids, blk, init, tgt, want) in dense.fixture_groups(GOLDEN_DIR, pack_levels).items():
        moves, best, states = reach.solve(oracle, S, mc, blk, tgt, init, 64, (S * S) ** T)
        np.testing.assert_array_equal(moves, want, err_msg=str((S, T, mc)))
        np.testing.assert_array_equal(best, dense.solve(oracle, S, mc, blk, tgt, init)[1], err_msg=str((S, T, mc)))
        assert (states >= moves).all()   # a shortest solution of d moves expands at least one state per depth
        total += len(ids)
    assert total == 400
