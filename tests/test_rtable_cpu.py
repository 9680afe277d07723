"""The reachable distance tables without a GPU: the rtable library's C-ABI (include/tiler_slider_rtable.h), its launch plan, its
code object, and its CPU yardstick (tests/rtable_reference.py) against the dense one (tests/table_reference.py) on every state it
reaches, and against the hashed solver's (tests/reach_reference.py) on the root."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cabi_harness import _dims, _instruction_counts, _kernel_metadata, _kernel_names, _struct_fields
from conftest import ROOT

# size, tiles, obstacles, seeds: shapes the dense tables take as well
DENSE = ((3, 2, 1, 64), (4, 2, 2, 64), (4, 4, 2, 8))
# 3x3 with five tiles, 59,049 placements: more than four tiles, C4 = 81^2 no power of two, and the dense yardstick still takes it
LONG = (3, 5, 1, 64)


def test_abi_version_and_constants_are_the_headers():
    import tiler_slider_amd
    from tiler_slider_amd import _rtable_cabi as xc
    header = open(os.path.join(ROOT, "include", "tiler_slider_rtable.h")).read()
    assert xc.lib().ts_rtable_abi_version() == xc.ABI_VERSION == 1
    for name, value in (("TS_RTABLE_ABI_VERSION", 1), ("TS_RTABLE_ABSENT", xc.SOLVE_ABSENT), ("TS_RTABLE_ROOT_INIT", xc.ROOT_INIT),
                        ("TS_RTABLE_ROOT_POS", xc.ROOT_POS)):
        assert int(re.search(rf"#define {name} \(?(-?\d+)\)?", header).group(1)) == value, name
    assert tiler_slider_amd.SOLVE_ABSENT == -4 and tiler_slider_amd.build_rtable_library is xc.build_library
    assert {"ReachTable", "SOLVE_ABSENT", "build_rtable_library"} <= set(tiler_slider_amd.__all__)
    assert xc.MIN_KERNELS == 16 and xc in tiler_slider_amd._libraries.ADDED and xc.ROOTS == {"init": 0, "pos": 1}
    # the four answers that are no move count are distinct
    assert len({tiler_slider_amd.SOLVE_NONE, tiler_slider_amd.SOLVE_DEPTH, tiler_slider_amd.SOLVE_FULL, tiler_slider_amd.SOLVE_ABSENT}) == 4


def test_struct_layouts():
    from tiler_slider_amd import _rtable_cabi as xc
    header = open(os.path.join(ROOT, "include", "tiler_slider_rtable.h")).read()
    for struct, cls, size in (("ts_rtable_cfg", xc.RtableCfg, 32), ("ts_rtable_out", xc.RtableOut, 32), ("ts_rtable_desc", xc.RtableDesc, 8 + 5 * 8 + 64)):
        assert _struct_fields(header, struct) == [f for f, _ in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    assert (xc.RtableCfg.root.offset, xc.RtableCfg.workspace.offset, xc.RtableCfg.workspace_bytes.offset) == (8, 16, 24)
    assert xc.RtableDesc.name.offset == 48


def test_supported_over_the_grid():
    from tiler_slider_amd import _cabi, _reach_cabi as rc, _rtable_cabi as xc
    L = xc.lib()
    for S in range(1, 12):
        for T in range(0, 12):
            for mc in (0, 1):
                want = _cabi.ERR_DIMS if T > S * S else 1 if S <= 8 and T <= 8 else 0
                assert L.ts_rtable_supported(C.byref(_dims(S, T, mc))) == want == rc.lib().ts_reach_supported(C.byref(_dims(S, T, mc))), (S, T)
    assert L.ts_rtable_supported(C.byref(_dims(8, 8, 0, 8, 255))) == 1          # any valid number of targets
    assert L.ts_rtable_supported(C.byref(_dims(1, 1))) == 1 and L.ts_rtable_supported(C.byref(_dims(4, 0))) == 1
    assert L.ts_rtable_supported(None) == _cabi.ERR_NULL
    for bad, want in ((_dims(0, 1), _cabi.ERR_DIMS), (_dims(4, -1), _cabi.ERR_DIMS), (_dims(33, 1), _cabi.ERR_LIMIT), (_dims(4, 2, 2), _cabi.ERR_DIMS),
                      (_dims(4, 2, 0, -1), _cabi.ERR_DIMS), (_dims(4, 2, 0, 8, 256), _cabi.ERR_LIMIT)):
        assert L.ts_rtable_supported(C.byref(bad)) == want
    assert xc.rtable_supported(_dims(5, 4)) and not xc.rtable_supported(_dims(9, 1)) and not xc.rtable_supported(_dims(4, 9))
    with pytest.raises(_cabi.TilerSliderLibraryError):
        xc.rtable_supported(_dims(0, 1))


def test_every_refusal_of_the_build_has_its_own_status_in_the_stated_order():
    """dims (NULL, DIMS), shape (LIMIT), cfg (NULL), argument (ARG), pointer (NULL): each call below breaks one rule and every later
    one, and gets the status of the first.  A HIP call on a box without a GPU would have answered TS_ERR_HIP."""
    from tiler_slider_amd import _cabi, _reach_cabi as rc, _rtable_cabi as xc
    L = xc.lib()
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    full = _cabi.State(p, p, p, p, p, p)
    ok = _dims(5, 4)
    need = xc.workspace_bytes(ok, 16, 1)
    good = xc.RtableCfg(8, 16, 0, p, need)
    out = xc.RtableOut(p, p, p, p)
    ref = lambda x: None if x is None else C.byref(x)
    build = lambda d, st, cfg, o: L.ts_rtable_build(ref(d), ref(st), ref(cfg), ref(o), None)
    bad_arg, no_ptr = xc.RtableCfg(-1, 16, 0, None, need), xc.RtableOut(None, None, None, None)
    assert build(None, None, bad_arg, no_ptr) == _cabi.ERR_NULL                       # 1. dims
    assert build(_dims(0, 2), None, bad_arg, no_ptr) == _cabi.ERR_DIMS
    assert build(_dims(4, 17), None, bad_arg, no_ptr) == _cabi.ERR_DIMS
    for S, T in ((9, 1), (16, 2), (4, 9), (8, 12)):                                    # 2. the shape
        assert build(_dims(S, T), None, bad_arg, no_ptr) == _cabi.ERR_LIMIT, (S, T)
        assert build(_dims(S, T), None, None, no_ptr) == _cabi.ERR_LIMIT, (S, T)
        assert L.ts_describe_rtable_build(C.byref(_dims(S, T)), C.byref(good), C.byref(xc.RtableDesc())) == _cabi.ERR_LIMIT
        assert L.ts_rtable_workspace_bytes(C.byref(_dims(S, T)), 0, 0) == _cabi.ERR_LIMIT
    assert build(ok, None, None, no_ptr) == _cabi.ERR_NULL                             # 3. cfg
    for depth, cap, root in ((-1, 16, 0), (253, 16, 0), (8, 0, 0), (8, -5, 0), (8, rc.REACH_MAX_CAPACITY + 1, 0), (8, 16, 2), (8, 16, -1)):   # 4. an argument
        assert build(ok, None, xc.RtableCfg(depth, cap, root, None, 1 << 40), no_ptr) == _cabi.ERR_ARG, (depth, cap, root)
        assert build(_dims(5, 4, 0, 0), None, xc.RtableCfg(depth, cap, root, None, 1 << 40), no_ptr) == _cabi.ERR_ARG   # also for an empty batch
    assert build(ok, None, xc.RtableCfg(8, 16, 0, None, need - 1), no_ptr) == _cabi.ERR_ARG   # a workspace too small for ONE level
    assert build(ok, None, xc.RtableCfg(8, 16, 0, None, -1), no_ptr) == _cabi.ERR_ARG
    assert build(ok, None, xc.RtableCfg(252, 16, 1, None, need), no_ptr) == _cabi.ERR_NULL   # 5. pointers
    assert build(ok, None, good, out) == _cabi.ERR_NULL
    assert build(ok, full, good, None) == _cabi.ERR_NULL
    assert build(ok, full, good, xc.RtableOut(None, p, p, p)) == _cabi.ERR_NULL               # table is required
    assert build(ok, full, good, xc.RtableOut(p, None, p, p)) == _cabi.ERR_NULL               # count is required
    assert build(ok, full, xc.RtableCfg(8, 16, 0, None, need), out) == _cabi.ERR_NULL         # the workspace
    for missing, root in (("init", 0), ("pos", 1), ("tgt", 0), ("blk", 0)):                   # the root cells are those cfg->root names
        st = _cabi.State(p, p, p, p, p, p)
        setattr(st, missing, None)
        assert build(ok, st, xc.RtableCfg(8, 16, root, p, need), out) == _cabi.ERR_NULL, missing
    # an empty batch: TS_OK, nothing launched, no pointer and no workspace looked at
    empty = _dims(5, 4, 0, 0)
    assert build(empty, None, xc.RtableCfg(8, 16, 1, None, 0), None) == _cabi.OK
    assert L.ts_rtable_last_hip_error() == 0
    d = xc.describe_rtable_build(empty, 8, 16, 0)
    assert (d["blocks"], d["levels_in_flight"], d["name"], d["slots"]) == (0, 0, "", 32)
    assert L.ts_describe_rtable_build(None, C.byref(good), C.byref(xc.RtableDesc())) == _cabi.ERR_NULL
    assert L.ts_describe_rtable_build(C.byref(ok), None, C.byref(xc.RtableDesc())) == _cabi.ERR_NULL
    assert L.ts_describe_rtable_build(C.byref(ok), C.byref(good), None) == _cabi.ERR_NULL
    assert L.ts_rtable_workspace_bytes(None, 16, 1) == _cabi.ERR_NULL
    for cap, flight in ((0, 1), (16, 0), (rc.REACH_MAX_CAPACITY + 1, 1), (rc.REACH_MAX_CAPACITY, 1 << 40)):
        assert L.ts_rtable_workspace_bytes(C.byref(ok), cap, flight) == _cabi.ERR_ARG, (cap, flight)
    for cap in (0, -1, rc.REACH_MAX_CAPACITY + 1):
        assert L.ts_rtable_slots(cap) == _cabi.ERR_ARG


def test_every_refusal_of_the_lookup_has_its_own_status_in_the_stated_order():
    from tiler_slider_amd import _cabi, _rtable_cabi as xc
    L = xc.lib()
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    full = _cabi.State(p, p, p, p, p, p)
    ok = _dims(5, 4)
    ref = lambda x: None if x is None else C.byref(x)
    look = lambda d, st, table, slots, count, n_rows, moves, best=None, action=None: L.ts_rtable_lookup(ref(d), ref(st), table, slots, count, n_rows, None,
                                                                                                         moves, best, action, None)
    assert look(None, None, None, 3, None, -1, None) == _cabi.ERR_NULL                    # 1. dims
    assert look(_dims(0, 2), None, None, 3, None, -1, None) == _cabi.ERR_DIMS
    for S, T in ((9, 1), (4, 9)):                                                          # 2. the shape
        assert look(_dims(S, T), None, None, 3, None, -1, None) == _cabi.ERR_LIMIT
    assert look(ok, None, None, 32, None, -1, None) == _cabi.ERR_ARG                       # 3. an argument
    for slots in (-2, 0, 1, 3, 48, (1 << 31) + 1, 1 << 32):
        assert look(ok, None, None, slots, None, 4, None) == _cabi.ERR_ARG, slots
        assert look(_dims(5, 4, 0, 0), None, None, slots, None, 4, None) == _cabi.ERR_ARG   # also for an empty batch
    assert look(ok, None, None, 32, None, 4, None) == _cabi.ERR_NULL                       # 4. pointers
    assert look(ok, full, p, 32, p, 4, None) == _cabi.ERR_NULL                             # no output at all
    assert look(ok, full, None, 32, p, 4, p) == _cabi.ERR_NULL and look(ok, full, p, 32, None, 4, p) == _cabi.ERR_NULL
    for missing in ("pos", "tgt", "blk"):
        st = _cabi.State(p, p, p, p, p, p)
        setattr(st, missing, None)
        assert look(ok, st, p, 32, p, 4, p) == _cabi.ERR_NULL, missing
    assert look(_dims(5, 4, 0, 0), None, None, 2, None, 0, None) == _cabi.OK and look(_dims(5, 4, 0, 0), None, None, 1 << 31, None, 7, None) == _cabi.OK
    assert L.ts_rtable_last_hip_error() == 0


def test_slots_and_workspace_bytes_are_what_describe_reports():
    from tiler_slider_amd import _reach_cabi as rc, _rtable_cabi as xc
    for cap in (1, 2, 3, 5, 1023, 1024, 1025, 4096, 8192, 100000, rc.REACH_MAX_CAPACITY):
        slots = 1 << max(1, (2 * cap - 1).bit_length())
        assert xc.slots(cap) == slots > cap and slots <= 1 << 31
        assert slots == rc.describe_reach(_dims(5, 4), 64, cap, 1 << 50)["slots_per_board"]   # the hashed solver's table, level for level
        for S, T, n in ((5, 4, 1), (8, 8, 257), (1, 1, 70000), (4, 0, 3)):
            one = xc.workspace_bytes(_dims(S, T), cap, 1)
            assert one == 8 * ((cap + 1) // 2) + 16 * cap and one % 8 == 0     # the log of slots and four successor slots a state
            for flight in (1, 3, 1024):
                assert xc.workspace_bytes(_dims(S, T), cap, flight) == flight * one
            d = xc.describe_rtable_build(_dims(S, T, 0, n), 252, cap, 7 * one + 5)
            assert (d["slots"], d["table_bytes"], d["workspace_bytes"]) == (slots, 8 * slots, one)
            assert d["levels_in_flight"] == d["blocks"] == min(n, 7) and d["threads_per_block"] == 256
    # at most 1,024 levels in flight however large the workspace, and never more than there are levels
    assert xc.describe_rtable_build(_dims(5, 4, 0, 5000), 252, 16, 1 << 40)["blocks"] == 1024
    assert xc.describe_rtable_build(_dims(5, 4, 0, 9), 252, 16, 1 << 40)["blocks"] == 9


def test_describe_names_the_compiled_build_kernels_and_the_code_object_holds_the_lookups():
    from tiler_slider_amd import _rtable_cabi as xc
    compiled = _kernel_names(xc.LIB_PATH)
    named = {xc.describe_rtable_build(_dims(S, min(T, S * S), mc), root=root)["name"] for S in range(1, 9) for T in (0, 1, 4, 8) for mc in (0, 1)
             for root in (0, 1)}
    assert sorted(named) == [f"k_rtable_build<{S}>" for S in range(1, 9)]
    assert compiled == sorted(named) + [f"k_rtable_lookup<{S}>" for S in range(1, 9)]


def test_the_kernels_use_no_scratch_no_float_and_plain_vector_memory_only():
    from tiler_slider_amd import _rtable_cabi as xc
    meta = _kernel_metadata(xc.LIB_PATH)
    assert len(meta) == 16
    for k in meta:
        assert k["private_segment_fixed_size"] == 0 and not k["uses_dynamic_stack"] and k["agpr_count"] == 0, k
        # the build's five control words; the lookup uses no LDS
        assert k["group_segment_fixed_size"] == (20 if "k_rtable_build" in k["name"] else 0), k
    counts = _instruction_counts(xc.LIB_PATH, (r"\bv_\w+_f(16|32|64)\b", r"\bscratch_", r"\bs_barrier\b", r"\bglobal_atomic_cmpswap_x2\b", r"\bglobal_atomic"))
    build = {k: v for k, v in counts.items() if "k_rtable_build" in k}
    look = {k: v for k, v in counts.items() if "k_rtable_lookup" in k}
    assert len(build) == len(look) == 8
    for k, (floats, scratch, barriers, cas, atomics) in build.items():
        assert floats == 0 and scratch == 0 and barriers > 0 and cas > 0, (k, floats, scratch, barriers, cas)
    for k, (floats, scratch, barriers, cas, atomics) in look.items():
        assert floats == 0 and scratch == 0 and barriers == 0 and atomics == 0, (k, floats, scratch, barriers, atomics)


def test_occupancy_cases_name_exactly_the_compiled_rtable_kernels():
    """tests/test_gpu_reach_occupancy.py runs one case per kernel - the builds on a full grid, the lookups at 4,096 waves -: its
    case table (tests/reach_cases.py) is the code object's list, no kernel without a case and no case without a kernel; the
    library names the build kernel for the case's dims and plans the grid the GPU test relies on, 1,024 blocks for 1,024 + 61
    levels."""
    import reach_cases as cases
    from tiler_slider_amd import _rtable_cabi as xc
    assert sorted(cases.RTABLE_CASES) == _kernel_names(xc.LIB_PATH)
    assert len(cases.RTABLE_CASES) == xc.MIN_KERNELS == 16
    for name, (S, T, K) in cases.RTABLE_CASES.items():
        what = "build" if "build" in name else "lookup"
        assert name == f"k_rtable_{what}<{S}>" and (T, K) == cases.SHAPES[S][:2] and T + K <= S * S and (T > 4 or S * S <= 4)
        for mc in (0, 1):
            for depth in (252, 3):
                for root in (0, 1):
                    d = xc.describe_rtable_build(_dims(S, T, mc, cases.N_BUILD), depth, cases.CAPACITY, root=root)
                    assert (d["name"], d["blocks"], d["levels_in_flight"], d["threads_per_block"]) == (f"k_rtable_build<{S}>", cases.GRID, cases.GRID, 256), d
    assert cases.N_LOOKUP % 64 != 0 and -(-cases.N_LOOKUP // 64) >= 4096   # one board per lane: at least 4,096 waves, a ragged last one


@pytest.mark.parametrize("S", range(1, 9))
def test_occupancy_cases_are_not_degenerate(oracle, S):
    """The conditions tests/reach_cases.py sets on the yardstick's answer hold for the levels it draws, in both colour modes: large
    levels that are built, FULL levels, won roots, spread root distances, entries of both kinds - and keys beyond 2^32 from 6x6."""
    import reach_cases as cases
    import rtable_reference as rt
    won = not_won = 0
    for mc in (False, True):
        blk, init, tgt = cases.levels(oracle, S, mc)
        s = cases.check_rtable(S, rt.build(oracle, S, mc, blk, tgt, init, 252, cases.CAPACITY))
        won, not_won = won + s["won"], not_won + cases.DISTINCT - s["won"]
        assert S == 1 or (s["won"] and s["won"] < cases.DISTINCT), s
    assert won and not_won


@pytest.mark.parametrize("S,T,K,n", DENSE + (LONG,))
@pytest.mark.parametrize("mc", (False, True))
def test_yardstick_equals_the_dense_one_on_every_state_it_reaches(oracle, S, T, K, n, mc):
    """Every state of R holds the dense table's entry (a path to the win stays inside R), no state of R is won or invalid there,
    the successors are the dense table's, and deepest / root_moves / count follow from the row."""
    import rtable_reference as rt
    import table_reference as dense
    if (S, T, K, n) == LONG:
        import reach_cases as cases
        assert (T, K) == cases.SHAPES[S][:2]
        blk, init, tgt = (np.ascontiguousarray(a[:, :n]) for a in cases.levels(oracle, S, mc))
    else:
        blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    exact = dense.exact(oracle, S, mc, blk, tgt, T)
    assert exact[exact < dense.UNREACHABLE].max() <= dense.MAX_DEPTH
    full = dense.cut(exact)
    ref = rt.build(oracle, S, mc, blk, tgt, init)
    assert (ref.count != rt.SOLVE_FULL).all() and ref.count.sum() == ref.idx.size > n
    for lv in range(n):
        keys, entries = ref.keys(lv), ref.entries(lv)
        assert (np.diff(keys) > 0).all() and len(keys) == ref.count[lv]
        np.testing.assert_array_equal(entries, full[lv, keys], err_msg=str((S, T, mc, lv)))
        assert ((entries >= 1) & (entries <= dense.MAX_DEPTH) | (entries == dense.NONE)).all()
        finite = entries[entries <= dense.MAX_DEPTH]
        assert ref.deepest[lv] == (finite.max() if finite.size else 0)
        root = int(dense.index_of(S, init[:, lv:lv + 1])[0])
        assert ref.root_moves[lv] == dense.to_moves(full[lv, root:root + 1])[0]
        assert (ref.count[lv] == 0) == (full[lv, root] == 0) and (ref.count[lv] == 0 or root in keys)
    # the lookup rule on every state of R against the dense lookup rule on the dense table
    lv = np.repeat(np.arange(n), ref.count)
    pos = np.concatenate([ref.cells(i) for i in range(n)], axis=1)
    b, t = np.ascontiguousarray(blk[:, lv]), np.ascontiguousarray(tgt[:, lv])
    got = rt.lookup(oracle, ref, b, t, pos, rows=lv)
    want = dense.lookup(oracle, S, b, pos, full, rows=lv)
    for g, w, name in zip(got, want, ("moves", "best", "action")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    # cut short: what is within reach keeps its distance, the rest is DEEP, or NONE where a round found nothing
    for depth in (0, 3):
        cut = rt.build(oracle, S, mc, blk, tgt, init, max_depth=depth)
        np.testing.assert_array_equal(cut.idx, ref.idx)
        near = (ref.entry >= 1) & (ref.entry <= depth)
        np.testing.assert_array_equal(cut.entry[near], ref.entry[near])
        assert np.isin(cut.entry[~near], (rt.DEEP, rt.NONE)).all() and (cut.deepest <= depth).all()
        stopped = np.array([not all((ref.entries(i) == d).any() for d in range(1, depth + 1)) for i in range(n)])
        np.testing.assert_array_equal(cut.entry[~near] == rt.NONE, stopped[cut.level[~near]])


@pytest.mark.parametrize("S,T,K,mc,n", ((4, 2, 2, False, 64), (4, 4, 2, True, 8), (5, 4, 3, True, 32), (5, 4, 3, False, 32), (8, 3, 10, False, 32)))
def test_yardsticks_root_moves_are_the_hashed_solvers_yardsticks(oracle, S, T, K, mc, n):
    """An unbounded breadth-first search from the root (tests/reach_reference.py) finds the root's distance, or that there is none;
    a level that cannot be won holds exactly the states that search expanded."""
    import reach_reference as reach
    import rtable_reference as rt
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    ref = rt.build(oracle, S, mc, blk, tgt, init)
    moves, states = reach.search(oracle, S, mc, blk, tgt, init, 32767, reach.UNBOUNDED)
    assert (moves <= rt.MAX_DEPTH).all()
    np.testing.assert_array_equal(ref.root_moves, moves)
    never = moves == reach.SOLVE_NONE
    np.testing.assert_array_equal(ref.count[never], states[never])
    assert (ref.count[~never] >= states[~never]).all()
    # the budget: FULL exactly where the closure is larger, and nothing of a FULL level is kept
    tight = rt.build(oracle, S, mc, blk, tgt, init, capacity=100)
    np.testing.assert_array_equal(tight.count, np.where(ref.count > 100, rt.SOLVE_FULL, ref.count))
    np.testing.assert_array_equal(tight.root_moves, np.where(ref.count > 100, rt.SOLVE_FULL, ref.root_moves))
    assert tight.idx.size == ref.count[ref.count <= 100].sum() and (tight.deepest[ref.count > 100] == 0).all()
