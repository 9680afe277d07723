"""The reach-table experts without a GPU: the rexpert library's C-ABI (include/tiler_slider_rexpert.h), its launch plans, its code
object, its occupancy cases, and the non-degeneracy conditions of the GPU tests' base case on the CPU yardstick
(tests/rexpert_reference.py) alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cabi_harness import _dims, _instruction_counts, _kernel_metadata, _kernel_names, _struct_fields
from conftest import ROOT

MAX_STEPS = 65535


def _header():
    return open(os.path.join(ROOT, "include", "tiler_slider_rexpert.h")).read()


def _cfg(ec, steps=4, mode=0, write_state=1, threshold=0, table=None, slots=32, count=None, n_rows=0):
    return ec.RexpertCfg(steps, mode, write_state, 0, 0, 0, 0, threshold, table, slots, count, n_rows, None)


def test_abi_version_and_constants_are_the_headers():
    import tiler_slider_amd
    from tiler_slider_amd import _rexpert_cabi as ec, _rollout_cabi, _targets_cabi
    assert ec.lib().ts_rexpert_abi_version() == ec.ABI_VERSION == 1
    assert int(re.search(r"#define TS_REXPERT_ABI_VERSION (\d+)", _header()).group(1)) == 1
    assert ec.MIN_KERNELS == 16 and ec in tiler_slider_amd._libraries.ADDED and len(tiler_slider_amd._libraries.ADDED) == 3
    assert tiler_slider_amd.build_rexpert_library is ec.build_library and "build_rexpert_library" in tiler_slider_amd.__all__
    # the outputs are the parents' structs, not copies
    assert ec.RolloutOut is _rollout_cabi.RolloutOut and ec.LabelsOut is _targets_cabi.LabelsOut
    assert (ec.LABELS_OUT_MOVES, ec.LABELS_OUT_BEST, ec.LABELS_OUT_ACTION) == (1, 2, 4)
    for name in ('#include "tiler_slider_rollout.h"', '#include "tiler_slider_rtable.h"', '#include "tiler_slider_targets.h"'):
        assert name in _header()
    src = open(ec.SRC).read()
    assert '#include "ts_core.h"' in src and '#include "ts_launch.h"' in src


def test_struct_layouts():
    from tiler_slider_amd import _rexpert_cabi as ec
    for struct, cls, size in (("ts_rexpert_cfg", ec.RexpertCfg, 16 + 4 * 8 + 5 * 8), ("ts_rexpert_labels_in", ec.RexpertLabelsIn, 5 * 8 + 2 * 8 + 8),
                              ("ts_rexpert_desc", ec.RexpertDesc, 8 + 4 * 8 + 64)):
        assert _struct_fields(_header(), struct) == [f for f, _ in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    assert (ec.RexpertCfg.seed.offset, ec.RexpertCfg.explore_threshold.offset, ec.RexpertCfg.table.offset, ec.RexpertCfg.rows.offset) == (16, 40, 48, 80)
    assert (ec.RexpertLabelsIn.slots.offset, ec.RexpertLabelsIn.steps.offset) == (40, 56) and ec.RexpertDesc.name.offset == 40


def test_supported_over_the_grid_is_what_both_parents_take():
    from tiler_slider_amd import _cabi, _rexpert_cabi as ec, _rollout_cabi as rc, _rtable_cabi as xc
    L = ec.lib()
    for S in range(1, 12):
        for T in range(0, 12):
            for Tt in (0, 1, 8, 9, 12):
                d = _dims(S, T, 0, 8, Tt)
                mine = L.ts_rexpert_supported(C.byref(d))
                a, b = rc.lib().ts_rollout_supported(C.byref(d), rc.RANDOM), xc.lib().ts_rtable_supported(C.byref(d))
                want = _cabi.ERR_DIMS if T > S * S else 1 if S <= 8 and T <= 8 and Tt <= 8 else 0
                assert mine == want == (a if a < 0 else int(a == 1 and b == 1)), (S, T, Tt, mine, a, b)
    assert L.ts_rexpert_supported(None) == _cabi.ERR_NULL
    for bad, want in ((_dims(0, 1), _cabi.ERR_DIMS), (_dims(4, -1), _cabi.ERR_DIMS), (_dims(33, 1), 0), (_dims(4, 2, 2), _cabi.ERR_DIMS),
                      (_dims(4, 2, 0, -1), _cabi.ERR_DIMS), (_dims(4, 2, 0, 8, 256), 0)):
        assert L.ts_rexpert_supported(C.byref(bad)) == want
    assert ec.rexpert_supported(_dims(5, 4)) and ec.rexpert_supported(_dims(8, 8)) and not ec.rexpert_supported(_dims(9, 1))
    with pytest.raises(_cabi.TilerSliderLibraryError):
        ec.rexpert_supported(_dims(0, 1))


def test_every_refusal_of_the_rollout_has_its_own_status_in_the_stated_order():
    """dims (NULL, DIMS, LIMIT), cfg (NULL), shape (LIMIT), argument (ARG), the empty launch (OK), pointer (NULL): each call below
    breaks one rule and every later one, and gets the status of the first.  A HIP call on a box without a GPU would have answered
    TS_ERR_HIP."""
    from tiler_slider_amd import _cabi, _rexpert_cabi as ec
    L = ec.lib()
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    full = _cabi.State(p, p, p, p, p, p)
    ok = _dims(5, 4)
    ref = lambda x: None if x is None else C.byref(x)
    play = lambda d, st, cfg, o: L.ts_rexpert_rollout(ref(d), ref(st), ref(cfg), ref(o), None)
    desc = lambda d, cfg, mask=0: L.ts_describe_rexpert_rollout(ref(d), ref(cfg), mask, C.byref(ec.RexpertDesc()))
    bad_arg = _cfg(ec, steps=-1, n_rows=4)
    assert play(None, None, bad_arg, None) == _cabi.ERR_NULL                              # 1. dims
    assert play(_dims(0, 2), None, bad_arg, None) == _cabi.ERR_DIMS
    assert play(_dims(33, 2), None, None, None) == _cabi.ERR_LIMIT
    assert play(ok, None, None, None) == _cabi.ERR_NULL                                   # 2. cfg
    for S, T, Tt in ((9, 1, 1), (16, 2, 2), (4, 9, 9), (4, 2, 9)):                        # 3. the shape
        assert play(_dims(S, T, 0, 8, Tt), None, bad_arg, None) == _cabi.ERR_LIMIT, (S, T, Tt)
        assert desc(_dims(S, T, 0, 8, Tt), bad_arg) == _cabi.ERR_LIMIT
    bad = [_cfg(ec, mode=2), _cfg(ec, mode=0x80000000), _cfg(ec, steps=-1), _cfg(ec, steps=MAX_STEPS + 1), _cfg(ec, threshold=(1 << 32) + 1),
           _cfg(ec, n_rows=-1)] + [_cfg(ec, slots=s) for s in (-2, 0, 1, 3, 48, (1 << 31) + 1, 1 << 32)]
    for cfg in bad:                                                                       # 4. an argument
        assert play(ok, None, cfg, None) == _cabi.ERR_ARG and desc(ok, cfg) == _cabi.ERR_ARG
        assert play(_dims(5, 4, 0, 0), None, cfg, None) == _cabi.ERR_ARG                  # also for an empty batch
    out = ec.RolloutOut(p, p, p, p, p, p, p, p, p)
    for empty, cfg in ((_dims(5, 4, 0, 0), _cfg(ec, n_rows=4)), (ok, _cfg(ec, steps=0, n_rows=4))):   # 5. nothing to launch
        assert play(empty, None, cfg, None) == _cabi.OK
    good = _cfg(ec, table=p, count=p, n_rows=4, threshold=1 << 32, slots=1 << 31, steps=MAX_STEPS)
    assert play(ok, None, good, out) == _cabi.ERR_NULL and play(ok, full, good, None) == _cabi.ERR_NULL   # 6. pointers
    for missing in ("pos", "tgt", "blk", "step_count", "done"):
        st = _cabi.State(p, p, p, p, p, p)
        setattr(st, missing, None)
        assert play(ok, st, good, out) == _cabi.ERR_NULL, missing
    no_init = _cabi.State(p, None, p, p, p, p)
    auto = _cfg(ec, mode=1, table=p, count=p, n_rows=4)
    assert play(ok, no_init, auto, out) == _cabi.ERR_NULL                                  # init: auto-reset mode only
    assert play(ok, full, _cfg(ec, table=None, count=p, n_rows=4), out) == _cabi.ERR_NULL
    assert play(ok, full, _cfg(ec, table=p, count=None, n_rows=4), out) == _cabi.ERR_NULL
    assert play(ok, full, _cfg(ec, table=p, count=p, n_rows=4, write_state=0), ec.RolloutOut()) == _cabi.ERR_NULL   # neither an output nor write_state
    assert L.ts_rexpert_last_hip_error() == 0
    # describe: any NULL first
    assert desc(None, good) == _cabi.ERR_NULL and desc(ok, None) == _cabi.ERR_NULL
    assert L.ts_describe_rexpert_rollout(C.byref(ok), C.byref(good), 0, None) == _cabi.ERR_NULL
    assert desc(_dims(0, 2), good) == _cabi.ERR_DIMS


def test_every_refusal_of_the_labels_has_its_own_status_in_the_stated_order():
    from tiler_slider_amd import _cabi, _rexpert_cabi as ec
    L = ec.lib()
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    full = _cabi.State(None, None, p, p, None, None)
    ok = _dims(5, 4)
    ref = lambda x: None if x is None else C.byref(x)
    label = lambda d, st, tin, o: L.ts_rexpert_labels(ref(d), ref(st), ref(tin), ref(o), None)
    lin = lambda first=p, pos_log=p, table=p, count=p, slots=32, n_rows=4, steps=3: ec.RexpertLabelsIn(first, pos_log, table, count, None, slots, n_rows, steps, 0)
    out, none = ec.LabelsOut(p, p, p), ec.LabelsOut()
    bad_arg = lin(steps=0)
    assert label(None, None, None, None) == _cabi.ERR_NULL                                 # 1. dims
    assert label(_dims(0, 2), None, None, None) == _cabi.ERR_DIMS
    assert label(_dims(33, 2), None, None, None) == _cabi.ERR_LIMIT
    assert label(ok, None, None, out) == _cabi.ERR_NULL and label(ok, None, bad_arg, None) == _cabi.ERR_NULL   # 2. in, out
    for S, T, Tt in ((9, 1, 1), (4, 9, 9), (4, 2, 9)):                                     # 3. the shape
        assert label(_dims(S, T, 0, 8, Tt), None, bad_arg, none) == _cabi.ERR_LIMIT
    for tin in [lin(steps=0), lin(steps=-3), lin(steps=MAX_STEPS + 1), lin(n_rows=-1)] + [lin(slots=s) for s in (-2, 0, 1, 3, 48, (1 << 31) + 1)]:
        assert label(ok, None, tin, none) == _cabi.ERR_ARG                                 # 4. an argument
        assert label(_dims(5, 4, 0, 0), None, tin, none) == _cabi.ERR_ARG                  # also for an empty batch
    assert label(_dims(5, 4, 0, 0), None, lin(None, None, None, None), none) == _cabi.OK   # 5. nothing to launch
    assert label(ok, None, lin(), out) == _cabi.ERR_NULL                                   # 6. pointers
    assert label(ok, full, lin(), none) == _cabi.ERR_NULL                                  # no output at all
    for missing in ("tgt", "blk"):
        st = _cabi.State(None, None, p, p, None, None)
        setattr(st, missing, None)
        assert label(ok, st, lin(), out) == _cabi.ERR_NULL, missing
    for tin in (lin(first=None), lin(pos_log=None), lin(table=None), lin(count=None)):
        assert label(ok, full, tin, out) == _cabi.ERR_NULL
    assert L.ts_rexpert_last_hip_error() == 0
    # describe: NULL, dims, the shape, steps, what
    dl = lambda d, steps, what, desc=True: L.ts_describe_rexpert_labels(ref(d), steps, what, C.byref(ec.RexpertDesc()) if desc else None)
    assert dl(None, 0, 0) == _cabi.ERR_NULL and dl(ok, 0, 0, desc=False) == _cabi.ERR_NULL
    assert dl(_dims(0, 2), 0, 0) == _cabi.ERR_DIMS and dl(_dims(9, 1), 0, 0) == _cabi.ERR_LIMIT
    assert dl(ok, 0, 0) == dl(ok, MAX_STEPS + 1, 7) == dl(ok, 3, 0) == dl(ok, 3, 8) == _cabi.ERR_ARG
    assert dl(ok, 3, 7) == dl(ok, MAX_STEPS, 1) == _cabi.OK


def test_describe_on_both_sides_of_every_edge():
    from tiler_slider_amd import _rexpert_cabi as ec, _rollout_cabi as rc
    logs = rc.OUT_ACT_LOG | rc.OUT_FLAGS_LOG | rc.OUT_POS_LOG
    for S, T in ((5, 4), (8, 8), (1, 1), (4, 0)):
        for n, steps, blocks in ((0, 1, 0), (1, 0, 0), (1, 1, 1), (64, 3, 1), (65, 3, 1), (256, 3, 1), (257, 3, 2), (262141, 6, 1024)):
            d = ec.describe_rexpert_rollout(_dims(S, T, 0, n), _cfg(ec, steps=steps), logs)
            assert (d["blocks"], d["waves"], d["threads_per_block"], d["lds_bytes"]) == (blocks, 4 * blocks, 256, 0), (S, T, n, steps, d)
            assert d["name"] == (f"k_rexpert_rollout<{S}>" if blocks else "") and d["samples"] == n * steps
            assert d["bytes"] == (n * steps * (2 + T) if blocks else 0)
            assert ec.describe_rexpert_rollout(_dims(S, T, 0, n), _cfg(ec, steps=steps), rc.OUT_WINS | rc.OUT_ACT_LOG)["bytes"] == (n * steps if blocks else 0)
        for n, steps, blocks in ((0, 1, 0), (1, 1, 1), (64, 3, 3), (65, 3, 3), (257, 3, 6), (262141, 6, 6144)):
            d = ec.describe_rexpert_labels(_dims(S, T, 0, n), steps)
            assert (d["blocks"], d["waves"], d["threads_per_block"], d["lds_bytes"]) == (blocks, 4 * blocks, 256, 0), (S, T, n, steps, d)
            assert d["name"] == (f"k_rexpert_labels<{S}>" if blocks else "") and d["samples"] == n * steps and d["bytes"] == (4 * n * steps if blocks else 0)
            assert ec.describe_rexpert_labels(_dims(S, T, 0, n), steps, ec.LABELS_OUT_ACTION)["bytes"] == (n * steps if blocks else 0)


def test_the_code_object_holds_exactly_the_sixteen_kernels_describe_names():
    from tiler_slider_amd import _rexpert_cabi as ec
    named = {ec.describe_rexpert_rollout(_dims(S, min(T, S * S), mc), _cfg(ec, mode=mode))["name"] for S in range(1, 9) for T in (0, 1, 4, 8)
             for mc in (0, 1) for mode in (0, 1)}
    named |= {ec.describe_rexpert_labels(_dims(S, min(T, S * S), mc), 2)["name"] for S in range(1, 9) for T in (0, 1, 4, 8) for mc in (0, 1)}
    want = [f"k_rexpert_labels<{S}>" for S in range(1, 9)] + [f"k_rexpert_rollout<{S}>" for S in range(1, 9)]
    assert sorted(named) == want == _kernel_names(ec.LIB_PATH)


def test_the_kernels_use_no_scratch_no_lds_no_barrier_and_only_load_the_table():
    from tiler_slider_amd import _rexpert_cabi as ec
    meta = _kernel_metadata(ec.LIB_PATH)
    assert len(meta) == 16 == ec.MIN_KERNELS
    for k in meta:
        assert k["private_segment_fixed_size"] == 0 and not k["uses_dynamic_stack"] and k["agpr_count"] == 0, k
        assert k["group_segment_fixed_size"] == 0, k
        assert k["vgpr_count"] <= 128, k   # four waves a SIMD at least
    counts = _instruction_counts(ec.LIB_PATH, (r"\bv_\w+_f(16|32|64)\b", r"\bscratch_", r"\bs_barrier\b", r"\bglobal_atomic", r"\bds_"))
    assert len(counts) == 16
    for k, found in counts.items():
        assert found == [0, 0, 0, 0, 0], (k, found)


def test_occupancy_cases_name_exactly_the_compiled_kernels():
    """tests/test_gpu_rexpert.py runs one case per kernel at 4,096 waves or more: its case table (tests/rexpert_cases.py) is the
    code object's list, and the library plans the grids the GPU test relies on."""
    import reach_cases
    import rexpert_cases as cases
    from tiler_slider_amd import _rexpert_cabi as ec
    assert sorted(cases.CASES) == _kernel_names(ec.LIB_PATH) and len(cases.CASES) == ec.MIN_KERNELS == 16
    assert cases.N_BOARDS == 262141 and cases.N_BOARDS % 64 != 0 and -(-cases.N_BOARDS // 64) == cases.WAVES == 4096
    for name, (S, T, K) in cases.CASES.items():
        what = "rollout" if "rollout" in name else "labels"
        assert name == f"k_rexpert_{what}<{S}>" and (T, K) == reach_cases.SHAPES[S][:2]
        for mc in (0, 1):
            d = _dims(S, T, mc, cases.N_BOARDS)
            d.max_steps = cases.MAX_STEPS
            if what == "rollout":
                got = ec.describe_rexpert_rollout(d, _cfg(ec, steps=cases.STEPS, mode=1, slots=2048, n_rows=128))
                assert (got["name"], got["waves"]) == (name, cases.WAVES)
            else:
                got = ec.describe_rexpert_labels(d, cases.STEPS)
                assert got["name"] == name and got["waves"] >= cases.WAVES and got["samples"] == cases.STEPS * cases.N_BOARDS


@pytest.mark.parametrize("S", (2, 3, 4, 5, 6, 8))
@pytest.mark.parametrize("mode", (1, 0), ids=("autoreset", "strict"))
def test_the_base_case_is_not_degenerate(oracle, S, mode):
    """The caps against a vacuous pass that tests/test_gpu_rexpert.py asserts before any GPU call, here on the yardstick alone, in
    both colour modes, from 3x3 up: board-steps the expert chose, lookups of each of the five kinds, boards that win, auto-resets
    and timeouts."""
    import rexpert_reference as rx
    for mc in (False, True):
        want = rx.base_case(oracle, S, mc, mode)[4]
        s = rx.check_base(S, mode, want)
        print(S, mc, mode, s)
        assert want["source"].sum() == rx.BASE["levels"] * rx.BASE["steps"] == want["kinds"].sum()


@pytest.mark.parametrize("S", (2, 3, 4, 5, 6, 8))
def test_the_expert_case_has_levels_of_both_kinds(oracle, S):
    """Case 2 of the GPU tests: at least 11 levels whose root is 1 .. 32 moves from the win and, from 3x3 up, at least 10 whose root
    can never win; on the yardstick, without exploration and in strict mode, the first win their rollout of 32 steps comes exactly
    after root_moves steps."""
    import reach_cases as cases
    import rexpert_reference as rx
    import rtable_reference as rt
    for mc in (False, True):
        blk, init, tgt = cases.levels(oracle, S, mc)
        ref = rt.build(oracle, S, mc, blk, tgt, init, 252, cases.CAPACITY)
        near, never = (ref.root_moves >= 1) & (ref.root_moves <= 32), ref.root_moves == rt.SOLVE_NONE
        assert near.sum() >= 11 and (S < 3 or never.sum() >= 10), (S, mc, near.sum(), never.sum())
        want = rx.rollout(oracle, ref, S, mc, 64, blk, init, tgt, 32, 0, threshold=0, seed=7)
        np.testing.assert_array_equal(want["first_win"][near], ref.root_moves[near])
        assert (want["wins"][never] == 0).all()
