"""The fused rollouts without a GPU: the rollout library's C-ABI (include/tiler_slider_rollout.h), its launch plan, its code
object, and the CPU yardstick (tests/rollout_reference.py) against the optimal move counts already in git."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cabi_harness import _dims, _instruction_counts, _kernel_metadata, _kernel_names
from conftest import GOLDEN_DIR, ROOT


def _cfg(steps=4, policy=1, mode=0, write_state=1, **kw):
    from tiler_slider_amd import _rollout_cabi as rc
    c = rc.RolloutCfg(steps, mode, policy, write_state, None, 0, 0, 0, 0, None, 0, None)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_rollout_library_exports_what_its_header_declares():
    from tiler_slider_amd import _rollout_cabi
    header = open(os.path.join(ROOT, "include", "tiler_slider_rollout.h")).read()
    assert '#include "tiler_slider_table.h"' in header
    for name, value in (("TS_ROLLOUT_MAX_STEPS", _rollout_cabi.ROLLOUT_MAX_STEPS),
                        ("TS_ROLLOUT_MAX_SIZE", _rollout_cabi.ROLLOUT_MAX_SIZE), ("TS_ROLLOUT_MAX_TILES", _rollout_cabi.ROLLOUT_MAX_TILES),
                        ("TS_ROLLOUT_GIVEN", _rollout_cabi.GIVEN), ("TS_ROLLOUT_RANDOM", _rollout_cabi.RANDOM), ("TS_ROLLOUT_TABLE", _rollout_cabi.TABLE)):
        assert int(re.search(rf"#define {name} \(?(-?\d+)\)?", header).group(1)) == value, name
    bits = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define TS_ROLLOUT_OUT_([A-Z_]+) (0x[0-9a-f]+)u", header)}
    assert [bits[f.upper()] for f in _rollout_cabi.OUT_FIELDS] == [1 << i for i in range(9)]
    assert all(getattr(_rollout_cabi, "OUT_" + k) == v for k, v in bits.items())
    assert (_rollout_cabi.GIVEN, _rollout_cabi.RANDOM, _rollout_cabi.TABLE, _rollout_cabi.ROLLOUT_MAX_STEPS) == (0, 1, 2, 65535)
    # the fields the issue names, in the binding's structures
    assert [f for f, _ in _rollout_cabi.RolloutCfg._fields_] == ["steps", "mode", "policy", "write_state", "actions", "seed", "step_index", "board_offset",
                                                                 "explore_threshold", "table", "n_rows", "rows"]
    assert [f for f, _ in _rollout_cabi.RolloutOut._fields_] == ["wins", "finished", "first_win", "win_moves", "reward_sum", "flags", "act_log",
                                                                 "flags_log", "pos_log"]
    import tiler_slider_amd
    assert tiler_slider_amd.Rollout is not None and callable(tiler_slider_amd.build_rollout_library)
    assert callable(tiler_slider_amd.VecTilerSliderEnv.rollout)


def test_rollout_supported_over_the_grid_and_the_table_rule_is_the_tables():
    """S 0 .. 10, T -1 .. 10, both colour modes (and an invalid one), the three policies: registers hold boards up to 8x8 with at
    most 8 tiles and targets; the table policy is supported exactly where ts_table_states is positive."""
    from tiler_slider_amd import _cabi, _rollout_cabi, _table_cabi
    L, LT = _rollout_cabi.lib(), _table_cabi.lib()
    seen = set()
    for S in range(0, 11):
        for T in range(-1, 11):
            for mc in (0, 1, 2):
                d = _dims(S, T, mc)
                invalid = S < 1 or T < 0 or mc == 2 or T > S * S
                for policy in (_rollout_cabi.GIVEN, _rollout_cabi.RANDOM, _rollout_cabi.TABLE):
                    got = L.ts_rollout_supported(C.byref(d), policy)
                    if invalid:
                        assert got == _cabi.ERR_DIMS, (S, T, mc, policy)
                        continue
                    fits = S <= 8 and T <= 8
                    if policy == _rollout_cabi.TABLE:
                        assert (got == 1) == (LT.ts_table_states(C.byref(d)) > 0) and got in (0, 1), (S, T, mc)
                        assert got == int(fits and (S * S) ** T <= 65536)
                    else:
                        assert got == int(fits), (S, T, mc, policy)
                    seen.add((policy, got))
                    # ts_rollout and ts_describe_rollout refuse exactly the unsupported shapes with TS_ERR_LIMIT
                    rc = L.ts_rollout(C.byref(d), None, C.byref(_cfg(policy=policy)), None, None)
                    assert rc == (_cabi.ERR_NULL if got == 1 else _cabi.ERR_LIMIT), (S, T, mc, policy, rc)
                assert L.ts_rollout_supported(C.byref(d), 3) == (_cabi.ERR_DIMS if invalid else _cabi.ERR_ARG)
    assert seen == {(p, g) for p in (0, 1, 2) for g in (0, 1)}
    # more targets than a lane keeps, with few tiles
    assert L.ts_rollout_supported(C.byref(_dims(4, 2, 0, Tt=8)), 2) == 1 and L.ts_rollout_supported(C.byref(_dims(4, 2, 0, Tt=9)), 2) == 0
    assert L.ts_rollout_supported(C.byref(_dims(33, 2)), 1) == 0 and L.ts_rollout_supported(None, 1) == _cabi.ERR_NULL
    assert _rollout_cabi.rollout_supported(_dims(8, 8), 1) and not _rollout_cabi.rollout_supported(_dims(8, 8), 2)
    with pytest.raises(_cabi.TilerSliderLibraryError):
        _rollout_cabi.rollout_supported(_dims(0, 1), 1)


def test_argument_validation_precedes_any_launch():
    """Every refusal below returns its own status: a HIP call on this GPU-less box would have answered TS_ERR_HIP."""
    from tiler_slider_amd import _cabi, _rollout_cabi as rc
    L = rc.lib()
    ok = _dims(4, 2)
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    full = _cabi.State(p, p, p, p, p, p)
    outs = rc.RolloutOut(*([p] * 9))
    run = lambda d, st, cfg, out: L.ts_rollout(C.byref(d) if d is not None else None, C.byref(st) if st is not None else None,
                                               C.byref(cfg) if cfg is not None else None, C.byref(out) if out is not None else None, None)
    assert run(None, full, _cfg(), outs) == _cabi.ERR_NULL
    assert run(ok, full, None, outs) == _cabi.ERR_NULL
    assert run(_dims(0, 2), full, _cfg(), outs) == _cabi.ERR_DIMS
    # unsupported shapes
    for S, T, policy in ((9, 1, 1), (16, 2, 0), (8, 9, 1), (5, 4, 2), (8, 3, 2)):
        assert run(_dims(S, T), full, _cfg(policy=policy), outs) == _cabi.ERR_LIMIT
        assert L.ts_describe_rollout(C.byref(_dims(S, T)), C.byref(_cfg(policy=policy)), 0, C.byref(rc.RolloutDesc())) == _cabi.ERR_LIMIT
    assert run(_dims(4, 2, Tt=9), full, _cfg(), outs) == _cabi.ERR_LIMIT
    # bad arguments: mode bits, policy, steps, threshold, n_rows
    bad = (_cfg(mode=2), _cfg(mode=0x80000000), _cfg(policy=3), _cfg(policy=-1), _cfg(steps=-1), _cfg(steps=65536), _cfg(steps=2**31 - 1),
           _cfg(policy=2, explore_threshold=2**32 + 1), _cfg(policy=2, explore_threshold=2**64 - 1), _cfg(policy=2, n_rows=-1))
    for cfg in bad:
        assert run(ok, full, cfg, outs) == _cabi.ERR_ARG, (cfg.mode, cfg.policy, cfg.steps, cfg.explore_threshold, cfg.n_rows)
    assert run(ok, full, _cfg(steps=65535, policy=2, explore_threshold=2**32, table=p, n_rows=1), None) == _cabi.ERR_NULL  # the edges are arguments
    # the order: unsupported shape, then bad argument, then missing pointer
    assert run(_dims(9, 1), None, _cfg(steps=-1), None) == _cabi.ERR_LIMIT
    assert run(_dims(5, 4), None, _cfg(policy=2, steps=-1), None) == _cabi.ERR_LIMIT
    assert run(ok, None, _cfg(steps=-1), None) == _cabi.ERR_ARG
    assert run(ok, None, _cfg(), None) == _cabi.ERR_NULL
    # missing pointers
    assert run(ok, None, _cfg(), outs) == _cabi.ERR_NULL
    assert run(ok, full, _cfg(), None) == _cabi.ERR_NULL
    for missing in ("pos", "tgt", "blk", "step_count", "done"):
        st = _cabi.State(p, p, p, p, p, p)
        setattr(st, missing, None)
        assert run(ok, st, _cfg(), outs) == _cabi.ERR_NULL, missing
    no_init = _cabi.State(p, None, p, p, p, p)
    assert run(ok, no_init, _cfg(mode=1), outs) == _cabi.ERR_NULL                      # auto-reset reads the initial cells
    assert run(ok, full, _cfg(policy=0), outs) == _cabi.ERR_NULL                       # GIVEN without actions
    assert run(ok, full, _cfg(policy=2, n_rows=3), outs) == _cabi.ERR_NULL             # TABLE: three rows of no table
    assert run(ok, full, _cfg(write_state=0), rc.RolloutOut()) == _cabi.ERR_NULL       # neither an output nor write_state
    # nothing to do: TS_OK without a launch, no pointer is looked at
    empty = _dims(4, 2, 0, 0)
    assert run(empty, None, _cfg(), None) == _cabi.OK
    assert run(empty, full, _cfg(steps=-1), outs) == _cabi.ERR_ARG
    assert run(ok, None, _cfg(steps=0), None) == _cabi.OK
    assert run(ok, full, _cfg(steps=0, policy=0), outs) == _cabi.OK
    assert L.ts_rollout_last_hip_error() == 0
    assert L.ts_describe_rollout(None, C.byref(_cfg()), 0, C.byref(rc.RolloutDesc())) == _cabi.ERR_NULL
    assert L.ts_describe_rollout(C.byref(ok), None, 0, C.byref(rc.RolloutDesc())) == _cabi.ERR_NULL
    assert L.ts_describe_rollout(C.byref(ok), C.byref(_cfg()), 0, None) == _cabi.ERR_NULL
    for d, cfg in ((empty, _cfg()), (ok, _cfg(steps=0))):
        got = rc.describe_rollout(d, cfg, 0x1ff)
        assert (got["blocks"], got["name"], got["logged_bytes"], got["lds_bytes"]) == (0, "", 0, 0)


def _supported_shapes():
    from tiler_slider_amd import _rollout_cabi as rc
    for S in range(1, 9):
        for T in range(0, min(S * S, 8) + 1):
            for policy in (rc.GIVEN, rc.RANDOM, rc.TABLE):
                if rc.lib().ts_rollout_supported(C.byref(_dims(S, T)), policy) == 1:
                    yield S, T, policy


def test_describe_rollout_names_exactly_the_compiled_kernels():
    """Every kernel of the rollout library's code object is what some supported call launches, and every launch names a kernel
    that exists: no compiled form that no call reaches, none missing.  One board per lane, four waves per block, no LDS."""
    from tiler_slider_amd import _rollout_cabi as rc
    compiled = _kernel_names(rc.LIB_PATH)
    assert len(compiled) == rc.MIN_KERNELS == 24
    named = set()
    for S, T, policy in _supported_shapes():
        for n in (1, 257, 1 << 20):
            for mc in (0, 1):
                for steps, mask in ((1, 0), (100, rc.OUT_ACT_LOG | rc.OUT_POS_LOG), (65535, 0x1ff)):
                    d = rc.describe_rollout(_dims(S, T, mc, n), _cfg(steps=steps, policy=policy, mode=mc), mask)
                    assert d["name"] == f"k_rollout<{S}, {policy}>"
                    assert (d["threads_per_block"], d["lds_bytes"], d["blocks"]) == (256, 0, -(-n // 256))
                    per_step = bool(mask & rc.OUT_ACT_LOG) + bool(mask & rc.OUT_FLAGS_LOG) + (T if mask & rc.OUT_POS_LOG else 0)
                    assert d["logged_bytes"] == per_step * steps * n
                    named.add(d["name"])
    assert sorted(named) == compiled
    import rollout_reference as rref
    assert sorted(rref.OCCUPANCY_CASES) == compiled      # tests/test_gpu_rollout.py runs one case per kernel at 4,096 waves
    for name, (S, T, K, policy) in rref.OCCUPANCY_CASES.items():
        assert rc.describe_rollout(_dims(S, T, 0, 4096 * 64), _cfg(policy=policy), 0)["name"] == name
        assert rc.describe_rollout(_dims(S, T, 0, 4096 * 64), _cfg(policy=policy), 0)["blocks"] * 4 >= 4096


def test_every_rollout_kernel_keeps_its_board_in_registers():
    """The code object's own metadata and instructions: no LDS, no private segment (scratch), no s_barrier, no ds_ and no
    scratch_ instruction in any of the 24 kernels."""
    from tiler_slider_amd import _rollout_cabi as rc
    kernels = _kernel_metadata(rc.LIB_PATH)
    assert len(kernels) == len([k for k in kernels if "k_rollout" in k["name"]]) == rc.MIN_KERNELS
    assert not any(k["group_segment_fixed_size"] or k["private_segment_fixed_size"] or k["uses_dynamic_stack"] for k in kernels), kernels
    counts = _instruction_counts(rc.LIB_PATH, (r"\b(s_barrier|ds_\w+|scratch_\w+)\b",))
    mine = {k: v[0] for k, v in counts.items() if "k_rollout" in k}
    assert len(mine) == rc.MIN_KERNELS and not any(mine.values()), mine


def test_restated_mix64_reproduces_the_oracles_action_stream(oracle):
    import rollout_reference as rref
    for seed, step, off, n in ((0, 0, 0, 257), (0xAC710005, 7, 0, 1000), (2**64 - 1, 2**40, 123456789, 513), (0x5EED, 65534, 2**33, 64)):
        r = rref.draws(n, seed, step, off)
        np.testing.assert_array_equal((r >> np.uint64(62)).astype(np.uint8), oracle.fill_actions(n, seed=seed, step_index=step, board_offset=off))
    low = rref.draws(1 << 16, 1, 2) & np.uint64(0xffffffff)
    assert 0.24 < (low < np.uint64(rref.threshold_of(0.25))).mean() < 0.26       # the explore bits are spread like a fraction
    assert rref.threshold_of(0.0) == 0 and rref.threshold_of(1.0) == 2**32


def test_yardstick_expert_wins_the_400_screenshot_levels_in_their_recorded_optimum(oracle):
    """tests/rollout_reference.py against numbers already in git: the table policy without exploration, strict mode, as many steps
    as the deepest level needs - every level is won exactly once, at step min_moves, with min_moves on its counter."""
    import rollout_reference as rref
    import solver_reference as ref
    import table_reference as tref
    from tiler_slider_amd.levels import pack_levels
    total = 0
    for (S, T, mc), (ids, blk, init, tgt, want) in ref.fixture_groups(GOLDEN_DIR, pack_levels).items():
        tab = tref.table(oracle, S, mc, blk, tgt, T)
        steps = int(want.max())
        got = rref.rollout(oracle, S, mc, 100, blk, init, tgt, steps, rref.TABLE, 0, table=tab, threshold=0, seed=0x5EED)
        np.testing.assert_array_equal(got["first_win"], want, err_msg=str((S, T, mc)))
        np.testing.assert_array_equal(got["win_moves"], want)
        assert (got["wins"] == 1).all() and (got["finished"] == 1).all() and got["done"].all()
        np.testing.assert_array_equal(got["step_count"], want)
        assert got["source"][1] == 0                                              # nothing explored
        # after its win a board is done: STEPPED_DONE in the log, its cells unchanged
        late = np.arange(1, steps + 1)[:, None] > want[None, :]
        assert (got["flags_log"][late] == rref.FLAG_STEPPED_DONE).all()
        assert (got["pos_log"][-1] == got["pos"]).all()
        total += len(ids)
    assert total == 400
