"""The trajectory targets without a GPU: the targets library's C-ABI (include/tiler_slider_targets.h), its launch plans, its code
object, and the CPU yardstick's own checks (tests/targets_reference.py): the restated reward, the coverage of its cases, the
returns' bound against float32 evaluations right and wrong, and the exact cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cabi_harness import _dims, _kernel_metadata, _kernel_names, _struct_fields
from conftest import ROOT
from tiler_slider_amd import _targets_cabi  # noqa: F401  every test here, the yardstick's self-checks included, belongs to the targets library

MAX_STEPS = 65535
NAN = float("nan")


def test_targets_library_exports_what_its_header_declares():
    from tiler_slider_amd import _targets_cabi as gc
    header = open(os.path.join(ROOT, "include", "tiler_slider_targets.h")).read()
    assert '#include "tiler_slider_train.h"' in header
    assert "BOTH SUCCESS AND TIMEOUT" in header and "NOT BUILT" in header and "NOT gamma-corrected" in header
    assert "NOT PART OF THE CONTRACT" in header and "reproducible bit for bit" in header
    for struct, cls in (("ts_returns_in", gc.ReturnsIn), ("ts_returns_out", gc.ReturnsOut), ("ts_labels_in", gc.LabelsIn),
                        ("ts_labels_out", gc.LabelsOut), ("ts_targets_desc", gc.TargetsDesc)):
        fields = _struct_fields(header, struct)   # "float gamma, lam" declares two
        assert fields == [f for f, _ in cls._fields_], struct
    assert (C.sizeof(gc.ReturnsIn), C.sizeof(gc.ReturnsOut), C.sizeof(gc.LabelsIn), C.sizeof(gc.LabelsOut), C.sizeof(gc.TargetsDesc)) == (80, 32, 48, 24, 112)
    for name, value in re.findall(r"#define (TS_(?:TARGETS|RETURNS|LABELS)_[A-Z_]+) (0x[0-9a-f]+|\d+)u?", header):
        if name != "TS_TARGETS_ABI_VERSION":
            assert getattr(gc, name[3:].replace("TARGETS_", "")) == int(value, 0), name
    import tiler_slider_amd as pkg
    assert callable(pkg.build_targets_library) and callable(pkg.VecTilerSliderEnv.trajectory_returns) and callable(pkg.VecTilerSliderEnv.trajectory_labels)
    assert pkg.RewardWeights() == (0.0, 1.0, 0.0, 0.0, 0.0, 0.0) and pkg.RewardWeights._fields == ("step", "win", "timeout", "invalid", "dist", "progress")
    assert pkg.TrajectoryReturns._fields == ("reward", "adv", "ret", "mask")
    assert {"RewardWeights", "TrajectoryReturns", "build_targets_library"} <= set(pkg.__all__)


def test_targets_supported_is_rollout_supported_and_table_states():
    """S 0 .. 10, T -1 .. 10, both colour modes (and an invalid one): the grid of the other libraries' tests."""
    from tiler_slider_amd import _cabi, _rollout_cabi as rc, _table_cabi as tc, _targets_cabi as gc
    L, LR, LT = gc.lib(), rc.lib(), tc.lib()
    seen = set()
    for S in range(0, 11):
        for T in range(-1, 11):
            for mc in (0, 1, 2):
                d = _dims(S, T, mc)
                ret, lab = L.ts_targets_supported(C.byref(d), gc.RETURNS), L.ts_targets_supported(C.byref(d), gc.LABELS)
                assert ret == LR.ts_rollout_supported(C.byref(d), rc.RANDOM), (S, T, mc)
                states = LT.ts_table_states(C.byref(d))
                assert lab == (states if states < 0 else int(states > 0)), (S, T, mc)
                seen.update((ret, lab))
                if ret < 0:
                    assert lab == ret
                    continue
                assert L.ts_targets_supported(C.byref(d), 2) == L.ts_targets_supported(C.byref(d), -1) == _cabi.ERR_ARG
                # the calls refuse exactly the unsupported shapes with TS_ERR_LIMIT: a supported one goes on to the missing flags_log / st
                rin, lin = gc.ReturnsIn(steps=1, value_stride=1), gc.LabelsIn(steps=1)
                assert L.ts_traj_returns(C.byref(d), None, C.byref(rin), C.byref(gc.ReturnsOut()), None) == (_cabi.ERR_NULL if ret else _cabi.ERR_LIMIT)
                assert L.ts_traj_labels(C.byref(d), None, C.byref(lin), C.byref(gc.LabelsOut()), None) == (_cabi.ERR_NULL if lab else _cabi.ERR_LIMIT)
                desc = gc.TargetsDesc()
                assert L.ts_describe_traj_returns(C.byref(d), 1, 1, C.byref(desc)) == (0 if ret else _cabi.ERR_LIMIT)
                assert L.ts_describe_traj_labels(C.byref(d), 1, 1, C.byref(desc)) == (0 if lab else _cabi.ERR_LIMIT)
    assert seen == {0, 1, _cabi.ERR_DIMS}
    for d in (_dims(4, 2, 0, Tt=8), _dims(4, 2, 0, Tt=9), _dims(33, 2), _dims(8, 3), _dims(3, 5), _dims(3, 6)):
        assert L.ts_targets_supported(C.byref(d), gc.RETURNS) == LR.ts_rollout_supported(C.byref(d), rc.RANDOM)
        assert L.ts_targets_supported(C.byref(d), gc.LABELS) == int(LT.ts_table_states(C.byref(d)) > 0)
    assert L.ts_targets_supported(None, 0) == _cabi.ERR_NULL
    assert gc.targets_supported(_dims(8, 8), gc.RETURNS) and not gc.targets_supported(_dims(8, 8), gc.LABELS)
    with pytest.raises(_cabi.TilerSliderLibraryError):
        gc.targets_supported(_dims(0, 1), gc.RETURNS)


def test_argument_validation_precedes_any_launch():
    """Every refusal below returns its own status, in the header's order: a HIP call on a box without a GPU would have answered
    TS_ERR_HIP."""
    from tiler_slider_amd import _cabi, _targets_cabi as gc
    L = gc.lib()
    ok, empty = _dims(4, 2), _dims(4, 2, 0, 0)
    buf = (C.c_uint8 * 8192)()
    p = (C.addressof(buf) + 15) & ~15
    full = _cabi.State(p, p, p, p, p, p)
    ref = lambda x: C.byref(x) if x is not None else None

    def rin(steps=3, stride=1, gamma=0.9, lam=0.9, dist=1.0, progress=1.0, **kw):
        a = dict(first=p, pos_log=p, flags_log=p, values=p, last_value=p)
        a.update(kw)
        return gc.ReturnsIn(a["first"], a["pos_log"], a["flags_log"], a["values"], a["last_value"], steps, stride, gamma, lam, 0.0, 1.0, 0.0, 0.0, dist, progress)

    def lin(steps=3, n_rows=8, **kw):
        a = dict(first=p, pos_log=p, table=p, rows=p)
        a.update(kw)
        return gc.LabelsIn(a["first"], a["pos_log"], a["table"], a["rows"], n_rows, steps, 0)

    rout, lout = gc.ReturnsOut(p, p, p, p), gc.LabelsOut(p, p, p)
    ret = lambda d, st, i, o=rout: L.ts_traj_returns(ref(d), ref(st), ref(i), ref(o), None)
    lab = lambda d, st, i, o=lout: L.ts_traj_labels(ref(d), ref(st), ref(i), ref(o), None)
    both = lambda d, st, ri, li, ro=rout, lo=lout: (ret(d, st, ri, ro), lab(d, st, li, lo))
    same = lambda code: (code, code)
    # 1. dims - its TS_ERR_LIMIT before the NULL checks
    assert both(None, full, rin(), lin()) == same(_cabi.ERR_NULL)
    assert both(_dims(0, 2), full, None, None, None, None) == same(_cabi.ERR_DIMS)
    assert both(_dims(33, 2), full, None, None, None, None) == same(_cabi.ERR_LIMIT)
    # 2. in / out
    assert both(ok, full, None, None) == same(_cabi.ERR_NULL)
    assert both(ok, full, rin(), lin(), None, None) == same(_cabi.ERR_NULL)
    assert both(_dims(9, 1), full, None, None) == same(_cabi.ERR_NULL)
    # 3. unsupported shape, before the arguments
    assert both(_dims(9, 1), full, rin(0), lin(0)) == same(_cabi.ERR_LIMIT)
    assert ret(_dims(4, 2, Tt=9), full, rin(0)) == _cabi.ERR_LIMIT and ret(_dims(8, 9), full, rin(0)) == _cabi.ERR_LIMIT
    assert lab(_dims(8, 3), full, lin(0)) == _cabi.ERR_LIMIT and ret(_dims(8, 3), None, rin()) == _cabi.ERR_NULL
    # 4. bad arguments, before the empty batch and before any pointer
    for steps in (0, -1, MAX_STEPS + 1, 2**31 - 1):
        for d in (ok, empty):
            assert both(d, None, rin(steps), lin(steps), gc.ReturnsOut(), gc.LabelsOut()) == same(_cabi.ERR_ARG), steps
        for fn in (L.ts_describe_traj_returns, L.ts_describe_traj_labels):
            assert fn(C.byref(ok), steps, 1, C.byref(gc.TargetsDesc())) == _cabi.ERR_ARG
    for bad in (dict(gamma=-0.001), dict(gamma=1.001), dict(gamma=NAN), dict(lam=-0.001), dict(lam=1.5), dict(lam=NAN), dict(stride=0), dict(stride=2),
                dict(stride=3), dict(stride=8), dict(stride=-1)):
        for d in (ok, empty):
            assert ret(d, None, rin(**bad), gc.ReturnsOut()) == _cabi.ERR_ARG, bad
    assert lab(ok, None, lin(n_rows=-1), gc.LabelsOut()) == _cabi.ERR_ARG and lab(empty, None, lin(n_rows=-1), gc.LabelsOut()) == _cabi.ERR_ARG
    for edge in (dict(gamma=0.0, lam=0.0), dict(gamma=1.0, lam=1.0, stride=4), dict(steps=MAX_STEPS), dict(steps=1)):   # the edges are arguments
        assert ret(ok, None, rin(**edge), gc.ReturnsOut()) == _cabi.ERR_NULL, edge
    assert lab(ok, None, lin(MAX_STEPS, 0), gc.LabelsOut()) == _cabi.ERR_NULL
    # 5. nothing to do: TS_OK without a launch, no further pointer is looked at
    assert both(empty, None, gc.ReturnsIn(steps=1, value_stride=1), gc.LabelsIn(steps=1), gc.ReturnsOut(), gc.LabelsOut()) == same(_cabi.OK)
    # 6. missing pointers, before the alignment
    odd = dict(values=p + 2)
    assert ret(ok, full, rin(flags_log=None, **odd)) == _cabi.ERR_NULL
    assert ret(ok, full, rin(pos_log=None, **odd)) == _cabi.ERR_NULL and ret(ok, full, rin(first=None, **odd)) == _cabi.ERR_NULL
    assert ret(ok, None, rin(**odd)) == _cabi.ERR_NULL and ret(ok, _cabi.State(p, p, None, p, p, p), rin(**odd)) == _cabi.ERR_NULL
    assert ret(ok, full, rin(**odd), gc.ReturnsOut()) == _cabi.ERR_NULL
    assert lab(ok, None, lin()) == _cabi.ERR_NULL and lab(ok, _cabi.State(p, p, p, None, p, p), lin()) == _cabi.ERR_NULL
    assert lab(ok, full, lin(first=None)) == _cabi.ERR_NULL and lab(ok, full, lin(pos_log=None)) == _cabi.ERR_NULL
    assert lab(ok, full, lin(table=None)) == _cabi.ERR_NULL and lab(ok, full, lin(), gc.LabelsOut()) == _cabi.ERR_NULL
    # ... and what may be missing: the alignment check is reached
    assert ret(ok, full, rin(progress=0.0, first=None, **odd)) == _cabi.ERR_ARG                      # no w_progress: no first
    assert ret(ok, None, rin(dist=0.0, progress=0.0, first=None, pos_log=None, **odd)) == _cabi.ERR_ARG     # no distance weight: no cells, no level
    assert ret(_dims(4, 0), None, rin(first=None, pos_log=None, **odd)) == _cabi.ERR_ARG             # no tiles: no cells
    assert ret(_dims(4, 2, Tt=0), None, rin(**odd)) == _cabi.ERR_ARG                                 # no targets: no tgt
    assert ret(ok, _cabi.State(None, None, p, None, None, None), rin(**odd)) == _cabi.ERR_ARG        # blk is never read
    # 7. a float pointer that is not 4-byte aligned
    for off in (1, 2, 3):
        for name in ("values", "last_value"):
            assert ret(ok, full, rin(**{name: p + off})) == _cabi.ERR_ARG, (name, off)
        for name in ("reward", "adv", "ret"):
            o = gc.ReturnsOut(p, p, p, p)
            setattr(o, name, p + off)
            assert ret(ok, full, rin(), o) == _cabi.ERR_ARG, (name, off)
    assert L.ts_targets_last_hip_error() == 0
    for fn in (L.ts_describe_traj_returns, L.ts_describe_traj_labels):
        assert fn(None, 1, 1, C.byref(gc.TargetsDesc())) == _cabi.ERR_NULL and fn(C.byref(ok), 1, 1, None) == _cabi.ERR_NULL
        assert fn(C.byref(ok), 1, 0, C.byref(gc.TargetsDesc())) == _cabi.ERR_ARG and fn(C.byref(ok), 1, 0x100, C.byref(gc.TargetsDesc())) == _cabi.ERR_ARG
    assert L.ts_describe_traj_labels(C.byref(ok), 1, 0x8, C.byref(gc.TargetsDesc())) == _cabi.ERR_ARG
    assert L.ts_describe_traj_returns(C.byref(ok), 1, 0xf0, C.byref(gc.TargetsDesc())) == _cabi.ERR_ARG      # inputs alone: no output asked
    for describe in (gc.describe_traj_returns, gc.describe_traj_labels):
        got = describe(empty, 7)
        assert (got["blocks"], got["name"], got["samples"], got["bytes_read"], got["bytes_written"]) == (0, "", 0, 0, 0)


def test_describe_names_exactly_the_compiled_kernels_and_counts_the_bytes():
    from tiler_slider_amd import _targets_cabi as gc
    compiled = _kernel_names(gc.LIB_PATH)
    assert len(compiled) == gc.MIN_KERNELS == 16
    named = set()
    for S in range(1, 9):
        for T in range(0, min(S * S, 8) + 1):
            for mc in (0, 1):
                for n, K in ((1, 1), (257, 5), (1 << 20, 100)):
                    d = _dims(S, T, mc, n)
                    r = gc.describe_traj_returns(d, K, 0xff)
                    assert r["name"] == f"k_traj_returns<{S}>" and r["samples"] == n * K and r["blocks"] == -(-n // 256)
                    assert (r["threads_per_block"], r["lds_bytes"], r["chunk_steps"]) == (256, 0, 4)
                    assert r["bytes_written"] == 13 * n * K                                  # three floats and a byte
                    assert r["bytes_read"] == n * K + ((K + 1) * T * n + T * n) + 4 * n * K + 4 * n   # flags; cells, first, targets; values; last_value
                    bare = gc.describe_traj_returns(d, K, gc.RETURNS_OUT_MASK)
                    assert (bare["bytes_read"], bare["bytes_written"]) == (n * K, n * K)
                    dist = gc.describe_traj_returns(d, K, gc.RETURNS_OUT_RET | gc.RETURNS_IN_CELLS)
                    assert (dist["bytes_read"], dist["bytes_written"]) == (n * K + K * T * n + T * n, 4 * n * K)
                    named.add(r["name"])
                    if not gc.targets_supported(d, gc.LABELS):
                        continue
                    lb = gc.describe_traj_labels(d, K)
                    assert lb["name"] == f"k_traj_labels<{S}>" and lb["samples"] == n * K and lb["blocks"] == -(-n // 256)
                    assert (lb["threads_per_block"], lb["lds_bytes"], lb["chunk_steps"]) == (256, 0, 4)
                    words = 2 if S * S > 32 else 1
                    assert (lb["bytes_read"], lb["bytes_written"]) == (K * T * n + 5 * n * K + 4 * words * n, 4 * n * K)
                    mv = gc.describe_traj_labels(d, K, gc.LABELS_OUT_MOVES)
                    assert (mv["bytes_read"], mv["bytes_written"]) == (K * T * n + n * K + 4 * words * n, 2 * n * K)
                    named.add(lb["name"])
    assert sorted(named) == compiled
    import targets_reference as gr
    assert sorted(gr.OCCUPANCY_CASES) == compiled      # tests/test_gpu_targets.py runs one case per kernel at 4,096 waves


def test_every_targets_kernel_keeps_its_board_in_registers_and_uses_no_lds():
    """The code object's own metadata: no private segment (scratch), no static LDS (and the describe calls report no dynamic LDS
    either), no accumulation registers (the hazard scan skips kernels that use them), no dynamic stack."""
    from tiler_slider_amd import _targets_cabi as gc
    kernels = _kernel_metadata(gc.LIB_PATH)
    assert len(kernels) == len([k for k in kernels if "k_traj_" in k["name"]]) == gc.MIN_KERNELS
    assert not any(k["group_segment_fixed_size"] or k["private_segment_fixed_size"] or k["agpr_count"] or k["uses_dynamic_stack"] for k in kernels), kernels


# ---------------------------------------------------------------------------------------------- the yardstick itself
def test_the_restated_reward_is_the_oracles_on_every_shape(oracle):
    """m() on NumPy against OracleBatch.reward() on random cells: single and multi colour, T != Tt, repeated targets, no tiles,
    1x1, and cell ids beyond the board (the oracle is handed the clipped ids)."""
    import targets_reference as gr
    rng = np.random.default_rng(2)
    for S, T, Tt, mc in ((4, 2, 2, False), (5, 3, 3, True), (8, 8, 8, True), (8, 8, 8, False), (3, 2, 3, True), (3, 3, 1, False), (3, 3, 2, True),
                         (4, 0, 2, False), (4, 2, 0, False), (1, 1, 1, True), (6, 5, 8, False)):
        n, Cc = 300, S * S
        cells, tgt = rng.integers(0, 256, (T, n)).astype(np.uint8), rng.integers(0, Cc, (Tt, n)).astype(np.uint8)
        if Tt > 1:
            tgt[1, ::3] = tgt[0, ::3]      # repeated targets
        clipped = np.minimum(cells, Cc - 1).astype(np.uint8)
        b = oracle.OracleBatch(S, mc, 100, np.zeros((oracle.blk_words(S), n), np.uint32), clipped, tgt)
        b.pos[...] = clipped
        want = b.reward()
        np.testing.assert_array_equal(gr.m_of(S, mc, cells, tgt), want, err_msg=str((S, T, Tt, mc)))
        assert (want <= 0).all() and (T == 0 or Tt == 0 or S == 1 or (want < 0).any())


def test_the_cases_cover_what_they_are_for(oracle):
    """Asserted on the yardstick's own numbers: the main auto-reset case has SUCCESS, TIMEOUT, AUTORESET and INVALID_MOVE on at least
    1 % of its board-steps each, the strict case stands done on at least 10 %, the given case has BAD_ACTION on 5 % - and in
    every case sum_k m(pos_log[k]) is the rollout's reward_sum (trajectory() asserts it)."""
    import targets_reference as gr
    auto = gr.trajectory(oracle, "auto")["log"]["flags_log"]
    shares = [gr.share(auto, bit) for bit in (gr.FLAG_SUCCESS, gr.FLAG_TIMEOUT, gr.FLAG_AUTORESET, gr.FLAG_INVALID_MOVE)]
    print("auto: SUCCESS, TIMEOUT, AUTORESET, INVALID_MOVE shares", [round(s, 3) for s in shares])
    assert min(shares) >= 0.01
    strict = gr.trajectory(oracle, "strict")["log"]["flags_log"]
    print("strict: STEPPED_DONE share", round(gr.share(strict, gr.FLAG_STEPPED_DONE), 3))
    assert gr.share(strict, gr.FLAG_STEPPED_DONE) >= 0.10 and gr.share(strict, gr.FLAG_AUTORESET) == 0
    given = gr.trajectory(oracle, "given")
    assert 0.04 <= float((given["actions"] > 3).mean()) <= 0.06 and gr.share(given["log"]["flags_log"], gr.FLAG_BAD_ACTION) >= 0.02
    for name in ("mc5", "s8", "long"):
        f = gr.trajectory(oracle, name)["log"]["flags_log"]
        assert gr.share(f, gr.END) > 0 and gr.share(f, gr.VOID) > 0, name
    lab = gr.labels(oracle, 4, given["blk"], given["first"], given["log"]["pos_log"], given["table"])
    assert (lab[2] != 255).mean() > 0.01 and (lab[2] == 255).mean() > 0.01 and lab[0].max() > 1


@pytest.mark.parametrize("name", ("auto", "long", "strict"))
def test_the_returns_bound_holds_a_float32_evaluation_and_notices_two_wrong_ones(oracle, name):
    """gamma = 0.97, lambda = 0.9, Gaussian values, every weight set: a float32 NumPy evaluation lies within the bound of the
    float64 one on every sample, void steps are exactly 0, and an evaluation that ignores the ends of episodes, or uses gamma
    for gamma * lambda, leaves the bound on more than half of the live samples."""
    import targets_reference as gr
    c = gr.trajectory(oracle, name)
    f, mb, ma = c["log"]["flags_log"], c["m_before"], c["m_after"]
    V, VL = gr.gaussian_values(c["K"], c["n"])
    w = gr.Weights(step=-0.01, win=1.0, timeout=-0.5, invalid=-0.1, dist=0.05, progress=0.25)
    want = gr.returns64(f, mb, ma, V, VL, 0.97, 0.9, w)
    live = want["mask"] != 0
    assert 0.2 < live.mean() < 1.0

    def worst(got):
        ratios = []
        for key in ("reward", "adv", "ret"):
            assert got[key].dtype == np.float32
            err = np.abs(got[key].astype(np.float64) - want[key])
            assert (got[key][~live] == 0).all()
            ratios.append(err[live] / want["bound"][live])
        return ratios

    right = worst(gr.returns32(f, mb, ma, V, VL, 0.97, 0.9, w))
    print(f"{name}: worst float32 error / bound {max(r.max() for r in right):.3f}")
    assert max(r.max() for r in right) <= 1.0 and max(r.max() for r in right) > 1e-3
    for wrong in (dict(ignore_ends=True), dict(gamma_for_gl=True)):
        beyond = float((worst(gr.returns32(f, mb, ma, V, VL, 0.97, 0.9, w, **wrong))[1] > 1.0).mean())
        print(f"{name}: {wrong} is beyond the bound on {beyond:.1%} of the live samples")
        assert beyond > 0.5, wrong
    assert np.array_equal(gr.returns32(f, mb, ma, V, VL, 0.97, 0.9, w)["mask"], want["mask"])


@pytest.mark.parametrize("gamma", (1.0, 0.5))
@pytest.mark.parametrize("name", ("auto", "strict", "given"))
def test_the_exact_cases_survive_float32(oracle, name, gamma):
    """Integer weights, integer values in -8 .. 8, lambda = 1, max_steps 6, K = 24: every intermediate of the float64 recursion
    is a float32 (asserted inside), so the float32 evaluation gives the same bits in any order."""
    import targets_reference as gr
    c = gr.trajectory(oracle, name)
    assert c["max_steps"] == 6 and c["K"] <= 24
    V, VL = gr.integer_values(c["K"], c["n"])
    want = gr.returns64(c["log"]["flags_log"], c["m_before"], c["m_after"], V, VL, gamma, 1.0, gr.INT_WEIGHTS, exact=True)
    got = gr.returns32(c["log"]["flags_log"], c["m_before"], c["m_after"], V, VL, gamma, 1.0, gr.INT_WEIGHTS)
    for key in ("reward", "adv", "ret"):
        np.testing.assert_array_equal(got[key].astype(np.float64), want[key])
        assert np.abs(want[key]).max() > 0
    # without values and with lambda = 1, ret is the discounted return-to-go: restated as a plain loop over one board's episodes
    plain = gr.returns64(c["log"]["flags_log"], c["m_before"], c["m_after"], None, None, gamma, 1.0, gr.INT_WEIGHTS)
    n0, f = 3, c["log"]["flags_log"]
    togo = 0.0
    for k in range(c["K"] - 1, -1, -1):
        if f[k, n0] & gr.VOID:
            assert plain["ret"][k, n0] == 0
            continue
        togo = plain["reward"][k, n0] + (0.0 if f[k, n0] & gr.END else gamma * togo)
        assert plain["ret"][k, n0] == togo == plain["adv"][k, n0]
