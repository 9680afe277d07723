"""The in-place step without a GPU: the update library's C-ABI (include/tiler_slider_update.h), what it takes and refuses before any
launch, its launch record and its code object."""
import ctypes as C
import os
import re

import pytest

import update_cases as cases
from cabi_harness import _declared, _dims, _instruction_counts, _kernel_metadata, _kernel_names
from conftest import ROOT


def test_update_library_exports_what_its_header_declares():
    from tiler_slider_amd import _cabi, _update_cabi as uc
    L = uc.lib()
    assert len(_declared("tiler_slider_update.h")) == 5
    header = open(os.path.join(ROOT, "include", "tiler_slider_update.h")).read()
    assert '#include "tiler_slider.h"' in header
    assert int(re.search(r"#define TS_UPDATE_MAX_SIZE (\d+)", header).group(1)) == uc.UPDATE_MAX_SIZE == 8
    assert int(re.search(r"#define TS_UPDATE_MAX_TILES (\d+)", header).group(1)) == uc.UPDATE_MAX_TILES == 8
    assert int(re.search(r"#define TS_KERNEL_UPDATE (\d+)", header).group(1)) == uc.KERNEL_UPDATE
    assert _cabi.KERNEL_NAMES[uc.KERNEL_UPDATE] == "k_step_update"
    # no TS_KERNEL_* of the step library has that value
    step_header = open(os.path.join(ROOT, "include", "tiler_slider.h")).read()
    assert uc.KERNEL_UPDATE not in {int(v) for v in re.findall(r"#define TS_KERNEL_\w+ (\d+)", step_header)}
    P = C.c_void_p
    assert L.ts_step_update.argtypes == [C.POINTER(_cabi.Dims), C.POINTER(_cabi.State), P, C.c_uint32, C.POINTER(_cabi.StepOut), P, P]
    proto = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert ("int32_t ts_step_update(const ts_dims *dims, const ts_state *st, const uint8_t *actions, uint32_t mode, "
            "const ts_step_out *out, void *shown, void *stream);") in proto
    assert "int32_t ts_describe_step_update(const ts_dims *dims, uint32_t outputs, ts_launch_desc *desc);" in proto
    import tiler_slider_amd
    assert callable(tiler_slider_amd.build_update_library) and "build_update_library" in tiler_slider_amd.__all__


def test_update_supported_over_the_grid():
    """S 0 .. 10, T and Tt -1 .. 10: TS_OK exactly for S <= 8, 1 <= T <= 8, Tt <= 8 with one observation and at most the reward."""
    from tiler_slider_amd import _cabi, _update_cabi as uc
    L = uc.lib()
    for S in range(0, 11):
        for T in range(-1, 11):
            for Tt in (-1, 0, 1, 2, 8, 9, 10):
                for mc in (0, 1):
                    d = _dims(S, T, mc, Tt=Tt)
                    base = _cabi.lib().ts_check_dims(C.byref(d))
                    want = base if base != _cabi.OK else (_cabi.OK if S <= 8 and 1 <= T <= 8 and Tt <= 8 else _cabi.ERR_LIMIT)
                    assert L.ts_update_supported(C.byref(d), _cabi.OUT_OBS) == want, (S, T, Tt, mc)
                    if want in (_cabi.OK, _cabi.ERR_LIMIT):
                        assert uc.update_supported(d, _cabi.OUT_OBS_U8 | _cabi.OUT_REWARD) == (want == _cabi.OK)
    assert L.ts_update_supported(None, _cabi.OUT_OBS) == _cabi.ERR_NULL
    ok = _dims(4, 2, 1)
    for outputs, want in ((_cabi.OUT_OBS, _cabi.OK), (_cabi.OUT_OBS_U8, _cabi.OK), (_cabi.OUT_OBS | _cabi.OUT_FLAGS, _cabi.OK),
                          (_cabi.OUT_OBS | _cabi.OUT_REWARD, _cabi.OK), (_cabi.OUT_OBS_U8 | _cabi.OUT_REWARD | _cabi.OUT_FLAGS, _cabi.OK),
                          (0, _cabi.ERR_ARG), (_cabi.OUT_FLAGS, _cabi.ERR_ARG), (_cabi.OUT_REWARD, _cabi.ERR_ARG),
                          (_cabi.OUT_OBS | _cabi.OUT_OBS_U8, _cabi.ERR_ARG), (_cabi.OUT_OBS | _cabi.OUT_ONEHOT, _cabi.ERR_ARG),
                          (_cabi.OUT_OBS | _cabi.OUT_VALID, _cabi.ERR_ARG), (_cabi.OUT_OBS_U8 | _cabi.OUT_VALID4, _cabi.ERR_ARG),
                          (_cabi.OUT_OBS | 0x80, _cabi.ERR_ARG)):
        assert L.ts_update_supported(C.byref(ok), outputs) == want, outputs
    # the shape is looked at before the outputs
    assert L.ts_update_supported(C.byref(_dims(9, 2)), _cabi.OUT_OBS | _cabi.OUT_ONEHOT) == _cabi.ERR_LIMIT


def test_argument_validation_precedes_any_launch():
    """No GPU here: every one of these calls has to answer before it touches the HIP runtime."""
    from tiler_slider_amd import _cabi, _update_cabi as uc
    L = uc.lib()
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    st = _cabi.State(p, p, p, p, p, p, None)

    def out(**kw):
        fields = dict(flags=p, obs=p, reward=None, onehot=None, valid=None, obs_u8=None, valid4=None)
        fields.update(kw)
        return _cabi.StepOut(*(fields[f] for f, _ in _cabi.StepOut._fields_))

    def call(d, st_=st, act=p, mode=0, o=None, shown=p):
        o = out() if o is None else o
        return L.ts_step_update(C.byref(d) if d is not None else None, C.byref(st_) if st_ is not None else None, act, mode,
                                C.byref(o) if o is not False else None, shown, None)

    ok = _dims(4, 2, 1)
    assert call(None) == _cabi.ERR_NULL
    assert call(_dims(0, 2)) == _cabi.ERR_DIMS
    assert call(ok, o=False) == _cabi.ERR_NULL
    assert call(_dims(9, 2)) == _cabi.ERR_LIMIT                      # S = 9
    assert call(_dims(4, 0, Tt=2)) == _cabi.ERR_LIMIT                # T = 0
    assert call(_dims(4, 9)) == _cabi.ERR_LIMIT                      # T = 9
    assert call(_dims(4, 2, Tt=9)) == _cabi.ERR_LIMIT
    assert call(ok, o=out(onehot=p)) == _cabi.ERR_ARG                # one-hot planes
    assert call(ok, o=out(valid=p)) == _cabi.ERR_ARG and call(ok, o=out(valid4=p)) == _cabi.ERR_ARG
    assert call(ok, o=out(obs_u8=p)) == _cabi.ERR_ARG                # both observation pointers
    assert call(ok, o=out(obs=None)) == _cabi.ERR_ARG                # none
    for mode in (2, 3, 8, 0x80000000):
        assert call(ok, mode=mode) == _cabi.ERR_ARG                  # an unknown mode bit
    assert call(_dims(9, 2), mode=8) == _cabi.ERR_LIMIT              # the shape before the mode
    # an empty batch: TS_OK without a launch and without looking at a pointer, after every check above
    empty = _dims(4, 2, 1, n=0)
    assert call(empty, st_=None, act=None, shown=None) == _cabi.OK
    assert call(empty, mode=8) == _cabi.ERR_ARG and call(empty, o=out(onehot=p)) == _cabi.ERR_ARG
    # missing pointers
    assert call(ok, shown=None) == _cabi.ERR_NULL                    # NULL shown
    assert call(ok, act=None) == _cabi.ERR_NULL and call(ok, st_=None) == _cabi.ERR_NULL
    assert call(ok, o=out(flags=None)) == _cabi.ERR_NULL
    for field in ("pos", "blk", "step_count", "done", "tgt"):
        broken = _cabi.State(p, p, p, p, p, p, None)
        setattr(broken, field, None)
        assert call(ok, st_=broken) == _cabi.ERR_NULL, field
    no_init = _cabi.State(p, None, p, p, p, p, None)
    assert call(ok, st_=no_init, mode=_cabi.MODE_AUTORESET) == _cabi.ERR_NULL
    # misaligned float observation / reward
    assert call(ok, o=out(obs=p + 2)) == _cabi.ERR_ARG and call(ok, o=out(reward=p + 1)) == _cabi.ERR_ARG
    assert L.ts_update_last_hip_error() == 0
    assert L.ts_describe_step_update(C.byref(ok), _cabi.OUT_OBS, None) == _cabi.ERR_NULL
    assert L.ts_describe_step_update(None, _cabi.OUT_OBS, C.byref(_cabi.LaunchDesc())) == _cabi.ERR_NULL


def test_describe_step_update_names_exactly_the_compiled_kernels_and_fills_the_launch_record():
    """Every kernel of the code object is what some supported call launches and every launch names a kernel that exists; the
    record has every key bench.py reads; a Dims object marked `step_in_place` answers _cabi.describe_launch with it."""
    from tiler_slider_amd import _cabi, _update_cabi as uc
    compiled = _kernel_names(uc.LIB_PATH)
    assert len(compiled) == uc.MIN_KERNELS == 32
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
    assert sorted(named) == compiled
    assert uc.describe_step_update(_dims(4, 2, 1, 16 << 20))["out_of_cache"] == 1
    empty = uc.describe_step_update(_dims(4, 2, 1, 0))
    assert (empty["name"], empty["kernel"], empty["blocks"]) == ("", 0, 0)
    keys = {"name", "boards_per_wave", "cached_every", "emit_edges", "xcd_piece", "blocks_per_cu", "blocks", "out_of_cache"}
    d = _dims(4, 2, 1, 1 << 20)
    full = _cabi.describe_launch(d, _cabi.OP_STEP, _cabi.OUT_OBS)
    assert keys <= set(full) and not full["name"].startswith("k_step_update")
    d.step_in_place = True
    marked = _cabi.describe_launch(d, _cabi.OP_STEP, _cabi.OUT_OBS | _cabi.OUT_FLAGS)
    assert set(marked) == set(full) and marked == uc.describe_step_update(d, _cabi.OUT_OBS) and marked["name"] == "k_step_update<4, 2, false>"
    assert _cabi.describe_launch(d, _cabi.OP_RESET, _cabi.OUT_OBS) == _cabi.describe_launch(_dims(4, 2, 1, 1 << 20), _cabi.OP_RESET, _cabi.OUT_OBS)


def test_every_update_kernel_keeps_its_board_in_registers():
    """The code object's own metadata and instructions: no LDS, no private segment (scratch), no s_barrier, no ds_ and no
    scratch_ instruction in any of the 32 kernels."""
    from tiler_slider_amd import _update_cabi as uc
    kernels = _kernel_metadata(uc.LIB_PATH)
    assert len(kernels) == len([k for k in kernels if "k_step_update" in k["name"]]) == uc.MIN_KERNELS
    assert not any(k["group_segment_fixed_size"] or k["private_segment_fixed_size"] or k["uses_dynamic_stack"] for k in kernels), kernels
    counts = _instruction_counts(uc.LIB_PATH, (r"\b(s_barrier|ds_\w+|scratch_\w+)\b",))
    mine = {k: v[0] for k, v in counts.items() if "k_step_update" in k}
    assert len(mine) == uc.MIN_KERNELS and not any(mine.values()), mine


def test_update_case_table_has_one_entry_per_compiled_kernel():
    """tests/update_cases.py: its keys are exactly the kernels of the code object, and the dims of every entry make
    ts_describe_step_update name the entry's key - with the float32 and with the uint8 output set."""
    from tiler_slider_amd import _cabi, _update_cabi as uc
    assert sorted(cases.CASES) == _kernel_names(uc.LIB_PATH) and len(cases.CASES) == uc.MIN_KERNELS
    for name, (S, T, Tt, K) in cases.CASES.items():
        assert 1 <= T <= S * S and K >= 0, name
        for outputs, u8 in ((_cabi.OUT_OBS, False), (_cabi.OUT_OBS | _cabi.OUT_REWARD, False), (_cabi.OUT_OBS_U8, True),
                            (_cabi.OUT_OBS_U8 | _cabi.OUT_REWARD | _cabi.OUT_FLAGS, True)):
            for mc in (0, 1):
                d = uc.describe_step_update(_dims(S, T, mc, 331, Tt=Tt), outputs)
                assert (d["name"] == name) == (u8 == cases.is_u8(name)), (name, outputs, d["name"])
    # the two observation types of a shape share their levels
    assert len({cases.shape_key(n) for n in cases.CASES}) == 16
    assert all(cases.shape_key(n) == cases.shape_key(n.replace("false", "true")) for n in cases.CASES)


@pytest.mark.parametrize("name", sorted(n for n in cases.CASES if not cases.is_u8(n)))
def test_update_case_levels_are_honest(oracle, name):
    """What the GPU tests of a case can see, from the oracle alone, in both colour modes: 331 boards of the case's levels, 24
    steps of the unpatched action stream, max_steps 6, autoreset mode - tiles move, boards win where the counts allow it and
    never elsewhere, episodes time out and are reset.  The levels are well formed: cells inside the board, tiles apart, no tile
    and no target on an obstacle."""
    import numpy as np
    S, T, Tt, K = cases.CASES[name]
    N = 331
    for mc in (True, False):
        blk, init, tgt = cases.levels(oracle, name, N, mc)
        assert blk.shape == ((S * S + 31) // 32, N) and init.shape == (T, N) and tgt.shape == (Tt, N)
        assert init.dtype == tgt.dtype == np.uint8 and blk.dtype == np.uint32
        assert int(init.max()) < S * S and (Tt == 0 or int(tgt.max()) < S * S or Tt > S * S)
        wall = np.zeros((S * S, N), bool)
        for p in range(S * S):
            wall[p] = (blk[p >> 5] >> np.uint32(p & 31)) & 1
        assert (wall.sum(axis=0) == K).all()
        cols = np.arange(N)
        for t in range(T):
            assert not wall[init[t], cols].any(), (name, "a tile on an obstacle")
            for u in range(t):
                assert (init[t] != init[u]).all(), (name, "two tiles on one cell")
        for j in range(Tt):
            assert not wall[np.minimum(tgt[j], S * S - 1), cols].any(), (name, "a target on an obstacle")
        ref = oracle.OracleBatch(S, mc, 6, blk, init, tgt)
        ref.reset()
        flags = np.stack([ref.step(oracle.fill_actions(N, seed=cases.ACTION_SEED, step_index=k), mode=oracle.MODE_AUTORESET,
                                   obs=False)["flags"] for k in range(24)])
        moved, wins, resets, timeouts = cases.assert_floors(name, mc, flags)
        print(f"{name} {'multi' if mc else 'single'} colour: {moved:.2f} moved, {wins} wins, {resets} autoresets, {timeouts} timeouts")
