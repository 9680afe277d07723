"""The reach policy tables without a GPU: the rptable library's C-ABI (include/tiler_slider_rptable.h), its refusals in the header's
order, its launch plans, its code object, and the CPU yardstick's own properties (tests/rptable_reference.py) on the levels of
tests/reach_cases.py and tests/deep_cases.py - among them the input conditions that tests/test_gpu_rptable.py relies on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rptable_reference as xr
import rstarts_reference as rs
import rtable_reference as rt
from cabi_harness import _dims, _instruction_counts, _kernel_metadata, _kernel_names, _struct_fields
from conftest import ROOT
from tiler_slider_amd import _rptable_cabi as xc


def _header():
    return open(os.path.join(ROOT, "include", "tiler_slider_rptable.h")).read()


def test_abi_version_constants_and_what_is_reused():
    import tiler_slider_amd as pkg
    from tiler_slider_amd import _libraries, _policy_cabi, _rtable_cabi
    header = _header()
    assert xc.lib().ts_rptable_abi_version() == xc.ABI_VERSION == 1
    assert int(re.search(r"#define TS_RPTABLE_ABI_VERSION (\d+)", header).group(1)) == 1
    for name, value in (("TS_RPTABLE_NO_ACTION", xc.NO_ACTION), ("TS_RPTABLE_FORM_NONE", xc.FORM_NONE), ("TS_RPTABLE_FORM_LDS", xc.FORM_LDS),
                        ("TS_RPTABLE_FORM_GLOBAL", xc.FORM_GLOBAL)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value, name
    assert xc in _libraries.SINCE and _libraries.SINCE[-1] is xc and xc.MIN_KERNELS == 32
    assert pkg.build_rptable_library is xc.build_library and {"ReachPolicyTable", "build_rptable_library"} <= set(pkg.__all__)
    assert issubclass(pkg.ReachPolicyTable, pkg.ReachTable)
    # the network, the roots and the slot format are reused, not redefined
    assert xc.Mlp is _policy_cabi.Mlp and xc.ROOTS is _rtable_cabi.ROOTS
    assert "typedef struct ts_mlp" not in header and "#define TS_RTABLE_ROOT" not in header
    for name in ('#include "tiler_slider_policy.h"', '#include "tiler_slider_ptable.h"', '#include "tiler_slider_rtable.h"'):
        assert name in header
    for phrase in ("home(key) = (uint32)((key * 0x9e3779b97f4a7c15) >> 32) >> (32 - log2(slots))", "always below C", "LIVE",
                   "bit-equal", "written exactly once", "this one successor in place of four", "A FULL level's row is therefore all zero",
                   "The final pass re-reads the keys", "the same bits on every run and for every slot order", "REFUSALS, in this order and before any HIP call"):
        assert phrase in header, phrase
    src = open(xc.SRC).read()
    assert '#include "ts_mlp.h"' in src and "logits_of<S, MT>" in src and "static_preact<S>" in src and "stage_weights(a, C)" in src
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ts_rptable.hip" in design and "k_rptable_actions" in design and "k_rptable_walk" in design and "k_rptable_score" in design


def test_struct_layouts():
    header = _header()
    for struct, cls in (("ts_rptable_cfg", xc.RptableCfg), ("ts_rptable_out", xc.RptableOut), ("ts_rptable_desc", xc.RptableDesc)):
        assert _struct_fields(header, struct) == [f for f, _ in cls._fields_], struct
    assert (C.sizeof(xc.RptableCfg), C.sizeof(xc.RptableOut), C.sizeof(xc.RptableDesc)) == (8, 24, 6 * 4 + 8 + 64)
    assert [(f, getattr(xc.RptableDesc, f).offset) for f, _ in xc.RptableDesc._fields_] == [
        ("form", 0), ("threads_per_block", 4), ("lds_bytes", 8), ("lds_slots", 12), ("weights_in_lds", 16), ("reserved", 20), ("blocks", 24),
        ("name", 32)]
    assert [(f, getattr(xc.RptableOut, f).offset) for f, _ in xc.RptableOut._fields_] == [("table", 0), ("root_moves", 8), ("deepest", 16)]


def test_supported_over_the_grid_is_the_reach_tables_and_the_policys_together():
    from tiler_slider_amd import _cabi, _policy_cabi as pc, _rtable_cabi as rc
    L, LP, LR = xc.lib(), pc.lib(), rc.lib()
    ones = 0
    for S in range(0, 12):
        for T in range(-1, 12):
            for Tt in (0, 1, 8, 9, 300):
                for mc in (0, 1, 2):
                    for H in (0, 1, 7, 64, 65):
                        d = _dims(S, T, mc, 8, Tt)
                        got, a, b = L.ts_rptable_supported(C.byref(d), H), LR.ts_rtable_supported(C.byref(d)), LP.ts_policy_supported(C.byref(d), H)
                        assert (got == 1) == (a == 1 and b == 1), (S, T, Tt, mc, H)
                        assert got == (1 if a == 1 and b == 1 else b if b < 0 else 0), (S, T, Tt, mc, H)
                        ones += got == 1
    assert ones > 500
    assert L.ts_rptable_supported(None, 1) == _cabi.ERR_NULL
    assert xc.rptable_supported(_dims(5, 4)) and xc.rptable_supported(_dims(8, 8), 64) and not xc.rptable_supported(_dims(9, 1))
    assert not xc.rptable_supported(_dims(4, 9)) and not xc.rptable_supported(_dims(5, 4), 65) and not xc.rptable_supported(_dims(5, 4, 0, 8, 9))
    with pytest.raises(_cabi.TilerSliderLibraryError):
        xc.rptable_supported(_dims(0, 1))


BAD_SLOTS = (-2, 0, 1, 3, 48, (1 << 31) + 1, 1 << 32)
BAD_SHAPES = ((9, 1, None), (16, 2, None), (4, 9, None), (5, 4, 9))     # (S, T, Tt): beyond the reach tables or the network


def _memory():
    buf = (C.c_uint8 * (1 << 17))()
    base = (C.addressof(buf) + 255) & ~255
    return buf, (lambda k: base + k * 4096)


def _state(at, **kw):
    from tiler_slider_amd import _cabi
    a = dict(pos=at(0), init=at(1), tgt=at(2), blk=at(3), step_count=at(4), done=at(5))
    a.update(kw)
    return _cabi.State(a["pos"], a["init"], a["tgt"], a["blk"], a["step_count"], a["done"], None)


ref_ = lambda x: C.byref(x) if x is not None else None


def test_every_refusal_of_the_actions_has_its_own_status_in_the_headers_order():
    """No HIP call is made before a refusal: on a machine without a GPU one would have answered TS_ERR_HIP."""
    from tiler_slider_amd import _cabi
    L = xc.lib()
    NULL, ARG, LIMIT, DIMS, OK = _cabi.ERR_NULL, _cabi.ERR_ARG, _cabi.ERR_LIMIT, _cabi.ERR_DIMS, _cabi.OK
    keep, at = _memory()
    N, slots = 4, 32       # table 1,024 bytes, count 16, act 128, logits 2,048
    ok = _dims(5, 4, n=N)
    mlp = lambda H=7, **kw: xc.Mlp(**{**dict(w1=at(6), b1=at(7), w2=at(8), b2=at(9), hidden=H, reserved=0), **kw})

    def call(d=ok, st="st", m="mlp", table=at(10), slots=slots, count=at(11), act=at(12), logits=at(13)):
        st = _state(at) if st == "st" else st
        m = mlp() if m == "mlp" else m
        return L.ts_rptable_actions(ref_(d), ref_(st), ref_(m), table, slots, count, act, logits, None)

    describe = lambda d, H=7, slots=slots: L.ts_describe_rptable_actions(ref_(d), H, slots, C.byref(xc.RptableDesc()))
    # 1. dims: the shared check, before the network
    assert call(d=None) == NULL and describe(None) == NULL and L.ts_describe_rptable_actions(C.byref(ok), 7, slots, None) == NULL
    assert call(d=_dims(0, 2), m=None) == DIMS and call(d=_dims(4, 17), m=None) == DIMS and call(d=_dims(4, 2, 2), m=None) == DIMS
    assert call(d=_dims(33, 2), m=None) == LIMIT and describe(_dims(0, 2)) == DIMS and describe(_dims(33, 2)) == LIMIT
    # 2. mlp, before the arguments
    assert call(m=None, slots=3) == NULL and call(d=_dims(9, 1), m=None) == NULL
    # 3. slots, the shape, the width: TS_ERR_ARG, before the empty batch and before any pointer
    empty = _dims(5, 4, n=0)
    for s in BAD_SLOTS:
        assert call(slots=s, st=None) == ARG and call(d=empty, slots=s) == ARG and describe(ok, slots=s) == ARG, s
    for S, T, Tt in BAD_SHAPES:
        assert call(d=_dims(S, T, Tt=Tt), st=None) == ARG and call(d=_dims(S, T, n=0, Tt=Tt)) == ARG and describe(_dims(S, T, Tt=Tt)) == ARG, (S, T, Tt)
    for H in (0, -1, 65):
        assert call(m=mlp(H), st=None) == ARG and call(d=empty, m=mlp(H)) == ARG and describe(ok, H) == ARG, H
    # 4. the empty batch: TS_OK without a launch, no further pointer is looked at
    assert call(d=empty, st=None, table=None, count=None, act=None, logits=1) == OK and call(d=empty, slots=1 << 31) == OK
    assert describe(empty) == describe(ok) == OK
    # 5. missing pointers, before the alignment (logits is misaligned throughout)
    off = at(13) + 4
    assert call(st=None, logits=off) == NULL
    for kw in (dict(table=None), dict(count=None), dict(act=None)):
        assert call(logits=off, **kw) == NULL, kw
    for name in ("w1", "b1", "w2", "b2"):
        assert call(m=mlp(**{name: None}), logits=off) == NULL, name
    assert call(st=_state(at, blk=None), logits=off) == NULL and call(st=_state(at, tgt=None), logits=off) == NULL
    assert call(d=_dims(5, 4, n=N, Tt=0), st=_state(at, tgt=None, pos=None, init=None, step_count=None, done=None), logits=off) == ARG   # not read: not needed
    # 6. the alignment of logits
    for k in (1, 4, 8, 15):
        assert call(logits=at(13) + k) == ARG, k
    assert L.ts_rptable_last_hip_error() == 0


def test_every_refusal_of_the_walk_has_its_own_status_in_the_headers_order():
    from tiler_slider_amd import _cabi
    L = xc.lib()
    NULL, ARG, LIMIT, DIMS, OK = _cabi.ERR_NULL, _cabi.ERR_ARG, _cabi.ERR_LIMIT, _cabi.ERR_DIMS, _cabi.OK
    keep, at = _memory()
    N, slots = 4, 32       # table and out->table 1,024 bytes each, act 128
    ok, empty = _dims(5, 4, n=N), _dims(5, 4, n=0)
    cfg = lambda max_depth=252, root=0: xc.RptableCfg(max_depth, root)
    out = lambda **kw: xc.RptableOut(**{**dict(table=at(14), root_moves=at(15), deepest=at(16)), **kw})

    def call(d=ok, st="st", table=at(10), slots=slots, count=at(11), act=at(12), c="cfg", o="out"):
        st = _state(at) if st == "st" else st
        c = cfg() if c == "cfg" else c
        o = out() if o == "out" else o
        return L.ts_rptable_walk(ref_(d), ref_(st), table, slots, count, act, ref_(c), ref_(o), None)

    describe = lambda d, slots=slots: L.ts_describe_rptable_walk(ref_(d), slots, C.byref(xc.RptableDesc()))
    # 1. dims
    assert call(d=None) == NULL and describe(None) == NULL and L.ts_describe_rptable_walk(C.byref(ok), slots, None) == NULL
    assert call(d=_dims(0, 2), c=None) == DIMS and call(d=_dims(4, 17), o=None) == DIMS and call(d=_dims(33, 2), c=None) == LIMIT
    assert describe(_dims(0, 2)) == DIMS and describe(_dims(33, 2)) == LIMIT
    # 2. cfg / out, before the arguments
    assert call(c=None, slots=3) == NULL and call(o=None, slots=3) == NULL and call(d=_dims(9, 1), c=None) == NULL
    # 3. the arguments, before the empty batch and before any pointer
    for s in BAD_SLOTS:
        assert call(slots=s, st=None) == ARG and call(d=empty, slots=s) == ARG and describe(ok, s) == ARG, s
    for S, T, Tt in BAD_SHAPES:
        assert call(d=_dims(S, T, Tt=Tt), st=None) == ARG and call(d=_dims(S, T, n=0, Tt=Tt)) == ARG and describe(_dims(S, T, Tt=Tt)) == ARG, (S, T, Tt)
    for depth in (-1, 253, 2 ** 31 - 1):
        assert call(c=cfg(max_depth=depth), st=None) == ARG and call(d=empty, c=cfg(max_depth=depth)) == ARG, depth
    for root in (-1, 2):
        assert call(c=cfg(root=root), st=None) == ARG and call(d=empty, c=cfg(root=root)) == ARG, root
    # 4. the empty batch
    assert call(d=empty, st=None, table=None, count=None, act=None, o=xc.RptableOut()) == OK and call(d=empty, slots=1 << 31, c=cfg(0, 1)) == OK
    assert describe(empty) == describe(ok) == OK
    # 5. missing pointers, before the overlap (out->table lies on the table throughout)
    on = dict(table=at(10))
    assert call(st=None, o=out(**on)) == NULL and call(table=None, o=out(table=at(12))) == NULL
    assert call(count=None, o=out(**on)) == NULL and call(act=None, o=out(**on)) == NULL and call(o=out(table=None)) == NULL
    assert call(st=_state(at, blk=None), o=out(**on)) == NULL and call(st=_state(at, tgt=None), o=out(**on)) == NULL
    assert call(st=_state(at, init=None), o=out(**on)) == NULL and call(st=_state(at, pos=None), c=cfg(root=1), o=out(**on)) == NULL
    # the root is read only where root_moves is asked for, and only the one cfg->root names
    assert call(st=_state(at, init=None), o=out(root_moves=None, **on)) == ARG and call(st=_state(at, pos=None), o=out(**on)) == ARG
    assert call(st=_state(at, init=None), c=cfg(root=1), o=out(**on)) == ARG
    # 6. out->table over the table or over act, byte-exactly
    for t in (at(10), at(10) + 1023, at(10) - 1023, at(12) + 127, at(12) - 1023):
        assert call(o=out(table=t)) == ARG, t - at(10)
    assert L.ts_rptable_last_hip_error() == 0


def test_every_refusal_of_the_score_has_its_own_status_in_the_headers_order():
    from tiler_slider_amd import _cabi
    L = xc.lib()
    NULL, ARG, LIMIT, DIMS, OK = _cabi.ERR_NULL, _cabi.ERR_ARG, _cabi.ERR_LIMIT, _cabi.ERR_DIMS, _cabi.OK
    keep, at = _memory()
    N, slots = 4, 32
    ok, empty = _dims(5, 4, n=N), _dims(5, 4, n=0)

    def call(d=ok, st="st", ptable=at(14), act=at(12), table=at(10), slots=slots, count=at(11), score=at(17)):
        st = _state(at) if st == "st" else st
        return L.ts_rptable_score(ref_(d), ref_(st), ptable, act, table, slots, count, score, None)

    describe = lambda d, slots=slots: L.ts_describe_rptable_score(ref_(d), slots, C.byref(xc.RptableDesc()))
    # 1. dims
    assert call(d=None) == NULL and describe(None) == NULL and L.ts_describe_rptable_score(C.byref(ok), slots, None) == NULL
    assert call(d=_dims(0, 2), slots=3) == DIMS and call(d=_dims(33, 2), slots=3) == LIMIT and describe(_dims(0, 2)) == DIMS
    # 2. slots and the shape, before the empty batch and before any pointer
    for s in BAD_SLOTS:
        assert call(slots=s, st=None) == ARG and call(d=empty, slots=s) == ARG and describe(ok, s) == ARG, s
    for S, T, Tt in BAD_SHAPES:
        assert call(d=_dims(S, T, Tt=Tt), st=None) == ARG and call(d=_dims(S, T, n=0, Tt=Tt)) == ARG and describe(_dims(S, T, Tt=Tt)) == ARG, (S, T, Tt)
    # 3. the empty batch
    assert call(d=empty, st=None, ptable=None, act=None, table=None, count=None, score=2) == OK and describe(empty) == describe(ok) == OK
    # 4. missing pointers, before the alignment (score is misaligned throughout)
    off = at(17) + 2
    assert call(st=None, score=off) == NULL and call(score=None) == NULL
    for kw in (dict(ptable=None), dict(act=None), dict(table=None), dict(count=None)):
        assert call(score=off, **kw) == NULL, kw
    assert call(st=_state(at, blk=None), score=off) == NULL and call(st=_state(at, tgt=None), score=off) == NULL
    assert call(st=_state(at, pos=None, init=None, step_count=None, done=None), score=off) == ARG   # not read: not needed
    # 5. the alignment of score
    for k in (1, 2, 3):
        assert call(score=at(17) + k) == ARG, k
    assert L.ts_rptable_last_hip_error() == 0


def test_describe_on_both_sides_of_the_walks_lds_threshold_and_of_weights_in_lds():
    lds = xc.describe_rptable_walk(_dims(5, 4), 2)["lds_slots"]
    assert lds >= 8192 and lds & (lds - 1) == 0        # a table of capacity 4,096 is walked in LDS
    for n, blocks in ((0, 0), (1, 1), (1023, 1023), (1024, 1024), (1085, 1024), (16384, 1024)):
        for S, T in ((1, 1), (5, 4), (8, 8)):
            for slots, form, name in ((2, xc.FORM_LDS, "false"), (lds, xc.FORM_LDS, "false"), (2 * lds, xc.FORM_GLOBAL, "true"),
                                      (1 << 31, xc.FORM_GLOBAL, "true")):
                d = xc.describe_rptable_walk(_dims(S, T, 1, n), slots)
                assert (d["form"], d["name"], d["blocks"]) == ((form, f"k_rptable_walk<{S}, {name}>", blocks) if n else (xc.FORM_NONE, "", 0)), (n, slots, d)
                assert (d["threads_per_block"], d["lds_slots"], d["lds_bytes"]) == (256, lds, 16 + 5 * lds if form == xc.FORM_LDS else 16), d
                assert d["lds_bytes"] <= 64 * 1024 and d["weights_in_lds"] == 0
                s = xc.describe_rptable_score(_dims(S, T, 1, n), slots)
                assert s == dict(form=xc.FORM_LDS if n else 0, threads_per_block=256, lds_bytes=128, lds_slots=0, weights_in_lds=0, blocks=blocks,
                                 name=f"k_rptable_score<{S}>" if n else ""), s
    # the actions: the policy library's forward plan with the list beside it
    seen = set()
    for S, T, mc in ((5, 4, 1), (8, 8, 1), (8, 8, 0), (4, 0, 0), (1, 1, 1)):
        for H in (1, 7, 16, 64):
            d = xc.describe_rptable_actions(_dims(S, T, mc, 128), H, 2048)
            planes = (T if mc else 1) * S * S
            want_staged = [t for t in (256, 128, 64) if T and 16 * H + 16 + ((4 * H * planes + 15) & ~15) + 4 * H * t + 5136 <= 65536]
            assert d["weights_in_lds"] == bool(want_staged) and d["threads_per_block"] == (want_staged[0] if want_staged else d["threads_per_block"]), (S, T, H, d)
            assert d["threads_per_block"] in (64, 128, 256) and d["lds_bytes"] <= 64 * 1024 and d["lds_bytes"] % 16 == 0
            assert (d["form"], d["blocks"], d["name"], d["lds_slots"]) == (xc.FORM_LDS, 128, f"k_rptable_actions<{S}>", 0)
            seen.add((S, T, mc, H, d["weights_in_lds"]))
    # the two shapes of the bit-equality test lie on either side
    assert (5, 4, 1, 64, 1) in seen and (8, 8, 1, 64, 0) in seen and (8, 8, 1, 7, 1) in seen
    assert xc.describe_rptable_actions(_dims(5, 4, 1, 0), 7, 2048)["name"] == ""


def _names():
    return ([f"k_rptable_actions<{S}>" for S in range(1, 9)] + [f"k_rptable_score<{S}>" for S in range(1, 9)]
            + [f"k_rptable_walk<{S}, {g}>" for S in range(1, 9) for g in ("false", "true")])


def test_the_code_object_holds_exactly_the_kernels_describe_names():
    lds = xc.describe_rptable_walk(_dims(5, 4), 2)["lds_slots"]
    named = set()
    for S in range(1, 9):
        for T in (0, 1, 4, 8):
            d = _dims(S, min(T, S * S), 1)
            named |= {xc.describe_rptable_actions(d, 7, 64)["name"], xc.describe_rptable_score(d, 64)["name"],
                      xc.describe_rptable_walk(d, lds)["name"], xc.describe_rptable_walk(d, 2 * lds)["name"]}
    assert sorted(named) == sorted(_names()) == _kernel_names(xc.LIB_PATH)


def test_no_kernel_has_scratch_and_the_walk_and_the_score_no_float():
    meta = _kernel_metadata(xc.LIB_PATH)
    assert len(meta) == 32 == xc.MIN_KERNELS
    lds = xc.describe_rptable_walk(_dims(5, 4), 2)["lds_slots"]
    for k in meta:
        assert k["private_segment_fixed_size"] == 0 and not k["uses_dynamic_stack"] and k["agpr_count"] == 0, k
        assert k["vgpr_count"] <= 64, k   # eight waves a SIMD
        want = 0 if "actions" in k["name"] else 128 if "score" in k["name"] else 16 if "Lb1E" in k["name"] else 16 + 5 * lds
        assert k["group_segment_fixed_size"] == want, k     # the actions: no static LDS in front of the dynamic region
    counts = _instruction_counts(xc.LIB_PATH, (r"\bv_\w+_f(16|32|64)\b", r"\bscratch_", r"\bs_barrier\b", r"\bglobal_atomic_(?!load|store)", r"\bbuffer_atomic"))
    assert len(counts) == 32
    for k, found in counts.items():
        assert found[1] == 0 and found[2] > 0 and found[3] == found[4] == 0, (k, found)
        assert (found[0] > 0) == ("actions" in k), (k, found)


# ---------------------------------------------------------------------------------------------------------- the yardstick's own
@pytest.mark.parametrize("S", (3, 4, 5, 6, 7, 8))
def test_the_input_conditions_hold_on_the_yardstick_alone(oracle, S):
    """The mixed tabular policy on the levels of reach_cases at capacity 1,024, summed over both colour modes: no GPU test passes
    on degenerate input."""
    solved = worse = none = deep = by_empty = by_cut = 0
    for mc in (False, True):
        ref = rs.case(oracle, S, mc)[3]
        act = xr.mixed_policy(ref, 7 + S)
        e, deepest, exhausted = xr.walk(ref, act)
        fin = (e >= 1) & (e <= 252)
        o = ref.entry
        assert ((e[fin] >= o[fin]) & (o[fin] >= 1) & (o[fin] <= 252)).all()     # no policy beats the optimum
        solved += int(fin.sum())
        worse += int((fin & (e > o)).sum())
        none += int((e == xr.NONE).sum())
        assert not (e == xr.DEEP).any() and exhausted.all()
        e3, deepest3, exhausted3 = xr.walk(ref, act, 3)
        deep += int((e3 == xr.DEEP).sum())
        held = ref.count > 0
        by_empty += int((exhausted3 & held).sum())
        by_cut += int((~exhausted3 & held).sum())
        assert np.array_equal(e3[e3 <= 3], e[e <= 3]) and (deepest3 <= 3).all() and np.array_equal(np.minimum(deepest, 3), deepest3)
        # the score of the walk: the columns are what they say
        sc = xr.score(ref, e, act)
        assert sc[:, 0].sum() == ref.idx.size and sc[:, 2].sum() == fin.sum() and sc[:, 7].sum() == 0 and (sc[:, 3] <= sc[:, 2]).all()
        assert sc[:, 5].sum() == (e[fin].astype(np.int64) - o[fin]).sum() and (sc[ref.count < 0] == 0).all()
    figures = dict(solved=solved, worse=worse, none=none, deep_at_3=deep, levels_by_rule=(by_empty, by_cut))
    print(S, figures)
    assert solved >= 100 and worse >= 10 and none >= 1000, (S, figures)
    assert deep >= 500 and by_empty >= 5 and by_cut >= 5, (S, figures)


@pytest.mark.parametrize("S", (3, 5, 8))
def test_walking_the_experts_moves_reproduces_the_table(oracle, S):
    for mc in (False, True):
        ref = rs.case(oracle, S, mc)[3]
        act = xr.expert(ref)
        e, deepest, _ = xr.walk(ref, act)
        solvable = (ref.entry >= 1) & (ref.entry <= 252)
        assert np.array_equal(act != 255, solvable) and np.array_equal(e[solvable], ref.entry[solvable]) and (e[~solvable] == xr.NONE).all()
        assert np.array_equal(deepest, ref.deepest)
        sc = xr.score(ref, e, act)
        assert np.array_equal(sc[:, 1], sc[:, 2]) and np.array_equal(sc[:, 1], sc[:, 3]) and np.array_equal(sc[:, 1], sc[:, 4]) and not sc[:, 5].any()
        blk, init, tgt = rs.case(oracle, S, mc)[:3]
        assert np.array_equal(xr.root_moves(oracle, ref, blk, tgt, init, e), ref.root_moves)


def test_the_host_filled_rows_hold_the_references_states_whatever_the_order(oracle):
    ref = rs.case(oracle, 5, True)[3]
    slots = 2048
    rows, slot = xr.rows_of(ref, slots)
    other, slot2 = xr.rows_of(ref, slots, "reversed")
    assert not np.array_equal(rows, other) and not np.array_equal(slot, slot2)
    full = ref.count < 0
    assert full.any() and np.array_equal(np.sort(rows[~full], axis=1), np.sort(other[~full], axis=1))
    assert np.array_equal(rows[ref.level, slot], xr.table_words(ref, ref.entry)) and np.array_equal(other[ref.level, slot2], rows[ref.level, slot])
    assert ((rows[~full] != 0).sum(axis=1) == ref.count[~full]).all() and ((rows[full] >> np.uint64(63)) != 0).any()
    laid = xr.scatter(ref, slot, ref.entry, slots, 0)
    assert laid.shape == (len(ref.count), slots) and np.array_equal(laid[~full], ((rows[~full] >> np.uint64(48)) & np.uint64(0xff)).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------- the deep levels
DEEP = {  # level -> |R|, the root's distance, finite chains, off the tree, the longest chain
    "MULTI": (359, 106, 203, 156, 133), "SMALL": (126, 37, 126, 0, 79), "LARGE": (994, 61, 994, 0, 340)}


@pytest.mark.parametrize("which", sorted(DEEP))
def test_the_deep_levels_from_their_roots(oracle, which):
    import deep_cases as deep
    import table_reference as tref
    lv = deep.levels()[getattr(deep, which)]
    ref, act, chain = xr.deep_reference(oracle, lv)
    finite = (chain >= 1) & (chain < tref.UNREACHABLE)
    figures = (int(ref.count[0]), int(ref.root_moves[0]), int(finite.sum()), int((chain == tref.UNREACHABLE).sum()), int(chain[finite].max()))
    print(which, figures)
    assert figures == DEEP[which], (which, figures)
    assert not (chain == 0).any() and not (chain == tref.INVALID_PLACEMENT).any()     # won placements are not stored
    # the reach walk's finite entries are walk_exact at that key, cut or not
    for depth in (252, figures[4], figures[4] - 1):
        e, deepest, exhausted = xr.walk(ref, act, min(depth, 252))
        cut = min(depth, 252)
        assert np.array_equal(e[finite & (chain <= cut)], chain[finite & (chain <= cut)].astype(np.uint8))
        rest = ~(finite & (chain <= cut))
        assert (e[rest] == (xr.NONE if exhausted[0] else xr.DEEP)).all() and deepest[0] == min(figures[4], cut)
    if which == "LARGE":
        e, _, exhausted = xr.walk(ref, act)
        assert (finite & (chain > 252)).sum() == 389 and (e == xr.DEEP).sum() == 389 and not exhausted[0] and np.array_equal(e == xr.DEEP, finite & (chain > 252))
    # the optimum over R is the dense table's at those keys
    dist = deep.exact(oracle, lv)[ref.idx]
    assert np.array_equal(ref.entry, np.where(dist == tref.UNREACHABLE, 255, dist).astype(np.uint8))
