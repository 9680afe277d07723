"""The reach-table curricula without a GPU: the rstarts library's C-ABI (include/tiler_slider_rstarts.h), its refusals in the
header's order, its launch plans, its code object, and the CPU yardstick's own properties (tests/rstarts_reference.py) on the
levels of tests/reach_cases.py - among them the non-degeneracy floors that tests/test_gpu_rstarts.py relies on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rstarts_reference as rs
from cabi_harness import _dims, _instruction_counts, _kernel_metadata, _kernel_names, _struct_fields
from conftest import ROOT
from tiler_slider_amd import _rstarts_cabi as xs

MAX_CAPACITY = 1 << 30


def _header():
    return open(os.path.join(ROOT, "include", "tiler_slider_rstarts.h")).read()


def test_abi_version_constants_and_the_reused_structs():
    import tiler_slider_amd as pkg
    from tiler_slider_amd import _libraries, _starts_cabi as sc
    header = _header()
    assert xs.lib().ts_rstarts_abi_version() == xs.ABI_VERSION == 1
    assert int(re.search(r"#define TS_RSTARTS_ABI_VERSION (\d+)", header).group(1)) == 1
    for name, value in (("TS_RSTARTS_FIRST", xs.FIRST), ("TS_RSTARTS_FORM_NONE", xs.FORM_NONE), ("TS_RSTARTS_FORM_LDS", xs.FORM_LDS),
                        ("TS_RSTARTS_FORM_GLOBAL", xs.FORM_GLOBAL)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value, name
    assert xs in _libraries.SINCE and xs.MIN_KERNELS == 10
    assert pkg.build_rstarts_library is xs.build_library and {"ReachIndex", "build_rstarts_library"} <= set(pkg.__all__)
    assert callable(pkg.VecTilerSliderEnv.build_reach_index) and pkg.ReachIndex.__name__ == "ReachIndex"
    # ts_starts_cfg and ts_starts_out are reused, not copied: the header declares neither and the binding holds the parents' classes
    assert xs.StartsCfg is sc.StartsCfg and xs.StartsOut is sc.StartsOut and (xs.ALL, xs.DONE) == (sc.ALL, sc.DONE)
    assert "typedef struct ts_starts_cfg" not in header and "typedef struct ts_starts_out" not in header
    for name in ('#include "tiler_slider_rtable.h"', '#include "tiler_slider_starts.h"'):
        assert name in header
    # the definition is in the header in full
    for phrase in ("ascending unsigned order", "first[0] = first[1] = 0", "first[253] is the number of states with a finite distance",
                   "EMPTY index", "SET of (key, entry) pairs", "arbitrary bytes", "((R >> 32) * count[n]) >> 32", "sorted[r][a + j]",
                   "distance 0 never matches", "always below C", "REFUSALS, in this order and before any HIP call"):
        assert phrase in header, phrase
    src = open(xs.SRC).read()
    assert '#include "ts_core.h"' in src and '#include "ts_launch.h"' in src
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ts_rstarts.hip" in design and "k_rstarts_place" in design and "k_rstarts_index" in design


def test_struct_layout():
    assert _struct_fields(_header(), "ts_rstarts_desc") == [f for f, _ in xs.RstartsDesc._fields_]
    assert C.sizeof(xs.RstartsDesc) == 4 * 4 + 2 * 8 + 64
    assert [(f, getattr(xs.RstartsDesc, f).offset) for f, _ in xs.RstartsDesc._fields_] == [
        ("form", 0), ("threads_per_block", 4), ("lds_bytes", 8), ("lds_states", 12), ("blocks", 16), ("bytes", 24), ("name", 32)]
    assert (C.sizeof(xs.StartsCfg), C.sizeof(xs.StartsOut)) == (56, 24)
    assert [(f, getattr(xs.StartsCfg, f).offset) for f, _ in xs.StartsCfg._fields_] == [
        ("lo", 0), ("hi", 4), ("band", 8), ("where", 16), ("write_pos", 20), ("write_init", 24), ("reserved", 28), ("seed", 32),
        ("step_index", 40), ("board_offset", 48)]
    assert [(f, getattr(xs.StartsOut, f).offset) for f, _ in xs.StartsOut._fields_] == [("count", 0), ("dist", 8), ("deepest", 16)]


def test_supported_over_the_grid_is_the_reach_tables():
    from tiler_slider_amd import _cabi, _rtable_cabi as rc
    L, LR = xs.lib(), rc.lib()
    for S in range(0, 12):
        for T in range(-1, 12):
            for Tt in (0, 1, 8, 9, 300):
                for mc in (0, 1, 2):
                    d = _dims(S, T, mc, 8, Tt)
                    assert L.ts_rstarts_supported(C.byref(d)) == LR.ts_rtable_supported(C.byref(d)), (S, T, Tt, mc)
    assert L.ts_rstarts_supported(None) == _cabi.ERR_NULL
    assert xs.rstarts_supported(_dims(5, 4)) and xs.rstarts_supported(_dims(8, 8)) and not xs.rstarts_supported(_dims(9, 1))
    assert not xs.rstarts_supported(_dims(4, 9))
    with pytest.raises(_cabi.TilerSliderLibraryError):
        xs.rstarts_supported(_dims(0, 1))


def test_every_refusal_of_the_index_has_its_own_status_in_the_headers_order():
    """No HIP call is made before a refusal: on a machine without a GPU one would have answered TS_ERR_HIP."""
    from tiler_slider_amd import _cabi
    L = xs.lib()
    NULL, ARG, OK = _cabi.ERR_NULL, _cabi.ERR_ARG, _cabi.OK
    buf = (C.c_uint8 * (1 << 16))()
    base = (C.addressof(buf) + 255) & ~255
    # 4 levels x 32 slots: table 1,024 bytes, count 16, sorted (W = 16) 512, first 4,096
    table, count, out, first = base, base + 1024, base + 2048, base + 4096
    index = lambda t=table, slots=32, c=count, n=4, W=16, s=out, f=first: L.ts_rstarts_index(t, slots, c, n, W, s, f, None)
    desc = lambda n=4, slots=32, W=16: L.ts_describe_rstarts_index(n, slots, W, C.byref(xs.RstartsDesc()))
    # 1. the arguments, before the empty batch and before any pointer
    for kw in [dict(n=-1)] + [dict(slots=s) for s in (-2, 0, 1, 3, 48, (1 << 31) + 1, 1 << 32)] + [dict(W=w) for w in (0, -1, MAX_CAPACITY + 1)]:
        assert index(t=None, c=None, s=None, f=None, **kw) == ARG, kw
        assert desc(**kw) == ARG, kw
        if "n" not in kw:
            assert index(t=None, n=0, **kw) == ARG, kw
    # 2. the empty batch
    assert index(t=None, c=None, s=None, f=None, n=0) == OK and index(n=0, slots=1 << 31, W=MAX_CAPACITY) == OK
    # 3. pointers, before the overlap (sorted lies on the table throughout)
    for kw in (dict(t=None), dict(c=None), dict(s=None), dict(f=None)):
        assert index(**{**dict(s=table), **kw}) == NULL, kw
    # 4. an output over an input or over the other output, byte-exactly
    for s in (table, table + 1023, table - 511, count + 15, count - 511, first + 4095, first - 511):
        assert index(s=s) == ARG, s - base
    for f in (table + 1023, table - 4095, count + 15, count - 4095):
        assert index(f=f) == ARG, f - base
    assert L.ts_rstarts_last_hip_error() == 0
    # describe: desc NULL first, then refusal 1
    assert L.ts_describe_rstarts_index(4, 32, 16, None) == NULL and L.ts_describe_rstarts_index(-1, 32, 16, None) == NULL
    assert desc() == desc(n=0) == OK


def test_every_refusal_of_the_placement_has_its_own_status_in_the_headers_order():
    """ts_starts_place's refusals with `table` replaced by `sorted` and `first`, and W checked."""
    from tiler_slider_amd import _cabi
    L = xs.lib()
    N = 8
    buf = (C.c_uint8 * (1 << 16))()
    base = (C.addressof(buf) + 255) & ~255
    at = lambda k: base + k * 1024
    NULL, ARG, LIMIT, DIMS, OK = _cabi.ERR_NULL, _cabi.ERR_ARG, _cabi.ERR_LIMIT, _cabi.ERR_DIMS, _cabi.OK
    ok = _dims(5, 4, n=N)

    def state(**kw):
        a = dict(pos=at(0), init=at(1), tgt=at(2), blk=at(3), step_count=at(4), done=at(5))
        a.update(kw)
        return _cabi.State(a["pos"], a["init"], a["tgt"], a["blk"], a["step_count"], a["done"], None)

    def cfg(**kw):
        a = dict(lo=1, hi=252, band=None, where=xs.ALL, write_pos=1, write_init=1, reserved=0, seed=7, step_index=0, board_offset=0)
        a.update(kw)
        return xs.StartsCfg(**a)

    def out(**kw):
        a = dict(count=at(6), dist=at(7), deepest=at(8))
        a.update(kw)
        return xs.StartsOut(**a)

    ref_ = lambda x: C.byref(x) if x is not None else None

    def call(d=ok, st=None, srt=at(10), first=at(20), W=16, n_rows=N, rows=None, c=None, o=None, keep_none=()):
        st = state() if st is None and "st" not in keep_none else st
        c = cfg() if c is None and "c" not in keep_none else c
        o = out() if o is None and "o" not in keep_none else o
        return L.ts_rstarts_place(ref_(d), ref_(st), srt, first, W, n_rows, rows, ref_(c), ref_(o), None)

    describe = lambda d: L.ts_describe_rstarts_place(ref_(d), C.byref(xs.RstartsDesc()))
    bad = cfg(lo=-1)          # an argument that would be refused later: what comes first is answered first
    # 1. dims: the shared check
    assert call(d=None) == NULL and describe(None) == NULL
    assert call(d=_dims(0, 2), c=bad) == DIMS and call(d=_dims(4, 17), c=bad) == DIMS and call(d=_dims(4, 2, 2), c=bad) == DIMS
    assert call(d=_dims(33, 2), keep_none=("c", "o")) == LIMIT and call(d=_dims(0, 2), keep_none=("c", "o")) == DIMS
    assert describe(_dims(0, 2)) == DIMS and describe(_dims(33, 2)) == LIMIT
    # 2. cfg / out, before the shape
    for S, T in ((5, 4), (9, 1)):
        assert call(d=_dims(S, T), keep_none=("c",)) == NULL and call(d=_dims(S, T), keep_none=("o",)) == NULL
    # 3. the shape, before the arguments
    for S, T in ((9, 1), (16, 2), (4, 9)):
        assert call(d=_dims(S, T), c=bad) == LIMIT and describe(_dims(S, T)) == LIMIT
    assert describe(ok) == OK and L.ts_describe_rstarts_place(C.byref(ok), None) == NULL
    # 4. the arguments, before the empty batch and before any pointer
    empty = _dims(5, 4, n=0)
    nothing = xs.StartsOut()
    for kw in (dict(lo=-1), dict(lo=253), dict(hi=-1), dict(hi=253), dict(hi=2 ** 31 - 1), dict(where=2), dict(where=-1), dict(write_pos=2),
               dict(write_pos=-1), dict(write_init=2), dict(write_init=-1)):
        assert call(c=cfg(**kw)) == ARG, kw
        assert call(d=empty, c=cfg(**kw), o=nothing, srt=None, first=None, keep_none=("st",)) == ARG, kw
    assert call(n_rows=-1) == ARG and call(d=empty, n_rows=-1) == ARG
    for W in (0, -1, MAX_CAPACITY + 1):
        assert call(W=W) == ARG and call(d=empty, W=W, srt=None) == ARG
    assert call(c=cfg(lo=5, hi=3), srt=None) == NULL       # an empty band is no error: on to the pointers
    assert call(c=cfg(lo=0, hi=0), first=None) == NULL and call(c=cfg(lo=252, hi=252), srt=None) == NULL
    # 5. the empty batch: TS_OK without a launch, no pointer is looked at
    assert call(d=empty, o=nothing, srt=None, first=None, keep_none=("st",)) == OK and call(d=empty, W=MAX_CAPACITY) == OK
    # 6. missing pointers, before the overlap (band lies on count throughout)
    on_count = dict(band=at(6))
    assert call(c=cfg(**on_count), keep_none=("st",)) == NULL
    assert call(c=cfg(**on_count), srt=None) == NULL and call(c=cfg(**on_count), first=None) == NULL
    for name in ("pos", "step_count", "done"):
        assert call(st=state(**{name: None}), c=cfg(**on_count)) == NULL, name
        if name != "done":
            assert call(st=state(**{name: None}), c=cfg(write_pos=0, **on_count)) == ARG, name     # not written: not needed
    assert call(st=state(init=None), c=cfg(**on_count)) == NULL and call(st=state(init=None), c=cfg(write_init=0, **on_count)) == ARG
    assert call(st=state(done=None), c=cfg(write_pos=0, where=xs.DONE, **on_count)) == NULL
    assert call(st=state(done=None), c=cfg(write_pos=0, **on_count)) == ARG
    assert call(st=state(tgt=None, blk=None), c=cfg(**on_count)) == ARG                            # the level is not read
    assert call(c=cfg(write_pos=0, write_init=0, band=at(30)), o=nothing) == NULL                  # no output and no write at all
    zero_tiles = _dims(5, 0, n=N)
    assert call(d=zero_tiles, st=state(pos=None, init=None), c=cfg(**on_count)) == ARG             # no tile: no cell is written
    # 7. band over anything that is written, byte-exactly: 2 N bytes of band, T N of cells, 4 N of int32, N of bytes
    for where_, size in ((at(0), 4 * N), (at(1), 4 * N), (at(4), 4 * N), (at(5), N), (at(6), 4 * N), (at(7), N), (at(8), N)):
        assert call(c=cfg(band=where_)) == ARG and call(c=cfg(band=where_ + size - 1)) == ARG and call(c=cfg(band=where_ - 2 * N + 1)) == ARG
    # then n_rows = 0: TS_OK without a launch; a band over what is only read is no overlap
    assert call(c=cfg(band=at(0), write_pos=0), n_rows=0) == OK and call(c=cfg(band=at(1), write_init=0), n_rows=0) == OK
    assert call(c=cfg(band=at(4), write_pos=0), n_rows=0) == OK and call(c=cfg(band=at(5), write_pos=0, where=xs.DONE), n_rows=0) == OK
    assert call(c=cfg(band=at(6)), o=out(count=None), n_rows=0) == OK and call(n_rows=0, srt=None, first=None) == OK
    assert L.ts_rstarts_last_hip_error() == 0


def test_describe_on_both_sides_of_the_lds_threshold():
    lds = xs.describe_rstarts_index(1, 2, 1)["lds_states"]
    assert lds >= 1024 and lds & (lds - 1) == 0
    for n, blocks in ((0, 0), (1, 1), (1023, 1023), (1024, 1024), (1085, 1024), (16384, 1024)):
        for W, slots, form, name in ((1, 2, xs.FORM_LDS, "k_rstarts_index<false>"), (lds - 1, 2 * lds, xs.FORM_LDS, "k_rstarts_index<false>"),
                                     (lds, 2 * lds, xs.FORM_LDS, "k_rstarts_index<false>"), (lds + 1, 4 * lds, xs.FORM_GLOBAL, "k_rstarts_index<true>"),
                                     (65536, 1 << 17, xs.FORM_GLOBAL, "k_rstarts_index<true>"), (MAX_CAPACITY, 1 << 31, xs.FORM_GLOBAL, "k_rstarts_index<true>")):
            d = xs.describe_rstarts_index(n, slots, W)
            assert (d["form"], d["name"], d["blocks"]) == ((form, name, blocks) if n else (xs.FORM_NONE, "", 0)), (n, W, d)
            assert (d["threads_per_block"], d["lds_states"], d["lds_bytes"], d["bytes"]) == (256, lds, 8 * lds + 16, 8 * W + 1024), (n, W, d)
            assert d["lds_bytes"] <= 64 * 1024      # what a block gets without asking
    for S, T in ((1, 1), (5, 4), (8, 8), (4, 0)):
        for n, blocks in ((0, 0), (1, 1), (256, 1), (257, 2), (rs.N_OCC, 1024)):
            d = xs.describe_rstarts_place(_dims(S, T, 0, n))
            assert d == dict(form=0, threads_per_block=256, lds_bytes=0, lds_states=0, blocks=blocks, bytes=0, name=f"k_rstarts_place<{S}>" if n else ""), d


def test_the_code_object_holds_exactly_the_kernels_describe_names():
    lds = xs.describe_rstarts_index(1, 2, 1)["lds_states"]
    named = {xs.describe_rstarts_place(_dims(S, min(T, S * S), mc))["name"] for S in range(1, 9) for T in (0, 1, 4, 8) for mc in (0, 1)}
    named |= {xs.describe_rstarts_index(3, 4 * lds, W)["name"] for W in (1, lds, lds + 1)}
    want = ["k_rstarts_index<false>", "k_rstarts_index<true>"] + [f"k_rstarts_place<{S}>" for S in range(1, 9)]
    assert sorted(named) == want == _kernel_names(xs.LIB_PATH)
    assert sorted(rs.occupancy_cases()) == want[2:]


def test_the_kernels_use_no_scratch_no_float_and_the_placement_no_lds():
    meta = _kernel_metadata(xs.LIB_PATH)
    assert len(meta) == 10 == xs.MIN_KERNELS
    lds_bytes = xs.describe_rstarts_index(1, 2, 1)["lds_bytes"]
    for k in meta:
        assert k["private_segment_fixed_size"] == 0 and not k["uses_dynamic_stack"] and k["agpr_count"] == 0, k
        assert k["group_segment_fixed_size"] == (lds_bytes if "index" in k["name"] else 0), k
        assert k["vgpr_count"] <= 64, k   # eight waves a SIMD
    counts = _instruction_counts(xs.LIB_PATH, (r"\bv_\w+_f(16|32|64)\b", r"\bscratch_", r"\bs_barrier\b", r"\bglobal_atomic", r"\bds_"))
    assert len(counts) == 10
    for k, found in counts.items():
        if "place" in k:
            assert found == [0, 0, 0, 0, 0], (k, found)
        else:
            assert found[:2] == [0, 0] and found[2] > 0 and found[3] == 0 and found[4] > 0, (k, found)


# ---------------------------------------------------------------------------------------------------------- the yardstick's own
def test_the_host_filled_row_holds_its_pairs_whatever_the_order():
    keys, entries = rs.synthetic_pairs(300, seed=3)
    row = rs.fill_row(keys, entries, 1024)
    other = rs.fill_row(keys, entries, 1024, order=np.random.default_rng(0).permutation(300))
    assert not np.array_equal(row, other) and np.array_equal(np.sort(row), np.sort(other))
    held = row[row != 0]
    assert held.size == 300 and (held >> np.uint64(63)).all() and set((held & rs.KEY_MASK).tolist()) == set(keys.tolist())
    srt, first = rs.index_of_pairs(keys, entries, 512)
    assert np.array_equal(srt[:300], np.sort(held)) and not srt[300:].any()
    assert first[0] == first[1] == 0 and first[253] == ((entries >= 1) & (entries <= 252)).sum() and (np.diff(first) >= 0).all()
    assert first[255] == (entries < 255).sum()
    for d in (1, 2, 7, 40, 41, 254):
        assert first[d] == (entries < d).sum()
    assert not rs.index_of_pairs(keys, entries, 299)[0].any() and not rs.index_of_pairs(keys, entries, 299)[1].any()


BANDS = ((1, 252), (2, 4), (1, 1))
FLOOR = 10


@pytest.mark.parametrize("S", (3, 4, 5, 6, 7, 8))
def test_the_yardstick_places_on_states_of_the_level_and_the_floors_hold(oracle, S):
    """On the levels of reach_cases at capacity 1,024, both colour modes: a drawn placement is a state of the level, inside the
    band, with the distance rtable_reference.lookup reads there; over one level and 64 * count boards every matching state is
    drawn; at least FLOOR of the 128 levels hold a placement in each of BANDS, and band [100, 252] is empty everywhere."""
    import reach_cases as cases
    import rtable_reference as rt
    T = cases.SHAPES[S][0]
    C_ = S * S
    for mc in (False, True):
        blk, init, tgt, ref, srt, first = rs.case(oracle, S, mc)
        L = cases.DISTINCT
        assert srt.shape == (L, cases.CAPACITY) and not srt[ref.count < 0].any() and not first[ref.count < 0].any()
        for n in range(L):   # a row is exactly the level's set
            if ref.count[n] >= 0:
                kept = srt[n, :ref.count[n]]
                assert np.array_equal(np.sort(kept & rs.KEY_MASK), ref.keys(n).astype(np.uint64)) and (np.diff(kept.astype(np.uint64)) > 0).all()
        figures = {}
        for lo, hi in BANDS + ((100, 252),):
            got = rs.place(srt, first, C_, T, L, lo, hi, seed=S)
            p = got["placed"]
            figures[(lo, hi)] = int(p.sum())
            assert np.array_equal(p, got["count"] > 0) and ((got["dist"][p] >= lo) & (got["dist"][p] <= hi)).all()
            pos = init.copy()
            pos[:, p] = got["cells"][:, p]
            assert np.array_equal(rt.keys_of(S, pos)[p], got["key"][p])
            moves = rt.lookup(oracle, ref, blk, tgt, pos)[0]
            assert np.array_equal(moves[p], got["dist"][p].astype(np.int16)), (S, mc, lo, hi)
            for n in np.flatnonzero(p)[:8]:
                e = ref.entries(n).astype(np.int64)
                assert got["count"][n] == ((e >= lo) & (e <= hi)).sum() and got["deepest"][n] == e[e <= 252].max()
        print(S, mc, figures, "deepest", int(ref.deepest.max()))
        for band in BANDS:
            assert figures[band] >= FLOOR, (S, mc, figures)
        assert figures[(100, 252)] == 0 and ref.deepest.max() < 100
        # every matching state of one level is drawn
        counts = rs.place(srt, first, C_, T, L, 2, 4)["count"]
        n = int(np.flatnonzero(counts > 1)[np.argmin(counts[counts > 1])])
        c = int(counts[n])
        many = rs.place(srt, first, C_, T, 64 * c, 2, 4, rows=np.full(64 * c, n), seed=11)
        e = ref.entries(n)
        assert many["placed"].all() and set(many["key"].tolist()) == set(ref.keys(n)[(e >= 2) & (e <= 4)].tolist())


def test_the_two_forms_of_the_yardsticks_placement_agree(oracle):
    """place_many() - the definition on whole arrays, for the occupancy cases - against the loop per board: rows with repeats and
    two indices out of range, a band per board with bytes above 252, random flags, another stream position."""
    import reach_cases as cases
    S, mc = 5, True
    T = cases.SHAPES[S][0]
    _, _, _, ref, srt, first = rs.case(oracle, S, mc)
    rng = np.random.default_rng(4)
    N = 700
    rows = rng.integers(0, cases.DISTINCT, N)
    rows[[5, 600]] = (-1, cases.DISTINCT)
    band = rng.integers(0, 12, (2, N)).astype(np.uint8)
    band[1, ::5] = rng.integers(253, 256, len(band[1, ::5]))
    band[0, 3::7] = rng.integers(253, 256, len(band[0, 3::7]))
    sel = rng.integers(0, 2, N).astype(bool)
    for kw in (dict(lo=1, hi=252), dict(lo=2, hi=4, selected=sel), dict(band=band), dict(band=band, selected=sel, seed=9, step_index=3, board_offset=10 ** 12)):
        a, b = rs.place(srt, first, S * S, T, N, rows=rows, **kw), rs.place_many(srt, first, S * S, T, N, rows=rows, **kw)
        assert a["placed"].sum() >= 20 and (~a["placed"]).sum() >= 20
        for name in a:
            assert np.array_equal(a[name], b[name]), (kw.keys(), name)
    a, b = rs.place(srt, first, S * S, T, cases.DISTINCT), rs.place_many(srt, first, S * S, T, cases.DISTINCT)
    assert all(np.array_equal(a[name], b[name]) for name in a)
