"""The curriculum starts without a GPU: the starts library's C-ABI (include/tiler_slider_starts.h), its refusals in the header's
order, its launch plan, its code object, and the CPU yardstick's own properties (tests/starts_reference.py) on real tables."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import starts_reference as sref
from cabi_harness import _dims, _kernel_metadata, _kernel_names, _struct_fields
from conftest import ROOT
from tiler_slider_amd import _starts_cabi as sc


def test_starts_library_exports_what_its_header_declares():
    header = open(os.path.join(ROOT, "include", "tiler_slider_starts.h")).read()
    assert '#include "tiler_slider_table.h"' in header
    for name, value in (("TS_STARTS_ALL", sc.ALL), ("TS_STARTS_DONE", sc.DONE),
                        ("TS_STARTS_PIECE_BYTES", sc.PIECE_BYTES), ("TS_STARTS_FORM_NONE", sc.FORM_NONE), ("TS_STARTS_FORM_WAVE", sc.FORM_WAVE)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value, name
    # the definition is in the header in full
    for phrase in ("match(i)", "min(hi_n, 252)", "((R >> 32) * count[n]) >> 32", "the j-th matching index in ascending order",
                   "(idx / C^t) % C", "0xd1b54a32d192ed03", "0x9e3779b97f4a7c15", "REFUSALS, in this order and before any HIP call"):
        assert phrase in header, phrase
    for struct, cls in (("ts_starts_cfg", sc.StartsCfg), ("ts_starts_out", sc.StartsOut), ("ts_starts_desc", sc.StartsDesc)):
        fields = _struct_fields(header, struct)
        assert fields == [f for f, _ in cls._fields_], struct
    assert (C.sizeof(sc.StartsCfg), C.sizeof(sc.StartsOut), C.sizeof(sc.StartsDesc)) == (56, 24, 104)
    assert [(f, getattr(sc.StartsCfg, f).offset) for f, _ in sc.StartsCfg._fields_] == [
        ("lo", 0), ("hi", 4), ("band", 8), ("where", 16), ("write_pos", 20), ("write_init", 24), ("reserved", 28), ("seed", 32),
        ("step_index", 40), ("board_offset", 48)]
    assert [(f, getattr(sc.StartsOut, f).offset) for f, _ in sc.StartsOut._fields_] == [("count", 0), ("dist", 8), ("deepest", 16)]
    assert [(f, getattr(sc.StartsDesc, f).offset) for f, _ in sc.StartsDesc._fields_] == [
        ("form", 0), ("lanes_per_board", 4), ("boards_per_block", 8), ("threads_per_block", 12), ("bytes_per_lane", 16), ("passes", 20),
        ("states", 24), ("blocks", 32), ("name", 40)]
    assert dict(sc.StartsCfg._fields_)["seed"] is C.c_uint64
    import tiler_slider_amd as pkg
    assert callable(pkg.build_starts_library) and {"StartInfo", "build_starts_library"} <= set(pkg.__all__)
    assert callable(pkg.VecTilerSliderEnv.place_at_distance)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ts_starts.hip" in design and "k_starts_place" in design


def test_supported_shapes_are_the_tables():
    from tiler_slider_amd import _cabi, _table_cabi
    L, LT = sc.lib(), _table_cabi.lib()
    for S in range(0, 11):
        for T in range(-1, 8):
            for mc in (0, 1, 2):
                d = _dims(S, T, mc)
                states = LT.ts_table_states(C.byref(d))
                assert L.ts_starts_supported(C.byref(d)) == (states if states < 0 else int(states > 0)), (S, T, mc)
    assert L.ts_starts_supported(None) == _cabi.ERR_NULL
    assert sc.starts_supported(_dims(4, 2)) and not sc.starts_supported(_dims(5, 4))
    with pytest.raises(_cabi.TilerSliderLibraryError):
        sc.starts_supported(_dims(0, 1))


def test_every_refusal_has_its_own_status_in_the_headers_order():
    """No HIP call is made before a refusal: on a machine without a GPU one would have answered TS_ERR_HIP."""
    from tiler_slider_amd import _cabi
    L = sc.lib()
    N = 8
    buf = (C.c_uint8 * (1 << 16))()
    base = (C.addressof(buf) + 255) & ~255
    at = lambda k: base + k * 1024         # regions apart: the largest, 8 boards x 256 states, takes two
    NULL, ARG, LIMIT, DIMS, OK = _cabi.ERR_NULL, _cabi.ERR_ARG, _cabi.ERR_LIMIT, _cabi.ERR_DIMS, _cabi.OK
    ok = _dims(4, 2, n=N)

    def state(**kw):
        a = dict(pos=at(0), init=at(1), tgt=at(2), blk=at(3), step_count=at(4), done=at(5))
        a.update(kw)
        return _cabi.State(a["pos"], a["init"], a["tgt"], a["blk"], a["step_count"], a["done"], None)

    def cfg(**kw):
        a = dict(lo=1, hi=252, band=None, where=sc.ALL, write_pos=1, write_init=1, reserved=0, seed=7, step_index=0, board_offset=0)
        a.update(kw)
        return sc.StartsCfg(**a)

    def out(**kw):
        a = dict(count=at(6), dist=at(7), deepest=at(8))
        a.update(kw)
        return sc.StartsOut(**a)

    ref_ = lambda x: C.byref(x) if x is not None else None
    table = at(10)

    def call(d=ok, st=None, tab=table, n_rows=N, rows=None, c=None, o=None, keep_none=()):
        st = state() if st is None and "st" not in keep_none else st
        c = cfg() if c is None and "c" not in keep_none else c
        o = out() if o is None and "o" not in keep_none else o
        return L.ts_starts_place(ref_(d), ref_(st), tab, n_rows, rows, ref_(c), ref_(o), None)

    bad = cfg(lo=-1)          # an argument that would be refused later: what comes first is answered first
    # 1. dims: the shared check
    assert call(d=None) == NULL
    assert call(d=_dims(0, 2), c=bad) == DIMS and call(d=_dims(4, 17), c=bad) == DIMS and call(d=_dims(4, 2, 2), c=bad) == DIMS
    assert call(d=_dims(33, 2), keep_none=("c", "o")) == LIMIT and call(d=_dims(0, 2), keep_none=("c", "o")) == DIMS
    # 2. cfg / out, before the shape
    for S, T in ((4, 2), (5, 4)):
        assert call(d=_dims(S, T), keep_none=("c",)) == NULL and call(d=_dims(S, T), keep_none=("o",)) == NULL
    # 3. the shape, before the arguments
    for S, T in ((5, 4), (8, 3), (9, 1), (16, 2)):
        assert call(d=_dims(S, T), c=bad) == LIMIT
        assert L.ts_describe_starts_place(C.byref(_dims(S, T)), C.byref(sc.StartsDesc())) == LIMIT
    # 4. the arguments, before the empty batch and before any pointer
    empty = _dims(4, 2, n=0)
    nothing = sc.StartsOut()
    for kw in (dict(lo=-1), dict(lo=253), dict(hi=-1), dict(hi=253), dict(hi=2 ** 31 - 1), dict(where=2), dict(where=-1), dict(write_pos=2),
               dict(write_pos=-1), dict(write_init=2), dict(write_init=-1)):
        assert call(c=cfg(**kw)) == ARG, kw
        assert call(d=empty, c=cfg(**kw), o=nothing, tab=None, keep_none=("st",)) == ARG, kw
    assert call(n_rows=-1) == ARG and call(d=empty, n_rows=-1) == ARG
    assert call(c=cfg(lo=5, hi=3), tab=None) == NULL       # an empty band is no error: on to the pointers
    assert call(c=cfg(lo=0, hi=0), tab=None) == NULL and call(c=cfg(lo=252, hi=252), tab=None) == NULL
    # 5. the empty batch: TS_OK without a launch, no pointer is looked at
    assert call(d=empty, o=nothing, tab=None, keep_none=("st",)) == OK and call(d=empty) == OK
    # 6. missing pointers, before the overlap (band lies on count throughout)
    on_count = dict(band=at(6))
    assert call(c=cfg(**on_count), keep_none=("st",)) == NULL
    assert call(c=cfg(**on_count), tab=None) == NULL
    for name in ("pos", "step_count", "done"):
        assert call(st=state(**{name: None}), c=cfg(**on_count)) == NULL, name
        if name != "done":
            assert call(st=state(**{name: None}), c=cfg(write_pos=0, **on_count)) == ARG, name     # not written: not needed
    assert call(st=state(init=None), c=cfg(**on_count)) == NULL and call(st=state(init=None), c=cfg(write_init=0, **on_count)) == ARG
    assert call(st=state(done=None), c=cfg(write_pos=0, where=sc.DONE, **on_count)) == NULL
    assert call(st=state(done=None), c=cfg(write_pos=0, **on_count)) == ARG
    assert call(st=state(tgt=None, blk=None), c=cfg(**on_count)) == ARG                            # the level is not read
    assert call(c=cfg(write_pos=0, write_init=0, band=at(20)), o=nothing) == NULL                  # no output and no write at all
    zero_tiles = _dims(4, 0, n=N)
    assert call(d=zero_tiles, st=state(pos=None, init=None), c=cfg(**on_count)) == ARG             # no tile: no cell is written
    # 7. band over anything that is written, byte-exactly: 2 N bytes of band, T N of cells, 4 N of int32, N of bytes
    for where_, size in ((at(0), 2 * N), (at(1), 2 * N), (at(4), 4 * N), (at(5), N), (at(6), 4 * N), (at(7), N), (at(8), N)):
        assert call(c=cfg(band=where_)) == ARG and call(c=cfg(band=where_ + size - 1)) == ARG and call(c=cfg(band=where_ - 2 * N + 1)) == ARG
    assert call(c=cfg(band=at(0), write_pos=0), n_rows=0) == OK and call(c=cfg(band=at(1), write_init=0), n_rows=0) == OK   # read only
    assert call(c=cfg(band=at(4), write_pos=0), n_rows=0) == OK and call(c=cfg(band=at(5), write_pos=0, where=sc.DONE), n_rows=0) == OK
    assert call(c=cfg(band=at(6)), o=out(count=None), n_rows=0) == OK
    # then n_rows = 0: TS_OK without a launch, with or without a table
    assert call(n_rows=0) == OK and call(n_rows=0, tab=None) == OK and call(n_rows=0, c=cfg(band=at(20))) == OK
    assert L.ts_starts_last_hip_error() == 0
    assert L.ts_describe_starts_place(None, C.byref(sc.StartsDesc())) == NULL and L.ts_describe_starts_place(C.byref(ok), None) == NULL
    assert L.ts_describe_starts_place(C.byref(_dims(0, 2)), C.byref(sc.StartsDesc())) == DIMS


def test_describe_plans_lanes_and_passes_and_names_exactly_the_compiled_kernels():
    compiled = _kernel_names(sc.LIB_PATH)
    assert len(compiled) == sc.MIN_KERNELS == 8 and compiled == sorted(f"k_starts_place<{S}>" for S in range(1, 9))
    # states -> (S, T), lanes per board, passes
    want = {1: ((1, 1), 1, 1), 81: ((3, 2), 8, 1), 256: ((4, 2), 16, 1), 625: ((5, 2), 64, 1), 4096: ((4, 3), 64, 4), 59049: ((3, 5), 64, 58)}
    for states, ((S, T), lanes, passes) in want.items():
        for n in (1, 7, 4096, 1 << 20):
            d = sc.describe_starts_place(_dims(S, T, 0, n))
            assert d["states"] == states == (S * S) ** T
            assert (d["form"], d["lanes_per_board"], d["passes"], d["name"]) == (sc.FORM_WAVE, lanes, passes, f"k_starts_place<{S}>"), (states, d)
            assert d["name"] in compiled
            assert (d["threads_per_block"], d["bytes_per_lane"], d["boards_per_block"]) == (64, 16, 64 // lanes)
            assert d["blocks"] == -(-n // d["boards_per_block"])
    # every supported shape: a lane per 16-byte piece, up to the wave
    from tiler_slider_amd import _table_cabi
    for S in range(1, 9):
        for T in range(0, 6):
            states = _table_cabi.lib().ts_table_states(C.byref(_dims(S, T))) if T <= S * S else -1
            if states <= 0:
                continue
            d = sc.describe_starts_place(_dims(S, T, 1, 1000))
            pieces = -(-states // 16)
            assert d["lanes_per_board"] == min(64, 1 << (pieces - 1).bit_length()) and d["passes"] == -(-pieces // d["lanes_per_board"])
            assert d["passes"] == 1 or d["lanes_per_board"] == 64
    nothing = sc.describe_starts_place(_dims(4, 2, 0, 0))
    assert (nothing["form"], nothing["blocks"], nothing["name"], nothing["states"], nothing["passes"]) == (sc.FORM_NONE, 0, "", 256, 0)


def test_occupancy_cases_name_exactly_the_compiled_starts_kernels():
    """tests/test_gpu_starts.py runs one case per kernel at 4,096 one-wave blocks and more: its case table
    (tests/starts_reference.py) is the code object's list, no kernel without a case and no case without a kernel; the library
    names that kernel for the case's dims and plans the grid the GPU test relies on, with a ragged last block where a block holds
    several boards."""
    assert sorted(sref.OCCUPANCY_CASES) == _kernel_names(sc.LIB_PATH)
    assert len(sref.OCCUPANCY_CASES) == sc.MIN_KERNELS == 8
    for name, (S, T) in sref.OCCUPANCY_CASES.items():
        assert name == f"k_starts_place<{S}>" and (S * S) ** T <= 65536
        per_block = sc.describe_starts_place(_dims(S, T, 0, 1))["boards_per_block"]
        n = sref.occupancy_boards(per_block)
        d = sc.describe_starts_place(_dims(S, T, 0, n))
        assert (d["name"], d["form"], d["threads_per_block"], d["boards_per_block"]) == (name, sc.FORM_WAVE, 64, per_block), d
        assert d["blocks"] >= sref.OCC_BLOCKS and (per_block == 1 or n % per_block != 0), d
    assert {sc.describe_starts_place(_dims(S, T, 0, 9))["boards_per_block"] for S, T in sref.OCCUPANCY_CASES.values()} >= {1, 4, 8, 64}


def test_the_starts_kernels_use_no_scratch_no_lds_and_no_agprs():
    kernels = _kernel_metadata(sc.LIB_PATH)
    assert len(kernels) == len([k for k in kernels if "k_starts_place" in k["name"]]) == sc.MIN_KERNELS
    assert not any(k["group_segment_fixed_size"] or k["private_segment_fixed_size"] or k["agpr_count"] or k["uses_dynamic_stack"] for k in kernels), kernels
    assert max(k["vgpr_count"] for k in kernels) <= 64, kernels      # eight waves per SIMD


def test_the_byte_arithmetic_of_the_kernel_on_the_host(tmp_path):
    """csrc/ts_bytes.h - the comparisons four bytes at a time, the gathers, the packed maximum, the j-th set bit - compiled for the
    host with the toolchain's clang++ and run against byte loops over every byte value (tests/native/starts_bytes_check.cpp),
    under AddressSanitizer and UBSan: a stand-alone program, no GPU."""
    from tiler_slider_amd import _cabi
    src = os.path.join(ROOT, "tests", "native", "starts_bytes_check.cpp")
    exe = str(tmp_path / "starts_bytes_check")
    subprocess.run([f"{_cabi._LLVM_BIN}/clang++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", src, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), (out.returncode, out.stdout, out.stderr)


# ---------------------------------------------------------------------------------------------------------------- the yardstick
@pytest.fixture(scope="module")
def real_tables(oracle):
    """(S, T, mc, blk, init, tgt, table) of the issue's three sets: 300 seeded levels each."""
    import table_reference as tref
    sets = []
    for S, T, K, mc in ((4, 2, 2, False), (4, 2, 2, True), (3, 2, 1, False)):
        blk, init, tgt = oracle.generate(S, T, T, K, 300, seed=0x5EED)
        sets.append((S, T, mc, blk, init, tgt, tref.table(oracle, S, mc, blk, tgt, T)))
    return sets


@pytest.mark.parametrize("lo,hi", ((1, 252), (2, 4), (0, 0), (5, 3)))
def test_yardstick_places_on_valid_placements_inside_the_band(oracle, real_tables, lo, hi):
    import table_reference as tref
    for S, T, mc, blk, init, tgt, tab in real_tables:
        n = tab.shape[0]
        r = sref.place(tab, S * S, T, n, lo, hi, seed=0xC0FFEE, step_index=3)
        finite = np.where(tab <= tref.MAX_DEPTH, tab.astype(np.int64), -1)
        np.testing.assert_array_equal(r["count"], ((finite >= lo) & (finite <= hi)).sum(axis=1))
        np.testing.assert_array_equal(r["deepest"], np.where(finite.max(axis=1) >= 0, finite.max(axis=1), 255))
        np.testing.assert_array_equal(r["placed"], r["count"] > 0)
        p = r["placed"]
        assert (r["dist"][~p] == 255).all() and (r["idx"][~p] == -1).all()
        if lo > hi:
            assert not p.any()
            continue
        assert ((r["dist"][p] >= lo) & (r["dist"][p] <= hi)).all()
        np.testing.assert_array_equal(tref.index_of(S, r["cells"][:, p]), r["idx"][p])
        np.testing.assert_array_equal(tab[np.flatnonzero(p), r["idx"][p]], r["dist"][p])
        assert tref.is_placement(S, blk[:, p], r["cells"][:, p]).all()
        # the lookup's yardstick reads the same distance where the board now stands
        moves, _, _ = tref.lookup(oracle, S, blk[:, p], r["cells"][:, p], tab[p])
        np.testing.assert_array_equal(moves, r["dist"][p].astype(np.int16))
        if (lo, hi) in ((1, 252), (2, 4)):
            assert 0.1 <= p.mean() <= 0.9, p.mean()      # the figures of the GPU test: neither case is empty


def test_yardstick_draws_every_matching_index_of_a_row():
    """One row, 64 * count boards: a uniform draw misses a given index with probability (1 - 1 / count) ** (64 count) < e ** -64."""
    rng = np.random.default_rng(3)
    for states, count in ((256, 1), (256, 7), (81, 30), (625, 100)):
        row = np.full(states, 255, np.uint8)
        where = rng.choice(states, count, replace=False)
        row[where] = rng.integers(2, 5, count)
        n = 64 * count
        r = sref.place(row[None, :], 1, 0, n, 2, 4, rows=np.zeros(n, np.int64), seed=11)
        assert (r["count"] == count).all() and r["placed"].all()
        assert sorted(set(r["idx"].tolist())) == sorted(where.tolist())
        # the draw is the action stream's: its top two bits are ts_fill_actions' action
        again = sref.place(row[None, :], 1, 0, n, 2, 4, rows=np.zeros(n, np.int64), seed=11, step_index=1)
        assert (again["idx"] != r["idx"]).any() or count == 1


def test_yardstick_band_per_board_rows_and_selection():
    rng = np.random.default_rng(4)
    tab = rng.integers(0, 256, (5, 81)).astype(np.uint8)
    n = 40
    rows = rng.integers(-1, 7, n)
    band = rng.integers(0, 256, (2, n)).astype(np.uint8)
    sel = rng.integers(0, 2, n).astype(bool)
    r = sref.place(tab, 9, 2, n, band=band, rows=rows, selected=sel, seed=5)
    for b in range(n):
        inside = 0 <= rows[b] < 5
        e = tab[rows[b]] if inside else np.zeros(0, np.uint8)
        m = [i for i, v in enumerate(e) if band[0, b] <= v <= min(band[1, b], 252)]
        assert r["count"][b] == len(m) and r["deepest"][b] == max([v for v in e if v <= 252], default=255)
        assert r["placed"][b] == (inside and sel[b] and len(m) > 0)
        if r["placed"][b]:
            assert r["idx"][b] in m and r["cells"][:, b].tolist() == [r["idx"][b] % 9, r["idx"][b] // 9]
    pos, init = rng.integers(0, 9, (2, n)).astype(np.uint8), rng.integers(0, 9, (2, n)).astype(np.uint8)
    sc_, done = rng.integers(0, 9, n).astype(np.int32), rng.integers(0, 2, n).astype(np.uint8)
    p2, i2, s2, d2 = sref.apply(r, pos, init, sc_, done, True, False)
    k = ~r["placed"]
    assert (i2 == init).all() and (p2[:, k] == pos[:, k]).all() and (s2[k] == sc_[k]).all() and (d2[k] == done[k]).all()
    assert (p2[:, ~k] == r["cells"][:, ~k]).all() and not s2[~k].any() and not d2[~k].any()
