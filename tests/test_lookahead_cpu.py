"""The lookahead without a GPU: the library's C-ABI (include/tiler_slider_lookahead.h), its launch plan, its code object, and the
CPU yardstick (tests/lookahead_reference.py): its bound against float32 evaluations of the whole backup in three orders, an
independent restatement of the search in plain Python, and the input conditions tests/test_gpu_lookahead.py relies on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cabi_harness import _declared, _dims, _exported, _instruction_counts, _kernel_metadata, _kernel_names, _scan_last_vgpr, _struct_fields
from conftest import ROOT
from tiler_slider_amd import _lookahead_cabi as lc

LDS_LIMIT = 65536
MAX_STEPS = 65535
ZERO, VALUE, QMAX = 0, 1, 2


def test_lookahead_library_exports_what_its_header_declares():
    from tiler_slider_amd import _ac_cabi, _cabi, _libraries, _policy_cabi, _train_cabi
    L = lc.lib()
    assert _exported(lc.LIB_PATH) == _declared("tiler_slider_lookahead.h") == sorted(lc.EXPORTS) and len(lc.EXPORTS) == 5
    assert L.ts_lookahead_abi_version() == lc.ABI_VERSION == 1
    assert lc in _libraries.SINCE and _libraries.name(lc) == "lookahead"
    header = open(os.path.join(ROOT, "include", "tiler_slider_lookahead.h")).read()
    assert '#include "tiler_slider_ac.h"' in header
    for name, value in (("MAX_DEPTH", lc.MAX_DEPTH), ("NO_ACTION", lc.NO_ACTION), ("LEAF_ZERO", lc.LEAVES["zero"]),
                        ("LEAF_VALUE", lc.LEAVES["value"]), ("LEAF_QMAX", lc.LEAVES["qmax"]), ("ABI_VERSION", lc.ABI_VERSION)):
        assert int(re.search(rf"#define TS_LOOKAHEAD_{name} (\d+)", header).group(1)) == value, name
    assert (lc.MAX_DEPTH, lc.NO_ACTION, lc.LEAVES) == (4, 255, {"zero": 0, "value": 1, "qmax": 2})
    prose = re.sub(r"[\s*]+", " ", header)
    for said in ("An invalid move is a child like any other", "no transposition table", "TIMEOUT is not modelled", "NOT BUILT here",
                 "functions of the q the kernel stores, bit for bit", "win_in is integer and exact", "There are no atomics"):
        assert said in prose, said
    # the structs the header includes are not redefined, and the binding uses the other bindings' classes
    for struct in ("ts_mlp", "ts_value_head", "ts_train_in"):
        assert not re.search(rf"typedef struct {struct} ", header), struct
    assert lc.Mlp is _policy_cabi.Mlp and lc.TrainIn is _train_cabi.TrainIn and lc.ValueHead is _ac_cabi.ValueHead
    assert _struct_fields(header, "ts_lookahead_cfg") == [f for f, _ in lc.LookaheadCfg._fields_] == ["depth", "leaf", "gamma", "w_step", "w_win", "w_invalid", "reserved"]
    assert _struct_fields(header, "ts_lookahead_out") == [f for f, _ in lc.LookaheadOut._fields_] == ["q", "value", "best", "win_in"]
    assert _struct_fields(header, "ts_lookahead_desc") == [f for f, _ in lc.LookaheadDesc._fields_]
    assert (C.sizeof(lc.LookaheadCfg), C.sizeof(lc.LookaheadOut), C.sizeof(lc.LookaheadDesc)) == (32, 32, 24 + 24 + 64)
    assert [lc.LookaheadCfg.depth.offset, lc.LookaheadCfg.leaf.offset, lc.LookaheadCfg.gamma.offset, lc.LookaheadCfg.w_invalid.offset] == [0, 4, 8, 20]
    assert lc.LookaheadDesc.blocks.offset == 24 and lc.LookaheadDesc.name.offset == 48
    P = C.c_void_p
    assert L.ts_lookahead.argtypes == [C.POINTER(_cabi.Dims), C.POINTER(_cabi.State), C.POINTER(lc.Mlp), C.POINTER(lc.ValueHead),
                                       C.POINTER(lc.TrainIn), C.POINTER(lc.LookaheadCfg), C.POINTER(lc.LookaheadOut), P]
    proto = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert ("int32_t ts_lookahead(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_value_head *head, "
            "const ts_train_in *in, const ts_lookahead_cfg *cfg, const ts_lookahead_out *out, void *stream);") in proto
    assert ("int32_t ts_describe_lookahead(const ts_dims *dims, int32_t hidden, int32_t steps, int32_t depth, int32_t leaf, "
            "ts_lookahead_desc *desc);") in proto
    import tiler_slider_amd
    assert tiler_slider_amd.Lookahead._fields == ("q", "value", "best", "win_in") and callable(tiler_slider_amd.build_lookahead_library)
    assert callable(tiler_slider_amd.VecTilerSliderEnv.lookahead) and callable(tiler_slider_amd.VecTilerSliderEnv.td_targets)
    assert {"Lookahead", "build_lookahead_library"} <= set(tiler_slider_amd.__all__)
    import __graft_entry__ as entry
    assert callable(entry._smoke_lookahead)


def test_lookahead_supported_is_policy_supported_for_the_network_leaves():
    """S 0 .. 10, T -1 .. 10, both colour modes (and an invalid one), H in {0, 1, 64, 65}: the grid of tests/test_policy_cpu.py.
    With LEAF_ZERO the width is ignored: the answer is the policy library's at width 1."""
    from tiler_slider_amd import _cabi, _policy_cabi as pc
    L, LP = lc.lib(), pc.lib()
    seen = set()
    for S in range(0, 11):
        for T in range(-1, 11):
            for mc in (0, 1, 2):
                d = _dims(S, T, mc)
                for H in (0, 1, 64, 65):
                    want = LP.ts_policy_supported(C.byref(d), H)
                    for leaf in (VALUE, QMAX):
                        assert L.ts_lookahead_supported(C.byref(d), H, leaf) == want, (S, T, mc, H, leaf)
                    zero = L.ts_lookahead_supported(C.byref(d), H, ZERO)
                    assert zero == LP.ts_policy_supported(C.byref(d), 1), (S, T, mc, H)
                    seen.update((want, zero))
                    if want < 0:
                        assert L.ts_lookahead_supported(C.byref(d), H, 7) == want      # the dims first
                        continue
                    assert L.ts_lookahead_supported(C.byref(d), H, 7) == L.ts_lookahead_supported(C.byref(d), H, -1) == _cabi.ERR_ARG
                    # the call and the describe call refuse exactly the unsupported combinations with TS_ERR_LIMIT
                    mlp, tin, out = pc.Mlp(None, None, None, None, H, 0), lc.TrainIn(None, None, 1, 0), lc.LookaheadOut(None, None, None, None)
                    for leaf, ok in ((VALUE, want), (QMAX, want), (ZERO, zero)):
                        cfg = lc.LookaheadCfg(2, leaf, 1.0, 0.0, 1.0, 0.0)
                        code = _cabi.ERR_NULL if ok == 1 else _cabi.ERR_LIMIT
                        assert L.ts_lookahead(C.byref(d), None, C.byref(mlp), None, C.byref(tin), C.byref(cfg), C.byref(out), None) == code, (S, T, mc, H, leaf)
                        assert L.ts_describe_lookahead(C.byref(d), H, 1, 2, leaf, C.byref(lc.LookaheadDesc())) == (0 if ok == 1 else _cabi.ERR_LIMIT)
    assert seen == {0, 1, _cabi.ERR_DIMS}
    for d, H in ((_dims(4, 2, 0, Tt=8), 64), (_dims(4, 2, 0, Tt=9), 64), (_dims(33, 2), 8)):
        assert L.ts_lookahead_supported(C.byref(d), H, VALUE) == LP.ts_policy_supported(C.byref(d), H)
    assert L.ts_lookahead_supported(None, 8, VALUE) == _cabi.ERR_NULL
    assert lc.lookahead_supported(_dims(8, 8), 64, QMAX) and not lc.lookahead_supported(_dims(8, 8), 65, QMAX)
    assert lc.lookahead_supported(_dims(8, 8), 65, ZERO) and not lc.lookahead_supported(_dims(9, 8), 1, ZERO)
    with pytest.raises(_cabi.TilerSliderLibraryError):
        lc.lookahead_supported(_dims(0, 1), 8, VALUE)
    with pytest.raises(_cabi.TilerSliderLibraryError):
        lc.lookahead_supported(_dims(4, 2), 8, 3)


def test_argument_validation_precedes_any_launch():
    """Every refusal below returns its own status, in the header's order: a HIP call on a box without a GPU would have answered
    TS_ERR_HIP."""
    from tiler_slider_amd import _cabi, _policy_cabi as pc
    L = lc.lib()
    ok = _dims(4, 2)
    buf = (C.c_uint8 * 8192)()
    p = (C.addressof(buf) + 15) & ~15
    full = _cabi.State(p, p, p, p, p, p)
    net, head = pc.Mlp(p, p, p, p, 16, 0), lc.ValueHead(p, p)
    tin = lambda steps=3, first=p, log=p: lc.TrainIn(first, log, steps, 0)
    cfg = lambda depth=2, leaf=VALUE, gamma=0.5: lc.LookaheadCfg(depth, leaf, gamma, -1.0, 8.0, -2.0)
    out = lambda q=p, value=p, best=p, win_in=p: lc.LookaheadOut(q, value, best, win_in)
    ref = lambda x: C.byref(x) if x is not None else None
    call = lambda d, st, mlp, hd, i, c, o: L.ts_lookahead(ref(d), ref(st), ref(mlp), ref(hd), ref(i), ref(c), ref(o), None)
    # 1. dims - its TS_ERR_LIMIT before the NULL checks
    assert call(None, full, net, head, tin(), cfg(), out()) == _cabi.ERR_NULL
    assert call(_dims(0, 2), full, None, None, None, None, None) == _cabi.ERR_DIMS
    assert call(_dims(33, 2), full, None, None, None, None, None) == _cabi.ERR_LIMIT
    # 2. in / cfg / out, and mlp where the leaf reads a network (its width is the next check's)
    assert call(ok, full, net, head, None, cfg(), out()) == _cabi.ERR_NULL
    assert call(ok, full, net, head, tin(), None, out()) == _cabi.ERR_NULL
    assert call(ok, full, net, head, tin(), cfg(), None) == _cabi.ERR_NULL
    assert call(_dims(9, 1), full, net, head, tin(0), None, out()) == _cabi.ERR_NULL              # before the shape
    for leaf in (VALUE, QMAX):
        assert call(_dims(9, 1), full, None, head, tin(0), cfg(9, leaf, 2.0), out()) == _cabi.ERR_NULL
    # 3. unsupported shape or width, before the arguments - and before the head, which is a pointer like the others
    for S, T, H in ((9, 1, 16), (16, 2, 16), (8, 9, 16), (4, 2, 0), (4, 2, 65), (4, 2, -1)):
        assert call(_dims(S, T), full, pc.Mlp(p, p, p, p, H, 0), None, tin(0), cfg(0, VALUE, 2.0), out()) == _cabi.ERR_LIMIT
    assert call(_dims(4, 2, Tt=9), full, net, head, tin(), cfg(), out()) == _cabi.ERR_LIMIT
    assert call(_dims(9, 1), full, None, None, tin(0), cfg(0, ZERO, 2.0), out()) == _cabi.ERR_LIMIT       # LEAF_ZERO: the shape alone
    assert call(_dims(9, 1), full, None, None, tin(0), cfg(0, 7, 2.0), out()) == _cabi.ERR_LIMIT          # an unknown leaf too
    assert call(ok, full, pc.Mlp(p, p, p, p, 65, 0), None, tin(), cfg(2, ZERO), out(p + 4)) == _cabi.ERR_ARG   # LEAF_ZERO: no width is read
    # 4. bad arguments, before the empty batch and before any pointer
    empty = _dims(4, 2, 0, 0)
    for d in (ok, empty):
        for steps in (0, -1, MAX_STEPS + 1, 2**31 - 1):
            assert call(d, None, net, None, tin(steps), cfg(), out(None, None, None, None)) == _cabi.ERR_ARG, steps
        for depth in (0, -1, 5, 2**31 - 1):
            assert call(d, None, net, None, tin(), cfg(depth), out(None, None, None, None)) == _cabi.ERR_ARG, depth
        for leaf in (-1, 3, 255):
            assert call(d, None, None, None, tin(), cfg(2, leaf), out(None, None, None, None)) == _cabi.ERR_ARG, leaf
        for gamma in (-0.001, 1.001, float("nan"), float("inf"), -float("inf")):
            assert call(d, None, net, None, tin(), cfg(2, VALUE, gamma), out(None, None, None, None)) == _cabi.ERR_ARG, gamma
    for steps in (0, MAX_STEPS + 1):
        assert L.ts_describe_lookahead(C.byref(ok), 16, steps, 2, VALUE, C.byref(lc.LookaheadDesc())) == _cabi.ERR_ARG
    for depth in (0, 5):
        assert L.ts_describe_lookahead(C.byref(ok), 16, 1, depth, VALUE, C.byref(lc.LookaheadDesc())) == _cabi.ERR_ARG
    assert L.ts_describe_lookahead(C.byref(ok), 16, 1, 2, 3, C.byref(lc.LookaheadDesc())) == _cabi.ERR_ARG
    for steps, depth, gamma in ((1, 1, 0.0), (MAX_STEPS, 4, 1.0)):                                 # the edges are arguments
        assert call(ok, None, net, None, tin(steps), cfg(depth, VALUE, gamma), out(None, None, None, None)) == _cabi.ERR_NULL
    # 5. nothing to do: TS_OK without a launch, no further pointer is looked at
    assert call(empty, None, pc.Mlp(None, None, None, None, 1, 0), None, lc.TrainIn(None, None, 1, 0), cfg(), out(None, None, None, None)) == _cabi.OK
    assert call(empty, None, None, None, lc.TrainIn(None, None, 1, 0), cfg(2, ZERO), out(None, None, None, None)) == _cabi.OK
    # 6. missing pointers, before the alignment (p + 4: a misaligned q pointer; p + 2: a misaligned value pointer)
    bad = out(p + 4, p + 2)
    assert call(ok, None, net, head, tin(), cfg(), bad) == _cabi.ERR_NULL
    for missing in ("tgt", "blk"):
        st = _cabi.State(p, p, p, p, p, p)
        setattr(st, missing, None)
        assert call(ok, st, net, head, tin(), cfg(), bad) == _cabi.ERR_NULL, missing
    bare = _cabi.State(None, None, p, p, None, None)                                               # pos, init, step_count, done are never read
    assert call(ok, bare, net, head, tin(), cfg(), bad) == _cabi.ERR_ARG
    assert call(_dims(4, 2, Tt=0), _cabi.State(None, None, None, p, None, None), net, head, tin(), cfg(), bad) == _cabi.ERR_ARG   # no targets: no tgt
    assert call(ok, full, net, head, tin(first=None), cfg(), bad) == _cabi.ERR_NULL
    assert call(ok, full, net, head, tin(log=None), cfg(), bad) == _cabi.ERR_NULL
    assert call(ok, full, net, head, tin(1, log=None), cfg(), bad) == _cabi.ERR_ARG                # steps = 1 needs no log
    assert call(_dims(4, 0), full, net, head, tin(first=None, log=None), cfg(), bad) == _cabi.ERR_ARG   # no tiles: no cells
    for missing in ("w1", "b1", "w2", "b2"):
        mlp = pc.Mlp(p, p, p, p, 16, 0)
        setattr(mlp, missing, None)
        for leaf in (VALUE, QMAX):
            assert call(ok, full, mlp, head, tin(), cfg(2, leaf), bad) == _cabi.ERR_NULL, missing
        assert call(ok, full, mlp, None, tin(), cfg(2, ZERO), bad) == _cabi.ERR_ARG                # LEAF_ZERO reads no network
    for missing in ("wv", "bv"):
        hd = lc.ValueHead(p, p)
        setattr(hd, missing, None)
        assert call(ok, full, net, hd, tin(), cfg(), bad) == _cabi.ERR_NULL, missing
        assert call(ok, full, net, hd, tin(), cfg(2, QMAX), bad) == _cabi.ERR_ARG                  # LEAF_QMAX reads no head
    assert call(ok, full, net, None, tin(), cfg(), bad) == _cabi.ERR_NULL
    assert call(ok, full, net, None, tin(), cfg(2, QMAX), bad) == _cabi.ERR_ARG
    assert call(ok, full, None, None, tin(), cfg(2, ZERO), bad) == _cabi.ERR_ARG
    assert call(ok, full, net, head, tin(), cfg(), out(None, None, None, None)) == _cabi.ERR_NULL  # not all four
    # 7. alignment: 16 bytes for q, 4 for value; each output alone is enough to pass the NULL check
    for off in (4, 8, 12):
        assert call(ok, full, net, head, tin(), cfg(), out(p + off)) == _cabi.ERR_ARG
        assert call(ok, full, net, head, tin(), cfg(), out(p + off, None, None, None)) == _cabi.ERR_ARG
    for off in (1, 2, 3):
        assert call(ok, full, net, head, tin(), cfg(), out(p, p + off)) == _cabi.ERR_ARG
        assert call(ok, full, net, head, tin(), cfg(), out(None, p + off, None, None)) == _cabi.ERR_ARG
    assert L.ts_lookahead_last_hip_error() == 0
    assert L.ts_describe_lookahead(None, 16, 1, 2, VALUE, C.byref(lc.LookaheadDesc())) == _cabi.ERR_NULL
    assert L.ts_describe_lookahead(C.byref(ok), 16, 1, 2, VALUE, None) == _cabi.ERR_NULL
    got = lc.describe_lookahead(empty, 16, 7, 3, VALUE)
    assert (got["blocks"], got["name"], got["samples"], got["leaves"], got["depth"]) == (0, "", 0, 0, 3)


def _supported_shapes():
    for S in range(1, 9):
        for T in range(0, min(S * S, 8) + 1):
            yield S, T


def _expected_block(S, T, mc, H):
    """The forward block of the actor-critic library, which this library plans with unchanged: the second
    layer and the value head, the staged tile-plane weights where they fit beside the hs columns of 256, 128 or 64 threads."""
    head = 16 * H + 16 + ((4 * (H + 1) + 15) & ~15)
    wt = 0 if T == 0 else (H * (T if mc else 1) * S * S * 4 + 15) & ~15
    for threads in (256, 128, 64):
        if wt and head + wt + H * 4 * threads <= LDS_LIMIT:
            return threads, head + wt + H * 4 * threads, 1
    threads = next(t for t in (256, 128, 64) if head + H * 4 * t <= LDS_LIMIT)
    return threads, head + H * 4 * threads, 0


def test_describe_names_exactly_the_compiled_kernels_and_no_block_asks_for_more_than_64_kib():
    compiled = _kernel_names(lc.LIB_PATH)
    assert len(compiled) == lc.MIN_KERNELS == 32
    named, staged = set(), set()
    for S, T in _supported_shapes():
        for mc in (0, 1):
            for H in (1, 16, 29, 64):
                want = _expected_block(S, T, mc, H)
                for n, steps, depth in ((1, 1, 1), (257, 5, 2), (1 << 20, 100, 3), (4096, 3, 4)):
                    for leaf in (VALUE, QMAX, ZERO):
                        d = lc.describe_lookahead(_dims(S, T, mc, n), H, steps, depth, leaf)
                        assert d["name"] == f"k_lookahead<{S}, {depth}>" and d["depth"] == depth and d["leaf_is_template"] == 0
                        assert d["samples"] == n * steps and d["leaves"] == n * steps * 4 ** depth
                        block = want if leaf != ZERO else (256, 0, 0)
                        assert (d["threads_per_block"], d["lds_bytes"], d["weights_in_lds"]) == block, (S, T, mc, H, leaf, d)
                        assert d["blocks"] == -(-n // block[0]) and 0 <= d["lds_bytes"] <= LDS_LIMIT
                        named.add(d["name"])
                staged.add(want[2])
    assert sorted(named) == compiled and staged == {0, 1}


def test_where_the_tile_plane_weights_live_on_both_sides_of_the_boundary():
    """8x8 / 8 multi colour: a unit costs 2,048 bytes of staged weights, 256 of one wave's hs column and 20 of the second layer
    and the head: 28 units fit a block's 64 KiB in LDS, 29 are gathered from L2 - the width tests/test_gpu_lookahead.py runs."""
    at = lambda H, leaf=VALUE: lc.describe_lookahead(_dims(8, 8, 1, 1 << 16), H, 1, 2, leaf)
    modes = {H: at(H)["weights_in_lds"] for H in range(1, 65)}
    assert [H for H in range(2, 65) if modes[H] != modes[H - 1]] == [29] and modes[28] == 1 and modes[29] == 0
    head = lambda H: 16 * H + 16 + ((4 * (H + 1) + 15) & ~15)
    assert (at(28)["threads_per_block"], at(28)["lds_bytes"]) == (64, head(28) + 28 * 2048 + 28 * 256) and at(28)["lds_bytes"] <= LDS_LIMIT
    assert (at(29)["threads_per_block"], at(29)["lds_bytes"]) == (256, head(29) + 29 * 1024)
    assert at(29, QMAX) == at(29, VALUE) and at(29, ZERO)["lds_bytes"] == 0
    # cfg1's shape stages its weights at every width
    assert all(lc.describe_lookahead(_dims(4, 2, 0, 1 << 16), H, 1, 2, VALUE)["weights_in_lds"] == 1 for H in range(1, 65))


def test_every_lookahead_kernel_keeps_its_ply_stack_in_registers_and_its_lds_dynamic():
    """The code object's own metadata and instructions: no private segment (scratch), no scratch_ instruction, no static LDS, no
    accumulation registers (the hazard scan skips kernels that use them; a ply stack spilled into them is still a spill), no
    atomics, the one barrier of stage_weights, and the hazard scan clean over all 32 kernels."""
    kernels = _kernel_metadata(lc.LIB_PATH)
    assert len(kernels) == len([k for k in kernels if "k_lookahead" in k["name"]]) == lc.MIN_KERNELS
    assert not any(k["group_segment_fixed_size"] or k["private_segment_fixed_size"] or k["agpr_count"] or k["uses_dynamic_stack"] for k in kernels), kernels
    assert max(k["vgpr_count"] for k in kernels) <= 256
    pats = (r"\bscratch_\w+", r"\bs_barrier\b", r"\bds_(read|write|load|store)\w*", r"atomic", r"cmpswap")
    mine = {k: v for k, v in _instruction_counts(lc.LIB_PATH, pats).items() if "k_lookahead" in k}
    assert len(mine) == lc.MIN_KERNELS
    for k, (n_scratch, n_barrier, n_ds, n_atomic, n_cas) in mine.items():
        assert n_scratch == 0 and n_ds > 0 and n_atomic == 0 and n_cas == 0 and 1 <= n_barrier <= 2, (k, n_scratch, n_barrier, n_ds, n_atomic)
    class_a, class_b, n_kernels = _scan_last_vgpr(lc.LIB_PATH)
    assert n_kernels == lc.MIN_KERNELS and class_a == [] and class_b == []


# ---------------------------------------------------------------------------------------------- the yardstick itself
def _plain_search(S, mc, blocked, targets, cells, depth, gamma, w, leaf_fn):
    """The definition once more, one board at a time in plain Python on (row, column) tuples - its own slide, its own win test, a
    recursion: what the vectorised yardstick is checked against.  Returns (q [4], win_in)."""
    def slide(cells, a):
        dr, dc = ((-1, 0), (1, 0), (0, -1), (0, 1))[a]
        cells = list(cells)
        occupied = set(cells)
        order = sorted(range(len(cells)), key=lambda t: -(cells[t][0] * dr + cells[t][1] * dc))   # the tiles in front move first
        for t in order:
            r, c = cells[t]
            occupied.discard((r, c))
            while 0 <= r + dr < S and 0 <= c + dc < S and (r + dr, c + dc) not in blocked and (r + dr, c + dc) not in occupied:
                r, c = r + dr, c + dc
            cells[t] = (r, c)
            occupied.add((r, c))
        return tuple(cells)

    def won(cells):
        return list(cells) == list(targets) if mc else set(cells) == set(targets)

    def children(cells, plies):
        qs, wins = [], []
        for a in range(4):
            nxt = slide(cells, a)
            w_ = won(nxt)
            r = w[0] + w[1] * w_ + w[2] * (nxt == tuple(cells))
            if plies == 1:
                x, below = leaf_fn(nxt), 0
            else:
                cq, below = children(nxt, plies - 1)
                x = max(cq)
            qs.append(r + gamma * (0.0 if w_ else x))
            wins.append(1 if w_ else below + 1 if below else 0)
        return qs, min([x for x in wins if x], default=0)

    if won(cells):
        return [0.0] * 4, 0
    return children(tuple(cells), depth)


def test_the_yardstick_is_the_plain_recursion(oracle):
    """40 boards of 4x4 / 2 single colour and 5x5 / 3 multi colour, depths 1 .. 3, the three leaf kinds with an integer network:
    the frontier expansion on the oracle and the recursion on tuples give the same q, value, best and win_in, exactly."""
    import lookahead_reference as lr
    for S, T, K, mc in ((4, 2, 2, False), (5, 3, 3, True)):
        n = 40
        blk, init, tgt = lr.near_win_levels(oracle, S, T, K, n, mc)
        D = lr.features(S, T, T, mc)
        mlp, head = lr.int_network(np.random.default_rng(S), D, 5)
        rc = lambda a: [divmod(int(c), S) for c in a]
        for depth in (1, 2, 3):
            for leaf in (lr.LEAF_ZERO, lr.LEAF_VALUE, lr.LEAF_QMAX):
                got = lr.search(oracle, S, mc, blk, tgt, init, depth, leaf, 0.5, (-1.0, 8.0, -2.0), mlp, head)
                for m in range(n):
                    blocked = {divmod(i, S) for i in range(S * S) if (int(blk[i // 32, m]) >> (i % 32)) & 1}
                    lv = (np.ascontiguousarray(blk[:, m:m + 1]), np.ascontiguousarray(tgt[:, m:m + 1]))

                    def leaf_fn(cells, lv=lv):
                        if leaf == lr.LEAF_ZERO:
                            return 0.0
                        pos = np.array([[r * S + c] for r, c in cells], init.dtype)
                        return float(lr.leaf_values64(lr.planes(oracle, S, mc, lv[0], lv[1], pos), leaf, mlp, head)[0][0])

                    q, win = _plain_search(S, mc, blocked, rc(tgt[:, m]), rc(init[:, m]), depth, 0.5, (-1.0, 8.0, -2.0), leaf_fn)
                    assert got["q"][m].tolist() == q and got["win_in"][m] == win, (S, depth, leaf, m)
                    assert got["value"][m] == max(q) and got["best"][m] == (255 if got["won0"][m] else q.index(max(q)))
                assert got["won0"].any() or S == 5


def _leaf32(x, leaf, mlp, head, order, rng):
    """float32 leaf values of planes x in one of three orders of the features and the hidden units."""
    f32 = np.float32
    w1, b1, w2, b2 = mlp
    n, (H, D) = x.shape[0], w1.shape
    feats = {"forward": np.arange(D), "backward": np.arange(D)[::-1], "shuffled": rng.permutation(D)}[order]
    feats = feats[np.isin(feats, np.nonzero(x.any(axis=0))[0])]      # adding 0 * w is exact: skip the features no sample has
    pre = np.zeros((n, H), f32) if order == "shuffled" else np.broadcast_to(b1, (n, H)).astype(f32)
    for f in feats:
        pre = (pre + x[:, f:f + 1] * w1[None, :, f]).astype(f32)
    if order == "shuffled":
        pre = (pre + b1).astype(f32)
    h = np.maximum(pre, f32(0))
    units = {"forward": np.arange(H), "backward": np.arange(H)[::-1], "shuffled": rng.permutation(H)}[order]
    rows = np.concatenate([w2, head[0][None]], axis=0)
    out = np.broadcast_to(np.concatenate([b2, head[1]]), (n, 5)).astype(f32)
    for j in units:
        out = (out + (h[:, j:j + 1] * rows[None, :, j]).astype(f32)).astype(f32)
    return out[:, 4] if leaf == VALUE else out[:, :4].max(axis=1)


def _backup32(plies, won0, X, gamma, w, M, order):
    """The whole backup in float32: r and the multiply-add in one of three orders (left to right unfused, right to left unfused,
    r first and one fused multiply-add emulated in float64)."""
    f32, f64 = np.float32, np.float64
    g, (ws, ww, wi) = f32(gamma), (f32(v) for v in w)
    X = X.astype(f32)
    for ply in reversed(plies):
        won, inv = ply["won"], ply["invalid"]
        x = np.where(won, f32(0), X).astype(f32)
        a, b = np.where(won, ww, f32(0)).astype(f32), np.where(inv, wi, f32(0)).astype(f32)
        if order == "forward":
            q = (((ws + a).astype(f32) + b).astype(f32) + (g * x).astype(f32)).astype(f32)
        elif order == "backward":
            q = (ws + (a + (b + (g * x).astype(f32)).astype(f32)).astype(f32)).astype(f32)
        else:
            r = ((b + ws).astype(f32) + a).astype(f32)
            q = (r.astype(f64) + f64(g) * x.astype(f64)).astype(f32)
        X = q.reshape(q.shape[0] // (4 * M), 4, M).max(axis=1).reshape(-1)
    q = q.reshape(4, M).T.copy()
    q[won0] = 0
    return q


@pytest.mark.parametrize("S,T,K,mc,H,depth,leaf", ((4, 2, 2, False, 64, 2, VALUE), (5, 3, 3, True, 16, 2, QMAX), (4, 2, 2, False, 7, 3, VALUE)))
def test_the_bound_holds_float32_evaluations_of_the_whole_backup_in_three_orders(oracle, S, T, K, mc, H, depth, leaf):
    """10,000 random boards, Gaussian weights, gamma = 0.97, Gaussian reward weights: every float32 q of three evaluations - the
    network summed in three orders, the backup in three - lies within the yardstick's bound of the float64 one; the orders do
    differ, and the bound means something: its median is below 0.1 % of the median |q|."""
    import lookahead_reference as lr
    n = 10000
    rng = np.random.default_rng(100 * S + H + depth)
    blk, init, tgt = lr.near_win_levels(oracle, S, T, K, n, mc)
    D = lr.features(S, T, T, mc)
    import ac_reference as ar
    mlp, head = lr.pref.random_mlp(rng, D, H), ar.random_head(rng, H)
    gamma, w = 0.97, tuple(rng.standard_normal(3).astype(np.float32).tolist())
    want = lr.search(oracle, S, mc, blk, tgt, init, depth, leaf, gamma, w, mlp, head)
    plies = want["plies"]
    outs, worst = [], 0.0
    for order in ("forward", "backward", "shuffled"):
        X = lr.leaves(oracle, S, mc, blk, tgt, plies[-1], n, leaf, evaluate=lambda x: (_leaf32(x, leaf, mlp, head, order, rng), 0.0))[0]
        q = _backup32(plies, want["won0"], X, gamma, w, n, order)
        assert q.dtype == np.float32 and q.shape == (n, 4)
        err = np.abs(q.astype(np.float64) - want["q"])
        assert (err <= want["qbound"]).all(), (order, float((err / np.maximum(want["qbound"], 1e-300)).max()))
        worst = max(worst, float((err[~want["won0"]] / want["qbound"][~want["won0"]]).max()))
        outs.append(q)
    assert (outs[0] != outs[1]).any() and (outs[0] != outs[2]).any()
    ratio = float(np.median(want["qbound"][~want["won0"]]) / np.median(np.abs(want["q"][~want["won0"]])))
    print(f"{S}x{S}/{T} H={H} depth {depth} leaf {leaf}: worst float32 error / bound {worst:.3f}, median bound / median |q| {ratio:.2e}")
    assert worst > 1e-4 and ratio < 1e-3


# (S, T, obstacles, multi colour, boards): the seven shapes of the issue's table
SHAPES = ((2, 1, 0, False, 500), (3, 4, 1, False, 500), (4, 2, 2, False, 1000), (4, 2, 2, True, 1000), (5, 3, 3, True, 1000),
          (8, 2, 10, False, 500), (8, 8, 6, True, 500))


def test_the_inputs_of_the_gpu_tests_put_wins_inside_the_horizon(oracle):
    """near_win_levels on seven shapes from 2x2 / 1 to 8x8 / 8 multi colour, searched with an integer network (leaf "value" at
    depth 1, "qmax" at depth 3) and without one (plain reward search at depth 3): what every case of tests/test_gpu_lookahead.py
    asserts of its own inputs holds here - a win inside the horizon on at least 25 % of the boards, each action the best on at
    least 5 % of those not won on entry, an invalid root move on at least 1 %, and boards won on entry on every shape up to 4x4.
    (Printed: at depth 1 a win lies inside the horizon of 45 to 58 % of the boards; 2x2 / 1 is won on entry on 42 %.)"""
    import lookahead_reference as lr
    for S, T, K, mc, n in SHAPES:
        blk, init, tgt = lr.near_win_levels(oracle, S, T, K, n, mc)
        mlp, head = lr.int_network(np.random.default_rng(S), lr.features(S, T, T, mc), 16)
        for depth, leaf in ((1, VALUE), (3, ZERO), (3, QMAX)):
            c = lr.conditions(lr.search(oracle, S, mc, blk, tgt, init, depth, leaf, 0.5, (-1.0, 8.0, -2.0), mlp, head))
            print(S, T, mc, depth, leaf, c)
            assert c["win"] >= 0.25 and min(c["best"]) >= 0.05 and c["invalid"] >= 0.01, (S, T, depth, c)
            assert c["won0"] > 0 or S > 4, (S, T, c)
