"""The policy tables without a GPU: the ptable library's C-ABI (include/tiler_slider_ptable.h), its struct layout, its refusals in
the header's order, its launch plans against the kernels of its code object, the code object's properties, and the CPU
yardstick's own properties (tests/ptable_reference.py) on inputs that carry the cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ptable_reference as xref
import table_reference as tref
from cabi_harness import _dims, _kernel_metadata, _kernel_names, _struct_fields
from conftest import ROOT
from tiler_slider_amd import _cabi, _policy_cabi as pc, _ptable_cabi as xc, _table_cabi as tc

NULL, ARG, LIMIT, DIMS, OK = _cabi.ERR_NULL, _cabi.ERR_ARG, _cabi.ERR_LIMIT, _cabi.ERR_DIMS, _cabi.OK
# states -> (S, T): the index spaces the describe plans are checked at
SHAPES = {1: (1, 1), 16: (4, 1), 81: (3, 2), 256: (4, 2), 625: (5, 2), 4096: (8, 2), 59049: (3, 5), 65536: (4, 4)}


def test_ptable_library_exports_what_its_header_declares():
    header = open(os.path.join(ROOT, "include", "tiler_slider_ptable.h")).read()
    assert '#include "tiler_slider_table.h"' in header and '#include "tiler_slider_policy.h"' in header
    for name, value in (("TS_PTABLE_NO_ACTION", xc.NO_ACTION), ("TS_PTABLE_SCORE_COLUMNS", xc.SCORE_COLUMNS), ("TS_PTABLE_FORM_NONE", xc.FORM_NONE),
                        ("TS_PTABLE_FORM_WAVE", xc.FORM_WAVE), ("TS_PTABLE_FORM_BLOCK", xc.FORM_BLOCK), ("TS_PTABLE_FORM_FLAT", xc.FORM_FLAT)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value, name
    # the definitions are in the header in full
    for phrase in ("idx = sum_t cell_t * (S*S)^t", "TS_TABLE_INVALID (253)", "TS_TABLE_DEEP    (254)", "TS_TABLE_NONE    (255)", "bit-equal",
                   "the lowest action among the", "succ(i) = the placement after ts_step's move act[i] where act[i] <= 3, and i itself otherwise",
                   "the least d >= 1 with succ^d(i) won", "word for word", "table[n][succ(i)] = o - 1", "signed", "Checked in this order"):
        assert phrase in header, phrase
    assert _struct_fields(header, "ts_ptable_desc") == [f for f, _ in xc.PtableDesc._fields_]
    assert C.sizeof(xc.PtableDesc) == 104
    assert [(f, getattr(xc.PtableDesc, f).offset) for f, _ in xc.PtableDesc._fields_] == [
        ("form", 0), ("lanes_per_level", 4), ("threads_per_block", 8), ("lds_bytes", 12), ("weights_in_lds", 16), ("passes", 20), ("states", 24),
        ("blocks", 32), ("name", 40)]
    assert [(f, getattr(pc.Mlp, f).offset) for f, _ in pc.Mlp._fields_] == [("w1", 0), ("b1", 8), ("w2", 16), ("b2", 24), ("hidden", 32), ("reserved", 36)]
    import tiler_slider_amd as pkg
    assert callable(pkg.build_ptable_library) and {"PolicyTable", "PolicyScore", "build_ptable_library"} <= set(pkg.__all__)
    assert issubclass(pkg.PolicyTable, pkg.DistanceTable)
    for method in ("build_policy_table", "walk_actions", "score_policy"):
        assert callable(getattr(pkg.VecTilerSliderEnv, method)), method
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ts_ptable.hip" in design and "k_ptable_walk" in design and "LATER" in design


def test_supported_is_the_tables_and_the_policys():
    L, LT, LP = xc.lib(), tc.lib(), pc.lib()
    for S in range(0, 11):
        for T in range(-1, 8):
            for Tt in (0, 1, 8, 9):
                for mc in (0, 1, 2):
                    for hidden in (0, 1, 64, 65):
                        d = _dims(S, T, mc, Tt=Tt)
                        states, pol = LT.ts_table_states(C.byref(d)), LP.ts_policy_supported(C.byref(d), hidden)
                        want = states if states < 0 else int(states > 0 and pol == 1)
                        assert L.ts_ptable_supported(C.byref(d), hidden) == want, (S, T, Tt, mc, hidden)
    assert L.ts_ptable_supported(None, 1) == NULL
    assert xc.ptable_supported(_dims(4, 2), 16) and not xc.ptable_supported(_dims(5, 4), 16) and not xc.ptable_supported(_dims(4, 2), 65)
    with pytest.raises(_cabi.TilerSliderLibraryError):
        xc.ptable_supported(_dims(0, 1))


def test_every_refusal_has_its_own_status_in_the_headers_order():
    """No HIP call is made before a refusal: on a machine without a GPU one would have answered TS_ERR_HIP."""
    L = xc.lib()
    N = 8
    buf = (C.c_uint8 * (1 << 17))()
    base = (C.addressof(buf) + 255) & ~255
    at = lambda k: base + k * 4096         # regions apart: the largest, 8 levels x 256 states x 16 bytes, takes eight
    ok, empty = _dims(4, 2, n=N), _dims(4, 2, n=0)
    size = N * 256

    def state(**kw):
        a = dict(tgt=at(0), blk=at(1))
        a.update(kw)
        return _cabi.State(None, None, a["tgt"], a["blk"], None, None, None)   # pos, init, step_count, done are never read

    def mlp(hidden=16, **kw):
        a = dict(w1=at(2), b1=at(3), w2=at(4), b2=at(5))
        a.update(kw)
        return pc.Mlp(a["w1"], a["b1"], a["w2"], a["b2"], hidden, 0)

    ref_ = lambda x: C.byref(x) if x is not None else None
    unsupported = ((5, 4), (8, 3), (9, 1), (16, 2))

    # ---- ts_ptable_actions
    def actions(d=ok, st="default", m="default", act=at(6), logits=at(8)):
        st = state() if st == "default" else st
        m = mlp() if m == "default" else m
        return L.ts_ptable_actions(ref_(d), ref_(st), ref_(m), act, logits, None)

    # 1. dims: the shared check, before mlp
    assert actions(d=None) == NULL
    assert actions(d=_dims(0, 2), m=None) == DIMS and actions(d=_dims(4, 17), m=None) == DIMS and actions(d=_dims(4, 2, 2), m=None) == DIMS
    assert actions(d=_dims(33, 2), m=None) == LIMIT
    # 2. mlp, before the shape
    for S, T in ((4, 2),) + unsupported[:3]:
        assert actions(d=_dims(S, T), m=None) == NULL
    # 3. the shape and the width, before the empty batch
    for S, T in unsupported:
        assert actions(d=_dims(S, T), st=None, act=None) == LIMIT and actions(d=_dims(S, T, n=0)) == LIMIT
        assert L.ts_describe_ptable_actions(C.byref(_dims(S, T)), 16, C.byref(xc.PtableDesc())) == LIMIT
    for hidden in (0, -1, 65):
        assert actions(m=mlp(hidden), st=None) == LIMIT and actions(d=empty, m=mlp(hidden)) == LIMIT
        assert L.ts_describe_ptable_actions(C.byref(ok), hidden, C.byref(xc.PtableDesc())) == LIMIT
    assert actions(d=_dims(4, 2, Tt=9), st=None) == LIMIT
    # 4. the empty batch: TS_OK without a launch, no pointer is looked at
    assert actions(d=empty, st=None, m=mlp(w1=None), act=None, logits=at(8) + 4) == OK and actions(d=empty) == OK
    # 5. missing pointers, before the alignment (logits is misaligned throughout)
    off = at(8) + 4
    assert actions(st=None, logits=off) == NULL and actions(act=None, logits=off) == NULL
    for name in ("w1", "b1", "w2", "b2"):
        assert actions(m=mlp(**{name: None}), logits=off) == NULL, name
    assert actions(st=state(blk=None), logits=off) == NULL and actions(st=state(tgt=None), logits=off) == NULL
    assert actions(d=_dims(4, 2, n=N, Tt=0), st=state(tgt=None), logits=off) == ARG                 # no target: tgt is not needed
    # 6. the alignment of logits
    for k in (1, 4, 8, 15):
        assert actions(logits=at(8) + k) == ARG, k

    # ---- ts_ptable_walk
    def walk(d=ok, st="default", act=at(6), depth=252, dist=at(7)):
        st = state() if st == "default" else st
        return L.ts_ptable_walk(ref_(d), ref_(st), act, depth, dist, None)

    assert walk(d=None) == NULL and walk(d=_dims(0, 2), depth=-1) == DIMS and walk(d=_dims(33, 2), depth=-1) == LIMIT
    for S, T in unsupported:
        assert walk(d=_dims(S, T), depth=-1, st=None) == LIMIT                                      # the shape, before the arguments
        assert L.ts_describe_ptable_walk(C.byref(_dims(S, T)), C.byref(xc.PtableDesc())) == LIMIT
    assert walk(d=_dims(4, 2, Tt=9), depth=-1) == LIMIT
    for depth in (-1, 253, 2 ** 31 - 1):
        assert walk(depth=depth, st=None) == ARG and walk(d=empty, depth=depth) == ARG              # before the empty batch and any pointer
    assert walk(d=empty, st=None, act=None, dist=None) == OK and walk(d=empty) == OK
    same = dict(dist=at(6))                                                                          # an overlap that would be refused later
    assert walk(st=None, **same) == NULL and walk(act=None, dist=at(6)) == NULL and walk(dist=None) == NULL
    assert walk(st=state(blk=None), **same) == NULL and walk(st=state(tgt=None), **same) == NULL
    assert walk(d=_dims(4, 2, n=N, Tt=0), st=state(tgt=None), **same) == ARG
    assert walk(**same) == ARG and walk(dist=at(6) + size - 1) == ARG and walk(dist=at(6) - size + 1) == ARG   # byte-exactly

    # ---- ts_ptable_score
    def score(d=ok, st="default", p=at(6), a=at(7), t=at(9), s=at(10)):
        st = state() if st == "default" else st
        return L.ts_ptable_score(ref_(d), ref_(st), p, a, t, s, None)

    assert score(d=None) == NULL and score(d=_dims(0, 2)) == DIMS and score(d=_dims(33, 2)) == LIMIT
    for S, T in unsupported:
        assert score(d=_dims(S, T), st=None) == LIMIT
        assert L.ts_describe_ptable_score(C.byref(_dims(S, T)), C.byref(xc.PtableDesc())) == LIMIT
    assert score(d=empty, st=None, p=None, a=None, t=None, s=at(10) + 1) == OK
    odd = at(10) + 2
    assert score(st=None, s=odd) == NULL and score(p=None, s=odd) == NULL and score(a=None, s=odd) == NULL and score(t=None, s=odd) == NULL
    assert score(s=None) == NULL and score(st=state(blk=None), s=odd) == NULL
    assert score(st=state(tgt=None), s=odd) == ARG                                                  # the targets are not read
    for k in (1, 2, 3):
        assert score(s=at(10) + k) == ARG, k

    # ---- the describe calls
    for fn, args in ((L.ts_describe_ptable_actions, (16,)), (L.ts_describe_ptable_walk, ()), (L.ts_describe_ptable_score, ())):
        assert fn(None, *args, C.byref(xc.PtableDesc())) == NULL and fn(C.byref(ok), *args, None) == NULL
        assert fn(C.byref(_dims(0, 2)), *args, C.byref(xc.PtableDesc())) == DIMS
    assert L.ts_ptable_last_hip_error() == 0


def test_describe_plans_name_exactly_the_compiled_kernels():
    compiled = _kernel_names(xc.LIB_PATH)
    want_names = sorted([f"k_ptable_actions<{S}>" for S in range(1, 9)] + [f"k_ptable_walk_wave<{S}>" for S in range(1, 9)] +
                        [f"k_ptable_walk_block<{S}>" for S in range(2, 9)] + [f"k_ptable_score<{S}>" for S in range(1, 9)])
    assert len(compiled) == xc.MIN_KERNELS == 31 and compiled == want_names
    seen = set()
    pow2 = lambda v: 1 << (v - 1).bit_length()
    for states, (S, T) in SHAPES.items():
        words = -(-states // 32)
        for n in (1, 3, 4096, 1 << 15):
            for mc in (0, 1):
                d = _dims(S, T, mc, n)
                # the walk: the table build's rule
                w = xc.describe_ptable_walk(d)
                block = states > 1024 or (states >= 256 and n < 32768)
                lanes = 256 if block else min(64, pow2(states))
                per_block = 1 if block else 64 // lanes
                assert w["states"] == states == (S * S) ** T
                assert (w["form"], w["lanes_per_level"], w["threads_per_block"]) == (xc.FORM_BLOCK if block else xc.FORM_WAVE, lanes, 256 if block else 64), (states, n, w)
                assert w["name"] == f"k_ptable_walk_{'block' if block else 'wave'}<{S}>" and w["name"] in compiled
                assert w["lds_bytes"] == per_block * (3 * words + 2) * 4 <= 64 * 1024 and w["blocks"] == -(-n // per_block)
                assert w["passes"] == -(-states // lanes)
                # the score: a group per level, always
                s = xc.describe_ptable_score(d)
                lanes = min(64, pow2(states))
                assert (s["form"], s["lanes_per_level"], s["threads_per_block"], s["lds_bytes"]) == (xc.FORM_WAVE, lanes, 64, 0), (states, n, s)
                assert s["name"] == f"k_ptable_score<{S}>" and s["blocks"] == -(-n // (64 // lanes)) and s["passes"] == -(-states // lanes)
                # the actions: the policy library's block, a lane per placement
                for hidden in (1, 16, 64):
                    a, p = xc.describe_ptable_actions(d, hidden), pc.describe_policy_logits(_dims(S, T, mc, 1000), hidden)
                    assert (a["threads_per_block"], a["lds_bytes"], a["weights_in_lds"]) == (p["threads_per_block"], p["lds_bytes"], p["weights_in_lds"])
                    assert a["lds_bytes"] <= 64 * 1024 and a["threads_per_block"] in (64, 128, 256)
                    assert (a["form"], a["passes"], a["states"]) == (xc.FORM_FLAT, 1, states)
                    assert a["blocks"] == -(-(n * states) // a["threads_per_block"]) and a["lanes_per_level"] == min(states, a["threads_per_block"])
                    assert a["name"] == f"k_ptable_actions<{S}>"
                    seen.add(a["name"])
                seen |= {w["name"], s["name"]}
        for fn in (xc.describe_ptable_walk, xc.describe_ptable_score, lambda d: xc.describe_ptable_actions(d, 16)):
            nothing = fn(_dims(S, T, 0, 0))
            assert (nothing["form"], nothing["blocks"], nothing["name"], nothing["states"], nothing["passes"]) == (xc.FORM_NONE, 0, "", states, 0)
    # every compiled kernel is some supported shape's plan; and no supported shape takes the L2-gather plan of the tile-plane
    # weights: an index space of at most 65,536 placements has at most 128 tile slots (8x8 / 2 tiles, multi colour), 32 KiB at
    # 64 hidden units, which fits beside the hs columns of one wave - so there is one plan per table shape to cover on the GPU
    for S in range(1, 9):
        for T in range(0, 6):
            if T > S * S or tc.lib().ts_table_states(C.byref(_dims(S, T))) <= 0:
                continue
            for n in (1, 1 << 15):
                for mc in (0, 1):
                    d = _dims(S, T, mc, n)
                    a = xc.describe_ptable_actions(d, 64)
                    assert a["weights_in_lds"] == (1 if T > 0 else 0), (S, T, mc)
                    seen |= {xc.describe_ptable_walk(d)["name"], xc.describe_ptable_score(d)["name"], a["name"]}
    assert {s for s in seen if isinstance(s, str)} == set(compiled)


def test_the_ptable_kernels_use_no_scratch_no_static_lds_and_no_agprs():
    kernels = _kernel_metadata(xc.LIB_PATH)
    assert len(kernels) == len([k for k in kernels if "k_ptable_" in k["name"]]) == xc.MIN_KERNELS
    assert not any(k["group_segment_fixed_size"] or k["private_segment_fixed_size"] or k["agpr_count"] or k["uses_dynamic_stack"] for k in kernels), kernels
    assert max(k["vgpr_count"] for k in kernels) <= 64, kernels      # eight waves per SIMD


# ---------------------------------------------------------------------------------------------------------------- the yardstick
# (generate's arguments, multi colour): the inputs of the issue
INPUTS = (((4, 2, 2, 2, 1, 3), True), ((4, 2, 2, 2, 1, 5), False), ((8, 1, 1, 10, 4, 11), False))


@pytest.fixture(scope="module")
def voted(oracle):
    """(S, T, mc, blk, tgt, mlp, summary) of the three inputs, each with its expert-vote network."""
    out = []
    for (S, T, Tt, K, n, seed), mc in INPUTS:
        blk, _, tgt = oracle.generate(S, T, Tt, K, n, seed=seed)
        mlp = xref.expert_vote_mlp(oracle, S, mc, blk, tgt, T)
        out.append((S, T, mc, blk, tgt, mlp, xref.summary(oracle, S, mc, blk, tgt, T, mlp)))
    return out


def test_the_inputs_carry_the_cases(voted):
    """The yardstick's own numbers on the expert-vote networks: the figures of DESIGN.md section 24."""
    got = [{k: s[k] for k in ("valid", "solvable", "solved", "optimal", "with_excess", "dist_ge_3", "longest")} for *_, s in voted]
    print(got)
    assert got[0] == dict(valid=182, solvable=181, solved=87, optimal=85, with_excess=2, dist_ge_3=55, longest=7)
    assert got[1] == dict(valid=182, solvable=180, solved=126, optimal=118, with_excess=8, dist_ge_3=28, longest=3)
    assert (got[2]["solved"], got[2]["optimal"], got[2]["with_excess"], got[2]["longest"]) == (43, 25, 18, 10)
    for (S, T, mc, *_), s in ((v[:3], v[-1]) for v in voted):
        assert s["dist_ge_3"] >= 20 and s["with_excess"] >= 1 and s["never"] >= 20 and s["ties"] >= 0.01 and s["deep_at_2"] > 0, (S, T, mc, s)
        assert s["solved"] <= s["solvable"] and s["optimal"] <= s["solved"] and s["excess"] >= s["with_excess"]


def test_the_vote_networks_are_integer_and_identity_on_the_tile_planes(voted):
    for S, T, mc, blk, tgt, (w1, b1, w2, b2), _ in voted:
        C_ = S * S
        assert w1.shape == ((T * C_ if mc else C_), (1 + 2 * T if mc else 3) * C_) and w2.shape == (4, w1.shape[0])
        assert (w1.sum(axis=1) == 1).all() and (w1[:, :C_] == 0).all() and not b1.any() and not b2.any()
        assert (w2 == np.round(w2)).all() and (w2 >= 0).all() and w2.max() < 2 ** 16 and w2.sum() > 0


def test_walking_the_experts_actions_reproduces_the_distance_table(oracle, voted):
    for S, T, mc, blk, tgt, _, _ in voted:
        expert, _ = xref.expert_actions(oracle, S, mc, blk, tgt, T, tref.table(oracle, S, mc, blk, tgt, T))
        for max_depth in (0, 2, 252):
            want = tref.table(oracle, S, mc, blk, tgt, T, max_depth)
            np.testing.assert_array_equal(xref.walk(oracle, S, mc, blk, tgt, T, expert, max_depth), want)
        # and the expert's score against its own table is perfect
        want = tref.table(oracle, S, mc, blk, tgt, T)
        sc = xref.score(oracle, S, mc, blk, tgt, T, want, expert, want)
        assert (sc[:, 1] == sc[:, 2]).all() and (sc[:, 2] == sc[:, 3]).all() and (sc[:, 3] == sc[:, 4]).all() and not sc[:, 5].any()


def test_walk_and_score_on_any_bytes(oracle):
    """A tabular policy of random bytes: moves above 3 stand still, every distance is a chain that ends on a won placement, and
    the score's columns are consistent with each other."""
    rng = np.random.default_rng(5)
    for (S, T, Tt, K, n, seed), mc in INPUTS[:2]:        # levels on which nearly every placement can be solved
        blk, _, tgt = oracle.generate(S, T, Tt, K, n, seed=seed)
        valid, _ = xref.placements(S, blk, T)
        # the expert's move on two placements of three, any byte on the others: chains, detours, dead ends and bytes that are no move
        expert, _ = xref.expert_actions(oracle, S, mc, blk, tgt, T, tref.table(oracle, S, mc, blk, tgt, T))
        act = np.where(rng.random(valid.shape) < 2 / 3, expert, rng.integers(0, 256, valid.shape)).astype(np.uint8)
        act[:, 1::5] = rng.integers(0, 4, act[:, 1::5].shape)
        succ = xref.successors(oracle, S, mc, blk, tgt, T, act)
        assert (succ[act > 3] == np.broadcast_to(np.arange(valid.shape[1]), valid.shape)[act > 3]).all()
        pt, table = xref.walk(oracle, S, mc, blk, tgt, T, act), tref.table(oracle, S, mc, blk, tgt, T)
        assert ((pt == 253) == ~valid).all() and ((pt == 0) == (table == 0)).all() and not (pt == 254).any()
        dist = (pt >= 1) & (pt <= 252)
        assert dist.any() and (pt == 255).any()
        assert (np.take_along_axis(pt, succ, axis=1)[dist] == pt[dist] - 1).all()          # a chain, link by link
        assert (pt[dist] >= table[dist]).all() and (table[dist] <= 252).all()              # never better than the optimum
        sc = xref.score(oracle, S, mc, blk, tgt, T, pt, act, table)
        assert (sc[:, 0] == valid.sum(axis=1)).all() and (sc[:, 2] <= sc[:, 1]).all() and (sc[:, 3] <= sc[:, 2]).all()
        assert (sc[:, 5] >= 0).all() and (sc[:, 7] == (table == 0).sum(axis=1)).all() and not sc[:, 6].any()
        cut = xref.walk(oracle, S, mc, blk, tgt, T, act, 1)
        assert (cut == 254).any() and ((cut == 254) | (cut == pt))[valid].all()
        # over tables nobody built the score is still defined: excess is signed
        junk = rng.integers(0, 256, valid.shape).astype(np.uint8)
        sj = xref.score(oracle, S, mc, blk, tgt, T, junk, act, rng.integers(0, 256, valid.shape).astype(np.uint8))
        assert (sj[:, 0] == sc[:, 0]).all() and sj[:, 5].any() and (sj[:, 1:5] <= sj[:, :1]).all()
