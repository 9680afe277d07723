"""The mixed rollouts without a GPU: the library's C-ABI (include/tiler_slider_mixed.h), its launch plan, its code object, the
wrapper's refusals, and the conditions the CPU yardstick (tests/mixed_reference.py) meets on the inputs of
tests/test_gpu_mixed.py, so that the GPU test cannot pass on idle input."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cabi_harness import _declared, _dims, _exported, _instruction_counts, _kernel_metadata, _kernel_names, _scan_last_vgpr, _struct_fields
from conftest import ROOT
from tiler_slider_amd import _mixed_cabi as mc_

LDS_LIMIT = 65536
MAX_STEPS = 65535
GREEDY, SAMPLE = 0, 1
DENSE, REACH = 0, 1
TWO32 = 1 << 32


def test_mixed_library_exports_what_its_header_declares():
    from tiler_slider_amd import _cabi, _libraries, _policy_cabi
    L = mc_.lib()
    assert _exported(mc_.LIB_PATH) == _declared("tiler_slider_mixed.h") == sorted(mc_.EXPORTS) and len(mc_.EXPORTS) == 5
    assert L.ts_mixed_abi_version() == mc_.ABI_VERSION == 1
    assert mc_ in _libraries.SINCE and _libraries.name(mc_) == "mixed"
    header = open(os.path.join(ROOT, "include", "tiler_slider_mixed.h")).read()
    for name, value in (("ABI_VERSION", mc_.ABI_VERSION), ("DENSE", mc_.DENSE), ("REACH", mc_.REACH), ("WHO_NETWORK", mc_.WHO_NETWORK),
                        ("WHO_EXPERT", mc_.WHO_EXPERT), ("WHO_RANDOM", mc_.WHO_RANDOM)):
        assert int(re.search(rf"#define TS_MIXED_{name} (\d+)", header).group(1)) == value, name
    for name, value in (("SALT", mc_.SALT), ("OUT_EXPERT_LOG", mc_.OUT_EXPERT_LOG), ("OUT_MOVES_LOG", mc_.OUT_MOVES_LOG), ("OUT_BEST_LOG", mc_.OUT_BEST_LOG),
                        ("OUT_WHO_LOG", mc_.OUT_WHO_LOG)):
        assert int(re.search(rf"#define TS_MIXED_{name} (0x[0-9a-f]+)", header).group(1), 16) == value, name
    assert mc_.SALT == 0x6a09e667f3bcc909 and (mc_.DENSE, mc_.REACH) == (0, 1) and (mc_.WHO_NETWORK, mc_.WHO_EXPERT, mc_.WHO_RANDOM) == (0, 1, 2)
    # the definition, word for word
    prose = re.sub(r"[\s*]+", " ", header)
    for said in ("r = mix64(key_k + (board_offset + n) kDrawMul)", "rnd = r >> 62", "g = mix64(r ^ TS_MIXED_SALT), TS_MIXED_SALT = 0x6a09e667f3bcc909",
                 "teach = (g & 0xffffffff) < beta_threshold", "explore = (r & 0xffffffff) < explore_threshold",
                 "a = explore ? rnd : (teach && x != 255) ? x : e", "who = explore ? 2 : (teach && x != 255) ? 1 : 0",
                 "TS_MIXED_DENSE: ts_table_lookup(table, n_rows, rows)", "TS_MIXED_REACH: ts_rtable_lookup(table, slots, count, n_rows, rows)",
                 "the NETWORK plays, not the random draw", "No atomics are used"):
        assert said in prose, said
    for struct in ("ts_mlp", "ts_policy_cfg", "ts_policy_out"):
        assert not re.search(rf"typedef struct {struct} ", header), struct
    assert mc_.Mlp is _policy_cabi.Mlp
    policy_header = open(os.path.join(ROOT, "include", "tiler_slider_policy.h")).read()
    cfg_fields = _struct_fields(header, "ts_mixed_cfg")
    assert cfg_fields == [f for f, _ in mc_.MixedCfg._fields_]
    assert cfg_fields[:8] == _struct_fields(policy_header, "ts_policy_cfg")
    assert cfg_fields[8:] == ["beta_threshold", "kind", "reserved", "dense", "table", "slots", "count", "n_rows", "rows"]
    out_fields = _struct_fields(header, "ts_mixed_out")
    assert out_fields == [f for f, _ in mc_.MixedOut._fields_] == list(mc_.OUT_FIELDS)
    assert out_fields[:10] == _struct_fields(policy_header, "ts_policy_out") and out_fields[10:] == ["expert_log", "moves_log", "best_log", "who_log"]
    assert _struct_fields(header, "ts_mixed_desc") == [f for f, _ in mc_.MixedDesc._fields_]
    assert (C.sizeof(mc_.MixedCfg), C.sizeof(mc_.MixedOut), C.sizeof(mc_.MixedDesc)) == (48 + 8 + 8 + 6 * 8, 14 * 8, 16 + 16 + 64)
    assert (mc_.MixedCfg.beta_threshold.offset, mc_.MixedCfg.kind.offset, mc_.MixedCfg.dense.offset, mc_.MixedCfg.rows.offset) == (48, 56, 64, 104)
    P = C.c_void_p
    assert L.ts_mixed_rollout.argtypes == [C.POINTER(_cabi.Dims), C.POINTER(_cabi.State), C.POINTER(mc_.Mlp), C.POINTER(mc_.MixedCfg),
                                           C.POINTER(mc_.MixedOut), P]
    proto = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert ("int32_t ts_mixed_rollout(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_mixed_cfg *cfg, "
            "const ts_mixed_out *out, void *stream);") in proto
    assert ("int32_t ts_describe_mixed_rollout(const ts_dims *dims, int32_t hidden, const ts_mixed_cfg *cfg, uint32_t out_mask, "
            "ts_mixed_desc *desc);") in proto
    assert "int32_t ts_mixed_supported(const ts_dims *dims, int32_t hidden, int32_t kind);" in proto
    import tiler_slider_amd
    assert callable(tiler_slider_amd.build_mixed_library) and "build_mixed_library" in tiler_slider_amd.__all__
    assert set(tiler_slider_amd.Rollout.MIXED_LOGS) == {"expert_log", "moves_log", "best_log", "who_log"}
    import __graft_entry__ as entry
    assert callable(entry._smoke_mixed)


def test_mixed_supported_is_the_policys_shape_and_the_tables():
    """S 0 .. 10, T -1 .. 10, both colour modes (and an invalid one), H in {0, 1, 64, 65}: DENSE is ts_policy_supported and
    ts_table_states > 0, REACH is ts_policy_supported and ts_rtable_supported, an unknown kind is TS_ERR_ARG where the policy's shape
    is supported and 0 where it is not."""
    from tiler_slider_amd import _cabi, _policy_cabi as pc, _rtable_cabi as xc, _table_cabi as tc
    L, LP, LT, LX = mc_.lib(), pc.lib(), tc.lib(), xc.lib()
    seen = set()
    for S in range(0, 11):
        for T in range(-1, 11):
            for mc in (0, 1, 2):
                d = _dims(S, T, mc)
                for H in (0, 1, 64, 65):
                    pol = LP.ts_policy_supported(C.byref(d), H)
                    got = [L.ts_mixed_supported(C.byref(d), H, kind) for kind in (DENSE, REACH, 2, -1)]
                    seen.update(got)
                    if pol < 0:
                        assert got == [pol] * 4, (S, T, mc, H, got)
                        continue
                    dense = int(pol == 1 and LT.ts_table_states(C.byref(d)) > 0)
                    reach = int(pol == 1 and LX.ts_rtable_supported(C.byref(d)) == 1)
                    unknown = _cabi.ERR_ARG if pol == 1 else 0
                    assert got == [dense, reach, unknown, unknown], (S, T, mc, H, got)
    assert seen == {0, 1, _cabi.ERR_DIMS, _cabi.ERR_ARG}
    assert L.ts_mixed_supported(None, 8, DENSE) == _cabi.ERR_NULL
    assert L.ts_mixed_supported(C.byref(_dims(33, 2)), 8, 7) == 0
    assert mc_.mixed_supported(_dims(4, 4), 64, DENSE) and not mc_.mixed_supported(_dims(4, 5), 64, DENSE) and mc_.mixed_supported(_dims(4, 5), 64, REACH)
    assert mc_.mixed_supported(_dims(8, 8), 64, REACH) and not mc_.mixed_supported(_dims(8, 8), 65, REACH)
    with pytest.raises(_cabi.TilerSliderLibraryError):
        mc_.mixed_supported(_dims(0, 1), 8, DENSE)
    with pytest.raises(_cabi.TilerSliderLibraryError):
        mc_.mixed_supported(_dims(4, 2), 8, 2)


def _cfg(steps=3, mode=0, select=GREEDY, write_state=1, eps=0, beta=TWO32 // 2, kind=DENSE, dense=None, table=None, slots=8, count=None, n_rows=4,
         rows=None):
    return mc_.MixedCfg(steps, mode, select, write_state, 7, 0, 0, eps, beta, kind, 0, dense, table, slots, count, n_rows, rows)


def test_argument_validation_precedes_any_launch():
    """Every refusal below returns its own status, in the header's order: a HIP call on a box without a GPU would have answered
    TS_ERR_HIP."""
    from tiler_slider_amd import _cabi, _policy_cabi as pc
    L = mc_.lib()
    ok = _dims(4, 2)
    buf = (C.c_uint8 * 8192)()
    p = (C.addressof(buf) + 15) & ~15
    full = _cabi.State(p, p, p, p, p, p)
    net = pc.Mlp(p, p, p, p, 16, 0)
    nothing = mc_.MixedOut(*([None] * 14))
    out = lambda **kw: mc_.MixedOut(*(kw.get(f, p if f == "wins" else None) for f in mc_.OUT_FIELDS))
    ref = lambda x: C.byref(x) if x is not None else None
    call = lambda d, st, mlp, c, o: L.ts_mixed_rollout(ref(d), ref(st), ref(mlp), ref(c), ref(o), None)
    dense = lambda **kw: _cfg(kind=DENSE, dense=p, **kw)
    reach = lambda **kw: _cfg(kind=REACH, table=p, count=p, **kw)
    # 1. dims - its TS_ERR_LIMIT before the NULL checks
    assert call(None, full, net, dense(), out()) == _cabi.ERR_NULL
    assert call(_dims(0, 2), full, None, None, None) == _cabi.ERR_DIMS
    assert call(_dims(33, 2), full, None, None, None) == _cabi.ERR_LIMIT
    # 2. cfg / mlp
    assert call(ok, full, None, dense(), out()) == _cabi.ERR_NULL
    assert call(ok, full, net, None, out()) == _cabi.ERR_NULL
    assert call(_dims(9, 1), full, None, dense(), out()) == _cabi.ERR_NULL          # before the shape
    # 3. unsupported shape or width, before the arguments; an unknown kind: the policy's shape alone, then TS_ERR_ARG
    for S, T, H in ((9, 1, 16), (16, 2, 16), (8, 9, 16), (4, 2, 0), (4, 2, 65), (4, 2, -1)):
        for kind in (DENSE, REACH, 5):
            assert call(_dims(S, T), full, pc.Mlp(p, p, p, p, H, 0), _cfg(steps=-1, kind=kind), out()) == _cabi.ERR_LIMIT, (S, T, H, kind)
    assert call(_dims(4, 2, Tt=9), full, net, dense(), out()) == _cabi.ERR_LIMIT
    assert call(_dims(4, 5), full, net, dense(steps=-1), out()) == _cabi.ERR_LIMIT    # 16^5 placements: beyond the dense tables
    assert call(_dims(4, 5), full, net, reach(steps=-1), out()) == _cabi.ERR_ARG      # ... and inside the reach tables'
    assert call(_dims(4, 5), None, net, _cfg(kind=5), None) == _cabi.ERR_ARG
    assert call(ok, None, net, _cfg(kind=-1), None) == _cabi.ERR_ARG
    # 4. bad arguments, before the empty batch and before any pointer
    empty = _dims(4, 2, 0, 0)
    for d in (ok, empty):
        for make in (dense, reach):
            for bad in (dict(steps=-1), dict(steps=MAX_STEPS + 1), dict(mode=2), dict(mode=0x80000001), dict(select=2), dict(select=-1),
                        dict(eps=TWO32 + 1), dict(beta=TWO32 + 1), dict(n_rows=-1)):
                assert call(d, None, net, make(**bad), nothing) == _cabi.ERR_ARG, bad
        for slots in (0, 1, 3, 6, -8, 1 << 32):
            assert call(d, None, net, reach(slots=slots), nothing) == _cabi.ERR_ARG, slots
            assert call(d, None, net, dense(slots=slots), nothing) == (_cabi.OK if d is empty else _cabi.ERR_NULL), slots   # DENSE reads no slots
    for slots in (2, 1 << 31):
        assert call(ok, None, net, reach(slots=slots), nothing) == _cabi.ERR_NULL
    assert call(ok, None, net, dense(steps=MAX_STEPS, mode=1, select=SAMPLE, eps=TWO32, beta=TWO32, n_rows=0), nothing) == _cabi.ERR_NULL   # the edges are arguments
    d_ = mc_.MixedDesc()
    assert L.ts_describe_mixed_rollout(C.byref(ok), 16, C.byref(dense(steps=-1)), 0, C.byref(d_)) == _cabi.ERR_ARG
    assert L.ts_describe_mixed_rollout(C.byref(ok), 65, C.byref(dense(steps=-1)), 0, C.byref(d_)) == _cabi.ERR_LIMIT
    assert L.ts_describe_mixed_rollout(C.byref(ok), 16, C.byref(_cfg(kind=9)), 0, C.byref(d_)) == _cabi.ERR_ARG
    # 5. nothing to do: TS_OK without a launch, no further pointer is looked at
    for make in (dense, reach):
        assert call(empty, None, pc.Mlp(None, None, None, None, 1, 0), make(), None) == _cabi.OK
        assert call(ok, None, pc.Mlp(None, None, None, None, 1, 0), make(steps=0), None) == _cabi.OK
    # 6. missing pointers, before the alignment (p + 4: a misaligned logits_log; p + 1: a misaligned moves_log)
    bad = out(logits_log=p + 4, moves_log=p + 1)
    assert call(ok, None, net, dense(), bad) == _cabi.ERR_NULL
    assert call(ok, full, net, dense(), None) == _cabi.ERR_NULL
    for missing in ("pos", "tgt", "blk", "step_count", "done"):
        st = _cabi.State(p, p, p, p, p, p)
        setattr(st, missing, None)
        assert call(ok, st, net, dense(), bad) == _cabi.ERR_NULL, missing
    no_init = _cabi.State(p, None, p, p, p, p)
    assert call(ok, no_init, net, dense(mode=1), bad) == _cabi.ERR_NULL
    assert call(ok, no_init, net, dense(mode=0), bad) == _cabi.ERR_ARG               # init is read in auto-reset only
    for missing in ("w1", "b1", "w2", "b2"):
        mlp = pc.Mlp(p, p, p, p, 16, 0)
        setattr(mlp, missing, None)
        assert call(ok, full, mlp, dense(), bad) == _cabi.ERR_NULL, missing
    assert call(ok, full, net, dense(write_state=0), nothing) == _cabi.ERR_NULL     # neither an output nor write_state
    assert call(ok, full, net, dense(write_state=1), mc_.MixedOut(*([None] * 9 + [p + 4] + [None] * 4))) == _cabi.ERR_ARG
    # ... the table: missing only where it is read and n_rows > 0
    table_logs = (dict(expert_log=p), dict(moves_log=p), dict(best_log=p))
    for kind, gone in ((DENSE, dict(kind=DENSE)), (REACH, dict(kind=REACH, count=p)), (REACH, dict(kind=REACH, table=p))):
        assert call(ok, full, net, _cfg(**gone), bad) == _cabi.ERR_NULL, gone                               # beta > 0
        assert call(ok, full, net, _cfg(beta=0, **gone), out(logits_log=p + 4, who_log=p)) == _cabi.ERR_ARG, gone   # not read: who_log needs no table
        for log in table_logs:
            assert call(ok, full, net, _cfg(beta=0, **gone), out(logits_log=p + 4, **log)) == _cabi.ERR_NULL, (gone, log)
            assert call(ok, full, net, _cfg(beta=0, n_rows=0, **gone), out(logits_log=p + 4, **log)) == _cabi.ERR_ARG, (gone, log)
        assert call(ok, full, net, _cfg(n_rows=0, **gone), bad) == _cabi.ERR_ARG, gone
    # 7. alignment: 16 bytes for logits_log, 2 for moves_log
    for off in (4, 8, 12):
        assert call(ok, full, net, dense(), out(logits_log=p + off)) == _cabi.ERR_ARG
    assert call(ok, full, net, dense(), out(moves_log=p + 1)) == _cabi.ERR_ARG
    assert call(ok, full, net, reach(), out(moves_log=p + 3)) == _cabi.ERR_ARG
    assert L.ts_mixed_last_hip_error() == 0
    assert L.ts_describe_mixed_rollout(None, 16, C.byref(dense()), 0, C.byref(d_)) == _cabi.ERR_NULL
    assert L.ts_describe_mixed_rollout(C.byref(ok), 16, None, 0, C.byref(d_)) == _cabi.ERR_NULL
    assert L.ts_describe_mixed_rollout(C.byref(ok), 16, C.byref(dense()), 0, None) == _cabi.ERR_NULL
    got = mc_.describe_mixed_rollout(empty, 16, dense())
    assert (got["blocks"], got["name"], got["logged_bytes"], got["table_read"]) == (0, "", 0, 1)


def _expected_block(S, T, mc, H):
    """The forward block of the policy library, which this library plans with unchanged."""
    head = 16 * H + 16
    wt = 0 if T == 0 else (H * (T if mc else 1) * S * S * 4 + 15) & ~15
    for threads in (256, 128, 64):
        if wt and head + wt + H * 4 * threads <= LDS_LIMIT:
            return threads, head + wt + H * 4 * threads, 1
    threads = next(t for t in (256, 128, 64) if head + H * 4 * t <= LDS_LIMIT)
    return threads, head + H * 4 * threads, 0


def test_describe_names_exactly_the_compiled_kernels_and_no_block_asks_for_more_than_64_kib():
    from tiler_slider_amd import _policy_cabi as pc
    import mixed_reference as mx
    compiled = _kernel_names(mc_.LIB_PATH)
    assert len(compiled) == mc_.MIN_KERNELS == 32 and sorted(mx.OCCUPANCY_CASES) == compiled
    named, staged = set(), set()
    every = 0x3fff
    for S in range(1, 9):
        for T in range(0, min(S * S, 8) + 1):
            for mc in (0, 1):
                for H in (1, 16, 29, 64):
                    want = _expected_block(S, T, mc, H)
                    for n, steps in ((1, 1), (257, 5), (1 << 20, 100)):
                        for sel in (GREEDY, SAMPLE):
                            for kind in (DENSE, REACH):
                                if kind == DENSE and (S * S) ** T > 65536:
                                    continue
                                d = mc_.describe_mixed_rollout(_dims(S, T, mc, n), H, _cfg(steps=steps, select=sel, kind=kind), every)
                                assert d["name"] == f"k_mixed_rollout<{S}, {sel}, {kind}>"
                                assert (d["threads_per_block"], d["lds_bytes"], d["weights_in_lds"]) == want, (S, T, mc, H, d)
                                assert d["blocks"] == -(-n // want[0]) and 0 < d["lds_bytes"] <= LDS_LIMIT and d["table_read"] == 1
                                assert d["logged_bytes"] == n * steps * (1 + 1 + T + 16 + 1 + 2 + 1 + 1)
                                named.add(d["name"])
                    # the block is the policy library's for the same shape
                    p = pc.describe_policy_rollout(_dims(S, T, mc, 257), H, pc.PolicyCfg(5, 0, GREEDY, 1, 0, 0, 0, 0))
                    assert (p["threads_per_block"], p["lds_bytes"], p["weights_in_lds"]) == want
                    staged.add(want[2])
    assert sorted(named) == compiled and staged == {0, 1}
    # the table is read for beta > 0 or one of the three logs, and for nothing else
    at = lambda beta, mask: mc_.describe_mixed_rollout(_dims(4, 2, 0, 64), 8, _cfg(beta=beta), mask)["table_read"]
    assert [at(0, 0), at(0, 0x3ff | mc_.OUT_WHO_LOG), at(1, 0), at(TWO32, 0)] == [0, 0, 1, 1]
    assert [at(0, m) for m in (mc_.OUT_EXPERT_LOG, mc_.OUT_MOVES_LOG, mc_.OUT_BEST_LOG)] == [1, 1, 1]


def test_every_mixed_kernel_keeps_its_board_in_registers_and_its_lds_dynamic():
    """The code object's own metadata and instructions: no private segment (scratch), no scratch_ instruction, no static LDS, no
    accumulation registers, no atomics, the one barrier of stage_weights, and the hazard scan clean over all 32 kernels."""
    kernels = _kernel_metadata(mc_.LIB_PATH)
    assert len(kernels) == len([k for k in kernels if "k_mixed_rollout" in k["name"]]) == mc_.MIN_KERNELS
    assert not any(k["group_segment_fixed_size"] or k["private_segment_fixed_size"] or k["agpr_count"] or k["uses_dynamic_stack"] for k in kernels), kernels
    assert max(k["vgpr_count"] for k in kernels) <= 256
    pats = (r"\bscratch_\w+", r"\bs_barrier\b", r"\bds_(read|write|load|store)\w*", r"atomic", r"cmpswap")
    mine = {k: v for k, v in _instruction_counts(mc_.LIB_PATH, pats).items() if "k_mixed_rollout" in k}
    assert len(mine) == mc_.MIN_KERNELS
    for k, (n_scratch, n_barrier, n_ds, n_atomic, n_cas) in mine.items():
        assert n_scratch == 0 and n_ds > 0 and n_atomic == 0 and n_cas == 0 and 1 <= n_barrier <= 2, (k, n_scratch, n_barrier, n_ds, n_atomic)
    class_a, class_b, n_kernels = _scan_last_vgpr(mc_.LIB_PATH)
    assert n_kernels == mc_.MIN_KERNELS and class_a == [] and class_b == []


def test_the_source_restates_the_lookups_and_includes_the_network_unchanged():
    src = open(mc_.SRC).read()
    assert '#include "ts_mlp.h"' in src and '#include "../../include/tiler_slider_mixed.h"' in src
    for other in ("ts_policy.hip", "ts_rexpert.hip", "ts_table.hip", "ts_rtable.hip", "ts_targets.hip"):
        assert f'#include "{other}"' not in src
    assert "0x9e3779b97f4a7c15" in src and "atomic" not in src.lower().replace("no atomics", "")
    assert os.path.join(ROOT, "tiler_slider_amd", "csrc", "ts_mlp.h") in mc_.HEADERS


def test_the_wrapper_refuses_what_it_cannot_play():
    """rollout_policy's three new arguments, checked before any device is touched (the environment is never constructed)."""
    import inspect
    from tiler_slider_amd import VecTilerSliderEnv
    from tiler_slider_amd import mixed
    sig = inspect.signature(VecTilerSliderEnv.rollout_policy)
    assert [(n, sig.parameters[n].default) for n in ("expert", "beta", "rows")] == [("expert", None), ("beta", 0.0), ("rows", None)]
    assert list(sig.parameters)[-3:] == ["expert", "beta", "rows"]
    env = object.__new__(VecTilerSliderEnv)
    for kw in (dict(beta=0.5), dict(rows=[0]), dict(beta=1.0, rows=[0])):
        with pytest.raises(ValueError, match="expert"):
            env.rollout_policy(3, None, **kw)
    assert mixed.EXPERT_LOGS == ("expert", "moves", "best", "who")


# ---------------------------------------------------------------------------------------------- the yardstick and its inputs
def test_teach_is_an_independent_draw_of_the_right_rate():
    import mixed_reference as mx
    import rollout_reference as rref
    r = np.concatenate([rref.draws(4096, 7, k) for k in range(24)])
    teach = mx.teach_of(r, TWO32 // 2)
    explore = (r & np.uint64(0xffffffff)) < np.uint64(TWO32 // 8)
    assert abs(teach.mean() - 0.5) < 0.01 and abs(explore.mean() - 0.125) < 0.01
    assert abs((teach & explore).mean() - 0.0625) < 0.005            # independent of the explore bits
    rnd = (r >> np.uint64(62)).astype(int)
    assert all(abs(teach[rnd == a].mean() - 0.5) < 0.02 for a in range(4))
    assert not mx.teach_of(r, 0).any() and mx.teach_of(r, TWO32).all()


@pytest.mark.parametrize("mode", (0, 1), ids=("strict", "autoreset"))
@pytest.mark.parametrize("mc", (False, True))
@pytest.mark.parametrize("S", (2, 3, 4, 5, 6, 7, 8))
def test_the_reach_base_cases_meet_the_floors(oracle, S, mc, mode):
    import mixed_reference as mx
    assert mx.REACH_SIZES == (2, 3, 4, 5, 6, 7, 8) and mx.BASE == dict(levels=128, steps=24, max_steps=12, beta=0.5, epsilon=0.125, seed=7, hidden=8)
    assert mx.FLOORS == dict(expert=15, expert_differs=15, random=300, network=2000, teach_no_move=500, wins=5, timeouts=25, resets=150, kinds=50)
    want = mx.base_case(oracle, mx.REACH, S, mc, mode)[3]
    print(S, mc, mode, mx.check_base(mx.REACH, S, mode, want))


@pytest.mark.parametrize("mode", (0, 1), ids=("strict", "autoreset"))
@pytest.mark.parametrize("mc", (False, True))
@pytest.mark.parametrize("shape", ((2, 2, 0), (3, 2, 1), (4, 2, 2), (5, 2, 3), (6, 2, 4), (7, 2, 6), (8, 2, 8), (4, 4, 2), (6, 3, 4)))
def test_the_dense_base_cases_meet_the_floors(oracle, shape, mc, mode):
    import mixed_reference as mx
    assert shape in mx.DENSE_SHAPES and len(mx.DENSE_SHAPES) == 9
    want = mx.base_case(oracle, mx.DENSE, shape, mc, mode)[3]
    print(shape, mc, mode, mx.check_base(mx.DENSE, shape[0], mode, want))


def test_the_yardstick_without_a_table_is_the_policy_yardstick(oracle):
    """beta = 0 and no table: every output of policy_reference.rollout, and who_log is the explore bit."""
    import mixed_reference as mx
    import policy_reference as pref
    import rollout_reference as rref
    (blk, init, tgt), _, mlp, _ = mx.base_case(oracle, mx.DENSE, (4, 2, 2), False, 1)
    thr = rref.threshold_of(0.125)
    a = mx.rollout(oracle, mx.DENSE, None, 4, False, 12, blk, init, tgt, mlp, 24, pref.GREEDY, 1, threshold=thr, seed=7)
    b = pref.rollout(oracle, 4, False, 12, blk, init, tgt, mlp, 24, pref.GREEDY, 1, threshold=thr, seed=7, exact32=True)
    for k in pref.OUTPUTS + ("pos", "step_count", "done"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert "expert_log" not in a and set(np.unique(a["who_log"])) == {0, 2} and int((a["who_log"] == 2).sum()) == b["explored"]
