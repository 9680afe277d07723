"""The neural-policy rollouts without a GPU: the policy library's C-ABI (include/tiler_slider_policy.h), its launch plan, its code
object, and the CPU yardstick's error bound (tests/policy_reference.py) against float32 evaluations in several orders."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cabi_harness import _dims, _instruction_counts, _kernel_metadata, _kernel_names, _struct_fields
from conftest import ROOT
from tiler_slider_amd import _policy_cabi  # noqa: F401  every test here, the yardstick's self-checks included, belongs to the policy library

LDS_LIMIT = 65536


def _cfg(steps=4, select=1, mode=0, write_state=1, **kw):
    from tiler_slider_amd import _policy_cabi as pc
    c = pc.PolicyCfg(steps, mode, select, write_state, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_policy_library_exports_what_its_header_declares():
    from tiler_slider_amd import _policy_cabi, _rollout_cabi
    header = open(os.path.join(ROOT, "include", "tiler_slider_policy.h")).read()
    assert '#include "tiler_slider_rollout.h"' in header
    for name, value in (("TS_POLICY_MAX_HIDDEN", _policy_cabi.POLICY_MAX_HIDDEN),
                        ("TS_POLICY_GREEDY", _policy_cabi.GREEDY), ("TS_POLICY_SAMPLE", _policy_cabi.SAMPLE)):
        assert int(re.search(rf"#define {name} \(?(-?\d+)\)?", header).group(1)) == value, name
    assert int(re.search(r"#define TS_POLICY_OUT_LOGITS_LOG (0x[0-9a-f]+)u", header).group(1), 16) == _policy_cabi.OUT_LOGITS_LOG == 0x200
    assert (_policy_cabi.GREEDY, _policy_cabi.SAMPLE, _policy_cabi.POLICY_MAX_HIDDEN) == (0, 1, 64)
    # the structures of the header, field by field
    for struct, cls in (("ts_mlp", _policy_cabi.Mlp), ("ts_policy_cfg", _policy_cabi.PolicyCfg), ("ts_policy_out", _policy_cabi.PolicyOut),
                        ("ts_policy_desc", _policy_cabi.PolicyDesc)):
        fields = _struct_fields(header, struct)
        assert fields == [f for f, _ in cls._fields_], struct
    assert _policy_cabi.OUT_FIELDS[:9] == _rollout_cabi.OUT_FIELDS and _policy_cabi.OUT_FIELDS[9] == "logits_log"
    assert C.sizeof(_policy_cabi.Mlp) == 40 and C.sizeof(_policy_cabi.PolicyCfg) == 48 and C.sizeof(_policy_cabi.PolicyDesc) == 96
    import tiler_slider_amd
    assert tiler_slider_amd.MlpPolicy is not None and callable(tiler_slider_amd.build_policy_library)
    assert callable(tiler_slider_amd.VecTilerSliderEnv.rollout_policy) and callable(tiler_slider_amd.VecTilerSliderEnv.policy_logits)
    assert "logits_log" in tiler_slider_amd.Rollout.__slots__


def test_policy_supported_is_the_random_rollouts_rule_for_every_allowed_width():
    """S 0 .. 10, T -1 .. 10, both colour modes (and an invalid one), H in {0, 1, 64, 65}."""
    from tiler_slider_amd import _cabi, _policy_cabi as pc, _rollout_cabi as rc
    L, LR = pc.lib(), rc.lib()
    seen = set()
    for S in range(0, 11):
        for T in range(-1, 11):
            for mc in (0, 1, 2):
                d = _dims(S, T, mc)
                random = LR.ts_rollout_supported(C.byref(d), rc.RANDOM)
                for H in (0, 1, 64, 65):
                    got = L.ts_policy_supported(C.byref(d), H)
                    if random < 0:
                        assert got == random == _cabi.ERR_DIMS, (S, T, mc, H)
                        continue
                    assert got == int(random == 1 and 1 <= H <= 64), (S, T, mc, H)
                    seen.add(got)
                    # the calls refuse exactly the unsupported combinations with TS_ERR_LIMIT
                    mlp = pc.Mlp(None, None, None, None, H, 0)
                    rcode = L.ts_policy_rollout(C.byref(d), None, C.byref(mlp), C.byref(_cfg()), None, None)
                    assert rcode == (_cabi.ERR_NULL if got == 1 else _cabi.ERR_LIMIT), (S, T, mc, H, rcode)
                    lcode = L.ts_policy_logits(C.byref(d), None, C.byref(mlp), None, None)
                    assert lcode == (_cabi.ERR_NULL if got == 1 else _cabi.ERR_LIMIT), (S, T, mc, H, lcode)
                    desc = pc.PolicyDesc()
                    assert L.ts_describe_policy_rollout(C.byref(d), H, C.byref(_cfg()), 0, C.byref(desc)) == (0 if got == 1 else _cabi.ERR_LIMIT)
                    assert L.ts_describe_policy_logits(C.byref(d), H, C.byref(desc)) == (0 if got == 1 else _cabi.ERR_LIMIT)
    assert seen == {0, 1}
    assert L.ts_policy_supported(C.byref(_dims(4, 2, 0, Tt=8)), 64) == 1 and L.ts_policy_supported(C.byref(_dims(4, 2, 0, Tt=9)), 64) == 0
    assert L.ts_policy_supported(C.byref(_dims(33, 2)), 8) == 0 and L.ts_policy_supported(None, 8) == _cabi.ERR_NULL
    assert pc.policy_supported(_dims(8, 8), 64) and not pc.policy_supported(_dims(8, 8), 65)
    with pytest.raises(_cabi.TilerSliderLibraryError):
        pc.policy_supported(_dims(0, 1), 8)


def test_argument_validation_precedes_any_launch():
    """Every refusal below returns its own status, in the header's order: a HIP call on a box without a GPU would have answered
    TS_ERR_HIP."""
    from tiler_slider_amd import _cabi, _policy_cabi as pc
    L = pc.lib()
    ok = _dims(4, 2)
    buf = (C.c_uint8 * 8192)()
    p = (C.addressof(buf) + 15) & ~15
    full = _cabi.State(p, p, p, p, p, p)
    net = pc.Mlp(p, p, p, p, 16, 0)
    outs = pc.PolicyOut(*([p] * 10))
    ref = lambda x: C.byref(x) if x is not None else None
    run = lambda d, st, mlp, cfg, out: L.ts_policy_rollout(ref(d), ref(st), ref(mlp), ref(cfg), ref(out), None)
    logits = lambda d, st, mlp, z: L.ts_policy_logits(ref(d), ref(st), ref(mlp), z, None)
    # dims, then cfg / mlp
    assert run(None, full, net, _cfg(), outs) == _cabi.ERR_NULL
    assert run(_dims(0, 2), full, None, None, outs) == _cabi.ERR_DIMS
    assert run(ok, full, net, None, outs) == _cabi.ERR_NULL
    assert run(ok, full, None, _cfg(), outs) == _cabi.ERR_NULL
    assert run(_dims(9, 1), full, None, _cfg(steps=-1), outs) == _cabi.ERR_NULL          # mlp is needed to know the width
    # unsupported shape or width
    for S, T, H in ((9, 1, 16), (16, 2, 16), (8, 9, 16), (4, 2, 0), (4, 2, 65), (4, 2, -1)):
        assert run(_dims(S, T), full, pc.Mlp(p, p, p, p, H, 0), _cfg(), outs) == _cabi.ERR_LIMIT
        assert logits(_dims(S, T), full, pc.Mlp(p, p, p, p, H, 0), p) == _cabi.ERR_LIMIT
    assert run(_dims(4, 2, Tt=9), full, net, _cfg(), outs) == _cabi.ERR_LIMIT
    # bad arguments: mode bits, select, steps, threshold
    bad = (_cfg(mode=2), _cfg(mode=0x80000000), _cfg(select=2), _cfg(select=-1), _cfg(steps=-1), _cfg(steps=65536), _cfg(steps=2**31 - 1),
           _cfg(explore_threshold=2**32 + 1), _cfg(explore_threshold=2**64 - 1))
    for cfg in bad:
        assert run(ok, full, net, cfg, outs) == _cabi.ERR_ARG, (cfg.mode, cfg.select, cfg.steps, cfg.explore_threshold)
        assert L.ts_describe_policy_rollout(C.byref(ok), 16, C.byref(cfg), 0, C.byref(pc.PolicyDesc())) == _cabi.ERR_ARG
    assert run(ok, full, net, _cfg(steps=65535, explore_threshold=2**32), None) == _cabi.ERR_NULL     # the edges are arguments
    # the order: unsupported, then bad argument, then missing pointer, then alignment
    assert run(_dims(9, 1), None, net, _cfg(steps=-1), None) == _cabi.ERR_LIMIT
    assert run(ok, None, pc.Mlp(None, None, None, None, 65, 0), _cfg(steps=-1), None) == _cabi.ERR_LIMIT
    assert run(ok, None, net, _cfg(steps=-1), None) == _cabi.ERR_ARG
    assert run(ok, None, net, _cfg(), None) == _cabi.ERR_NULL
    odd = pc.PolicyOut(*([p] * 9 + [p + 4]))
    assert run(ok, None, net, _cfg(), odd) == _cabi.ERR_NULL
    assert run(ok, full, net, _cfg(), odd) == _cabi.ERR_ARG
    # missing pointers
    assert run(ok, full, net, _cfg(), None) == _cabi.ERR_NULL
    for missing in ("pos", "tgt", "blk", "step_count", "done"):
        st = _cabi.State(p, p, p, p, p, p)
        setattr(st, missing, None)
        assert run(ok, st, net, _cfg(), outs) == _cabi.ERR_NULL, missing
    assert run(ok, _cabi.State(p, None, p, p, p, p), net, _cfg(mode=1), outs) == _cabi.ERR_NULL      # auto-reset reads the initial cells
    for missing in ("w1", "b1", "w2", "b2"):
        mlp = pc.Mlp(p, p, p, p, 16, 0)
        setattr(mlp, missing, None)
        assert run(ok, full, mlp, _cfg(), outs) == _cabi.ERR_NULL, missing
        assert logits(ok, full, mlp, p) == _cabi.ERR_NULL, missing
    assert run(ok, full, net, _cfg(write_state=0), pc.PolicyOut()) == _cabi.ERR_NULL                 # neither an output nor write_state
    # the logits call
    assert logits(None, full, net, p) == _cabi.ERR_NULL and logits(ok, full, None, p) == _cabi.ERR_NULL
    assert logits(_dims(0, 2), full, net, p) == _cabi.ERR_DIMS
    assert logits(ok, None, net, p) == _cabi.ERR_NULL and logits(ok, full, net, None) == _cabi.ERR_NULL
    for missing in ("pos", "tgt", "blk"):
        st = _cabi.State(p, p, p, p, p, p)
        setattr(st, missing, None)
        assert logits(ok, st, net, p) == _cabi.ERR_NULL, missing
    assert logits(ok, full, net, p + 8) == _cabi.ERR_ARG
    # nothing to do: TS_OK without a launch, no further pointer is looked at
    empty = _dims(4, 2, 0, 0)
    assert run(empty, None, net, _cfg(), None) == _cabi.OK and logits(empty, None, net, None) == _cabi.OK
    assert run(empty, full, net, _cfg(steps=-1), outs) == _cabi.ERR_ARG
    assert run(ok, None, net, _cfg(steps=0), None) == _cabi.OK
    assert run(ok, full, pc.Mlp(None, None, None, None, 1, 0), _cfg(steps=0), odd) == _cabi.OK
    assert L.ts_policy_last_hip_error() == 0
    assert L.ts_describe_policy_rollout(None, 16, C.byref(_cfg()), 0, C.byref(pc.PolicyDesc())) == _cabi.ERR_NULL
    assert L.ts_describe_policy_rollout(C.byref(ok), 16, None, 0, C.byref(pc.PolicyDesc())) == _cabi.ERR_NULL
    assert L.ts_describe_policy_rollout(C.byref(ok), 16, C.byref(_cfg()), 0, None) == _cabi.ERR_NULL
    assert L.ts_describe_policy_logits(None, 16, C.byref(pc.PolicyDesc())) == _cabi.ERR_NULL
    assert L.ts_describe_policy_logits(C.byref(ok), 16, None) == _cabi.ERR_NULL
    for d, cfg in ((empty, _cfg()), (ok, _cfg(steps=0))):
        got = pc.describe_policy_rollout(d, 16, cfg, 0x3ff)
        assert (got["blocks"], got["name"], got["logged_bytes"]) == (0, "", 0)
    assert pc.describe_policy_logits(empty, 16)["blocks"] == 0 and pc.describe_policy_logits(empty, 16)["name"] == ""


def _supported_shapes():
    for S in range(1, 9):
        for T in range(0, min(S * S, 8) + 1):
            yield S, T


def _expected_block(S, T, mc, H):
    """The plan of the header and DESIGN.md section 15, restated: the second layer (w2 and b2, 16 H + 16 bytes) in front, then the
    tile-plane weights [H][T' S S] (rounded up to 16 bytes), then hs [H][threads] float32; the most waves of four, two, one that
    fit 64 KiB with the weights staged, else the weights stay in global memory."""
    head = 16 * H + 16
    wt = 0 if T == 0 else (H * (T if mc else 1) * S * S * 4 + 15) & ~15
    for threads in (256, 128, 64):
        if wt and head + wt + H * 4 * threads <= LDS_LIMIT:
            return threads, head + wt + H * 4 * threads, 1
    threads = next(t for t in (256, 128, 64) if head + H * 4 * t <= LDS_LIMIT)
    return threads, head + H * 4 * threads, 0


def test_describe_names_exactly_the_compiled_kernels_and_no_block_asks_for_more_than_64_kib():
    from tiler_slider_amd import _policy_cabi as pc
    compiled = _kernel_names(pc.LIB_PATH)
    assert len(compiled) == pc.MIN_KERNELS == 24
    named, staged_seen = set(), set()
    for S, T in _supported_shapes():
        for mc in (0, 1):
            for H in (1, 7, 16, 28, 29, 64):
                want = _expected_block(S, T, mc, H)
                for n in (1, 257, 1 << 20):
                    lg = pc.describe_policy_logits(_dims(S, T, mc, n), H)
                    assert lg["name"] == f"k_policy_logits<{S}>" and lg["logged_bytes"] == 16 * n
                    assert (lg["threads_per_block"], lg["lds_bytes"], lg["weights_in_lds"]) == want, (S, T, mc, H)
                    assert lg["blocks"] == -(-n // want[0]) and 0 < lg["lds_bytes"] <= LDS_LIMIT
                    named.add(lg["name"])
                    for select in (pc.GREEDY, pc.SAMPLE):
                        for steps, mask in ((1, 0), (100, 0x040 | 0x100), (65535, 0x3ff)):
                            d = pc.describe_policy_rollout(_dims(S, T, mc, n), H, _cfg(steps=steps, select=select, mode=mc), mask)
                            assert d["name"] == f"k_policy_rollout<{S}, {select}>"
                            assert (d["threads_per_block"], d["lds_bytes"], d["weights_in_lds"]) == want, (S, T, mc, H)
                            assert d["blocks"] == -(-n // want[0]) and 0 < d["lds_bytes"] <= LDS_LIMIT
                            per_step = bool(mask & 0x040) + bool(mask & 0x080) + (T if mask & 0x100 else 0) + (16 if mask & 0x200 else 0)
                            assert d["logged_bytes"] == per_step * steps * n
                            named.add(d["name"])
                staged_seen.add(want[2])
    assert sorted(named) == compiled and staged_seen == {0, 1}
    import policy_reference as pref
    assert sorted(pref.OCCUPANCY_CASES) == compiled      # tests/test_gpu_policy.py runs one case per kernel at 4,096 waves
    for name, (S, T, K, select) in pref.OCCUPANCY_CASES.items():
        d = (pc.describe_policy_logits(_dims(S, T, 0, 4096 * 64), 64) if select is None else
             pc.describe_policy_rollout(_dims(S, T, 0, 4096 * 64), 64, _cfg(select=select), 0))
        assert d["name"] == name and d["blocks"] * (d["threads_per_block"] // 64) >= 4096


def test_the_lds_or_l2_decision_on_both_sides_of_its_boundary():
    """8x8 with eight tiles in multi colour, 512 slots: a hidden unit costs 16 bytes of w2, 2,048 bytes of tile-plane weights and
    256 bytes of one wave's hs.  28 units are 64,976 bytes with b2 - staged, one wave per block; 29 are 67,296 - the weights stay
    in global memory and the block gets its four waves back.  cfg1's shape stages at every width."""
    from tiler_slider_amd import _policy_cabi as pc
    at = lambda H, S=8, T=8, mc=1: pc.describe_policy_rollout(_dims(S, T, mc, 1 << 16), H, _cfg(), 0)
    d28, d29, d64 = at(28), at(29), at(64)
    assert (d28["weights_in_lds"], d28["threads_per_block"], d28["lds_bytes"]) == (1, 64, 16 + 28 * (16 + 2048 + 256))
    assert (d29["weights_in_lds"], d29["threads_per_block"], d29["lds_bytes"]) == (0, 256, 16 + 29 * (16 + 1024))
    assert (d64["weights_in_lds"], d64["threads_per_block"], d64["lds_bytes"]) == (0, 128, 16 + 64 * (16 + 512))
    assert d28["blocks"] == 1024 and d29["blocks"] == 256
    for H, threads in ((16, 256), (59, 256), (60, 128), (64, 128)):   # 4x4 / 2 tiles, single colour: 64 H bytes of weights, 65,152 in all at H = 59
        d = at(H, 4, 2, 0)
        assert (d["weights_in_lds"], d["threads_per_block"], d["lds_bytes"]) == (1, threads, 16 + H * (16 + 64 + 4 * threads)), H
    # no tiles: no tile planes, nothing to stage but the second layer
    assert at(16, 4, 0, 1)["weights_in_lds"] == 0 and at(16, 4, 0, 0)["weights_in_lds"] == 0
    assert at(16, 4, 0, 1)["lds_bytes"] == 16 + 16 * (16 + 1024)


def test_every_policy_kernel_keeps_its_board_in_registers_and_its_lds_dynamic():
    """The code object's own metadata and instructions: no private segment (scratch), no scratch_ instruction, no static LDS
    (every byte of LDS is the dynamic allocation ts_describe_policy_* reports); one barrier site per kernel at most twice (the
    staging), LDS instructions present."""
    from tiler_slider_amd import _policy_cabi as pc
    kernels = _kernel_metadata(pc.LIB_PATH)
    assert len(kernels) == len([k for k in kernels if "k_policy_" in k["name"]]) == pc.MIN_KERNELS
    assert not any(k["group_segment_fixed_size"] or k["private_segment_fixed_size"] or k["uses_dynamic_stack"] for k in kernels), kernels
    counts = _instruction_counts(pc.LIB_PATH, (r"\bscratch_\w+", r"\bs_barrier\b", r"\bds_(read|write|load|store)\w*"))
    mine = {k: v for k, v in counts.items() if "k_policy_" in k}
    assert len(mine) == pc.MIN_KERNELS
    for k, (n_scratch, n_barrier, n_ds) in mine.items():
        assert n_scratch == 0 and 1 <= n_barrier <= 2 and n_ds > 0, (k, n_scratch, n_barrier, n_ds)


def _float32_orders(x, mlp, rng):
    """Three float32 evaluations of the network on x [n, D]: features first to last, last to first, and pairwise in a random
    order with the bias added last; the second layer likewise."""
    w1, b1, w2, b2 = mlp
    n, (H, D) = x.shape[0], w1.shape
    outs = []
    for order in ("forward", "backward", "shuffled"):
        feats = {"forward": np.arange(D), "backward": np.arange(D)[::-1], "shuffled": rng.permutation(D)}[order]
        pre = np.zeros((n, H), np.float32) if order == "shuffled" else np.broadcast_to(b1, (n, H)).astype(np.float32)
        for f in feats:
            pre = (pre + x[:, f:f + 1] * w1[None, :, f]).astype(np.float32)
        if order == "shuffled":
            pre = (pre + b1).astype(np.float32)
        h = np.maximum(pre, np.float32(0))
        units = {"forward": np.arange(H), "backward": np.arange(H)[::-1], "shuffled": rng.permutation(H)}[order]
        z = np.zeros((n, 4), np.float32) if order == "shuffled" else np.broadcast_to(b2, (n, 4)).astype(np.float32)
        for j in units:
            z = (z + (h[:, j:j + 1] * w2[None, :, j]).astype(np.float32)).astype(np.float32)
        if order == "shuffled":
            z = (z + b2).astype(np.float32)
        outs.append(z)
    return outs


@pytest.mark.parametrize("S,T,mc,H", ((4, 2, False, 64), (5, 3, True, 16), (8, 8, True, 7)))
def test_the_yardsticks_bound_holds_float32_evaluations_in_three_orders(oracle, S, T, mc, H):
    """10,000 random boards, Gaussian weights: every float32 logit lies within the bound of the float64 one, the orders do differ
    (the bound is exercised, not vacuous), and it is tight enough to mean something: below 1e-4 of the logits' scale."""
    import policy_reference as pref
    n = 10000
    rng = np.random.default_rng(S * 100 + H)
    blk, init, tgt = oracle.generate(S, T, T, 3, n, seed=0xB0D + S)
    b = oracle.OracleBatch(S, mc, 100, blk, init, tgt)
    b.reset()
    x = b.encode_onehot().reshape(n, -1)
    assert x.shape[1] == (1 + 2 * T if mc else 3) * S * S and set(np.unique(x)) == {0.0, 1.0}
    mlp = pref.random_mlp(rng, x.shape[1], H)
    z, bound = pref.logits64(x, mlp)
    outs = _float32_orders(x, mlp, rng)
    worst = 0.0
    for got in outs:
        err = np.abs(got.astype(np.float64) - z)
        assert (err <= bound).all(), float((err / bound).max())
        worst = max(worst, float((err / bound).max()))
    assert any((outs[0] != o).any() for o in outs[1:])
    assert worst > 0.01 and float(bound.max()) < 1e-4 * max(1.0, float(np.abs(z).max()))
    print(f"{S}x{S}/{T} H={H}: worst float32 error / bound {worst:.3f}, largest bound {bound.max():.3g}, largest |z| {np.abs(z).max():.3g}")


def test_the_restated_selection_rule():
    import policy_reference as pref
    z = np.array([[1, 3, 3, 2], [5, 5, 5, 5], [0, -1, -2, 7], [2, 1, 2, 0]], np.float32)
    r = np.zeros(4, np.uint64)
    assert pref.select(z, r, pref.GREEDY).tolist() == [1, 0, 3, 0]
    # SAMPLE on uniform logits: u in [0, 1/4) -> 0, ... ; u = bits 32 .. 55
    zz = np.zeros((4, 4), np.float32)
    u24 = np.array([0, (1 << 22), (1 << 23) + 5, (1 << 24) - 1], np.uint64)
    rr = (u24 << np.uint64(32)) | np.uint64(0xff000000ffffffff)        # the other bits do not matter
    assert pref.select(zz, rr, pref.SAMPLE).tolist() == [0, 1, 2, 3]
    assert pref.uniforms(rr).tolist() == [0.0, 0.25, 0.5 + 5 * 2.0**-24, 1 - 2.0**-24]
    a, explore = pref.choose(z, np.array([3 << 62, (1 << 62) | 5, 4, 2 << 62], np.uint64), pref.GREEDY, 5)
    assert explore.tolist() == [True, False, True, True] and a.tolist() == [3, 0, 0, 2]
    assert pref.sample_margin(zz, rr).tolist() == [0.25, 0.0, 5 * 2.0**-24, 0.25 - 2.0**-24]
