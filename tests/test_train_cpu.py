"""The trainable policies without a GPU: the train library's C-ABI (include/tiler_slider_train.h), its launch plans, its code
object, and the CPU yardstick's gradient bound (tests/train_reference.py) against float32 evaluations in several orders."""
import ctypes as C
import os

import numpy as np
import pytest

from cabi_harness import _dims, _instruction_counts, _kernel_metadata, _kernel_names, _struct_fields
from conftest import ROOT
from tiler_slider_amd import _train_cabi  # noqa: F401  every test here, the yardstick's self-checks included, belongs to the training library

LDS_LIMIT = 65536
MAX_STEPS = 65535


def test_train_library_exports_what_its_header_declares():
    from tiler_slider_amd import _policy_cabi, _train_cabi as tc
    header = open(os.path.join(ROOT, "include", "tiler_slider_train.h")).read()
    assert '#include "tiler_slider_policy.h"' in header
    assert "ORDER OF THE SUMS IS NOT PART OF THE CONTRACT" in header and "NOT reproducible bit for bit" in header
    for struct, cls in (("ts_train_in", tc.TrainIn), ("ts_mlp_grad", tc.MlpGrad), ("ts_train_desc", tc.TrainDesc)):
        fields = _struct_fields(header, struct)
        assert fields == [f for f, _ in cls._fields_], struct
    assert C.sizeof(tc.TrainIn) == 24 and C.sizeof(tc.MlpGrad) == 32 and C.sizeof(tc.TrainDesc) == 112
    assert tc.Mlp is _policy_cabi.Mlp
    import tiler_slider_amd
    assert tiler_slider_amd.PolicyNet is not None and callable(tiler_slider_amd.build_train_library)
    assert callable(tiler_slider_amd.VecTilerSliderEnv.trajectory_logits) and callable(tiler_slider_amd.MlpPolicy.from_kernel_layout)
    assert "start_pos" in tiler_slider_amd.Rollout.__slots__


def test_train_supported_is_policy_supported():
    """S 0 .. 10, T -1 .. 10, both colour modes (and an invalid one), H in {0, 1, 64, 65}: the grid of tests/test_policy_cpu.py."""
    from tiler_slider_amd import _cabi, _policy_cabi as pc, _train_cabi as tc
    L, LP = tc.lib(), pc.lib()
    seen = set()
    for S in range(0, 11):
        for T in range(-1, 11):
            for mc in (0, 1, 2):
                d = _dims(S, T, mc)
                for H in (0, 1, 64, 65):
                    got = L.ts_train_supported(C.byref(d), H)
                    assert got == LP.ts_policy_supported(C.byref(d), H), (S, T, mc, H)
                    seen.add(got)
                    if got < 0:
                        continue
                    # the calls refuse exactly the unsupported combinations with TS_ERR_LIMIT
                    mlp, tin = pc.Mlp(None, None, None, None, H, 0), tc.TrainIn(None, None, 1, 0)
                    want = _cabi.ERR_NULL if got == 1 else _cabi.ERR_LIMIT
                    assert L.ts_train_forward(C.byref(d), None, C.byref(mlp), C.byref(tin), None, None) == want, (S, T, mc, H)
                    assert L.ts_train_backward(C.byref(d), None, C.byref(mlp), C.byref(tin), None, None, None) == want, (S, T, mc, H)
                    desc = tc.TrainDesc()
                    assert L.ts_describe_train_forward(C.byref(d), H, 1, C.byref(desc)) == (0 if got == 1 else _cabi.ERR_LIMIT)
                    assert L.ts_describe_train_backward(C.byref(d), H, 1, C.byref(desc)) == (0 if got == 1 else _cabi.ERR_LIMIT)
    assert seen == {0, 1, _cabi.ERR_DIMS}
    for d, H in ((_dims(4, 2, 0, Tt=8), 64), (_dims(4, 2, 0, Tt=9), 64), (_dims(33, 2), 8)):
        assert L.ts_train_supported(C.byref(d), H) == LP.ts_policy_supported(C.byref(d), H)
    assert L.ts_train_supported(None, 8) == _cabi.ERR_NULL
    assert tc.train_supported(_dims(8, 8), 64) and not tc.train_supported(_dims(8, 8), 65)
    with pytest.raises(_cabi.TilerSliderLibraryError):
        tc.train_supported(_dims(0, 1), 8)


def test_argument_validation_precedes_any_launch():
    """Every refusal below returns its own status, in the header's order: a HIP call on a box without a GPU would have answered
    TS_ERR_HIP."""
    from tiler_slider_amd import _cabi, _policy_cabi as pc, _train_cabi as tc
    L = tc.lib()
    ok = _dims(4, 2)
    buf = (C.c_uint8 * 8192)()
    p = (C.addressof(buf) + 15) & ~15
    full = _cabi.State(p, p, p, p, p, p)
    net = pc.Mlp(p, p, p, p, 16, 0)
    grad = tc.MlpGrad(p, p, p, p)
    tin = lambda steps=3, first=p, log=p: tc.TrainIn(first, log, steps, 0)
    ref = lambda x: C.byref(x) if x is not None else None
    fwd = lambda d, st, mlp, i, z: L.ts_train_forward(ref(d), ref(st), ref(mlp), ref(i), z, None)
    bwd = lambda d, st, mlp, i, dz, g: L.ts_train_backward(ref(d), ref(st), ref(mlp), ref(i), dz, ref(g), None)
    both = lambda d, st, mlp, i, z=p, g=grad: (fwd(d, st, mlp, i, z), bwd(d, st, mlp, i, z, g))
    same = lambda code: (code, code)
    # 1. dims - its TS_ERR_LIMIT before the NULL checks
    assert both(None, full, net, tin()) == same(_cabi.ERR_NULL)
    assert both(_dims(0, 2), full, None, None) == same(_cabi.ERR_DIMS)
    assert both(_dims(33, 2), full, None, None) == same(_cabi.ERR_LIMIT)
    # 2. mlp / in
    assert both(ok, full, None, tin()) == same(_cabi.ERR_NULL)
    assert both(ok, full, net, None) == same(_cabi.ERR_NULL)
    assert both(_dims(9, 1), full, None, tin(0)) == same(_cabi.ERR_NULL)          # mlp is needed to know the width
    # 3. unsupported shape or width, before the steps
    for S, T, H in ((9, 1, 16), (16, 2, 16), (8, 9, 16), (4, 2, 0), (4, 2, 65), (4, 2, -1)):
        assert both(_dims(S, T), full, pc.Mlp(p, p, p, p, H, 0), tin(0)) == same(_cabi.ERR_LIMIT)
    assert both(_dims(4, 2, Tt=9), full, net, tin()) == same(_cabi.ERR_LIMIT)
    # 4. steps outside 1 .. 65535, before the empty batch and before any pointer
    empty = _dims(4, 2, 0, 0)
    for steps in (0, -1, MAX_STEPS + 1, 2**31 - 1):
        assert both(ok, None, net, tin(steps), None, None) == same(_cabi.ERR_ARG), steps
        assert both(empty, None, net, tin(steps), None, None) == same(_cabi.ERR_ARG), steps
        assert L.ts_describe_train_backward(C.byref(ok), 16, steps, C.byref(tc.TrainDesc())) == _cabi.ERR_ARG
        assert L.ts_describe_train_forward(C.byref(ok), 16, steps, C.byref(tc.TrainDesc())) == _cabi.ERR_ARG
    assert both(ok, None, net, tin(MAX_STEPS), None, None) == same(_cabi.ERR_NULL)     # the edges are arguments
    assert both(ok, None, net, tin(1), None, None) == same(_cabi.ERR_NULL)
    # 5. nothing to do: TS_OK without a launch, no further pointer is looked at
    assert both(empty, None, pc.Mlp(None, None, None, None, 1, 0), tc.TrainIn(None, None, 1, 0), None, None) == same(_cabi.OK)
    # 6. missing pointers, before the alignment
    assert both(ok, None, net, tin(), p + 4) == same(_cabi.ERR_NULL)
    for missing in ("tgt", "blk"):
        st = _cabi.State(p, p, p, p, p, p)
        setattr(st, missing, None)
        assert both(ok, st, net, tin()) == same(_cabi.ERR_NULL), missing
    bare = _cabi.State(None, None, p, p, None, None)                                    # pos, init, step_count, done are never read
    assert both(ok, bare, net, tin(), p + 4) == same(_cabi.ERR_ARG)
    assert both(_dims(4, 2, Tt=0), _cabi.State(None, None, None, p, None, None), net, tin(), p + 4) == same(_cabi.ERR_ARG)   # no targets: no tgt
    assert both(ok, full, net, tin(first=None)) == same(_cabi.ERR_NULL)
    assert both(ok, full, net, tin(log=None)) == same(_cabi.ERR_NULL)
    assert both(ok, full, net, tin(1, log=None), p + 4) == same(_cabi.ERR_ARG)          # steps = 1 needs no log
    assert both(_dims(4, 0), full, net, tin(first=None, log=None), p + 4) == same(_cabi.ERR_ARG)   # no tiles: no cells
    for missing in ("w1", "b1", "w2", "b2"):
        mlp = pc.Mlp(p, p, p, p, 16, 0)
        setattr(mlp, missing, None)
        assert both(ok, full, mlp, tin()) == same(_cabi.ERR_NULL), missing
        g = tc.MlpGrad(p, p, p, p)
        setattr(g, missing, None)
        assert bwd(ok, full, net, tin(), p + 4, g) == _cabi.ERR_NULL, missing
    assert bwd(ok, full, net, tin(), p + 4, None) == _cabi.ERR_NULL
    assert both(ok, full, net, tin(), None) == same(_cabi.ERR_NULL)
    # 7. alignment
    for off in (4, 8, 12):
        assert both(ok, full, net, tin(), p + off) == same(_cabi.ERR_ARG)
    assert L.ts_train_last_hip_error() == 0
    for fn in (L.ts_describe_train_forward, L.ts_describe_train_backward):
        assert fn(None, 16, 1, C.byref(tc.TrainDesc())) == _cabi.ERR_NULL and fn(C.byref(ok), 16, 1, None) == _cabi.ERR_NULL
    for describe in (tc.describe_train_forward, tc.describe_train_backward):
        got = describe(empty, 16, 7)
        assert (got["blocks"], got["name"], got["samples"], got["flush_bytes"]) == (0, "", 0, 0)


def _supported_shapes():
    for S in range(1, 9):
        for T in range(0, min(S * S, 8) + 1):
            yield S, T


def _expected_forward(S, T, mc, H):
    """The forward's block is the policy library's (tests/test_policy_cpu.py: _expected_block)."""
    head = 16 * H + 16
    wt = 0 if T == 0 else (H * (T if mc else 1) * S * S * 4 + 15) & ~15
    for threads in (256, 128, 64):
        if wt and head + wt + H * 4 * threads <= LDS_LIMIT:
            return threads, head + wt + H * 4 * threads, 1
    threads = next(t for t in (256, 128, 64) if head + H * 4 * t <= LDS_LIMIT)
    return threads, head + H * 4 * threads, 0


def _expected_backward(S, T, mc, H):
    """The backward's plan restated from DESIGN.md section 16: one wave; always the second layer (16 H + 16), the hs and sd
    columns (2 x 256 H) and the accumulators of w2, b1, b2 (20 H + 16); then the whole w1 accumulator [H][D | 1] if it fits (2),
    else its tile planes [H][slots | 1] (1), else nothing (0); then the staged tile-plane weights if they still fit.
    Returns (lds_bytes, weights_in_lds, grads_in_lds, blocks of a large batch)."""
    C = S * S
    D, slots = (1 + 2 * T if mc else 3) * C, (T if mc else 1) * C
    fixed = (16 * H + 16) + 2 * 256 * H + (20 * H + 16)
    whole, tiles = 4 * H * (D | 1), 4 * H * (slots | 1)
    mode, acc = (2, whole) if fixed + whole <= LDS_LIMIT else (1, tiles) if T and fixed + tiles <= LDS_LIMIT else (0, 0)
    wt = 0 if T == 0 else (H * slots * 4 + 15) & ~15
    staged = int(wt > 0 and fixed + acc + wt <= LDS_LIMIT)
    lds = fixed + acc + staged * wt
    return lds, staged, mode, 256 * max(1, min(8, 160 * 1024 // lds))


def test_describe_names_exactly_the_compiled_kernels_and_no_block_asks_for_more_than_64_kib():
    from tiler_slider_amd import _train_cabi as tc
    compiled = _kernel_names(tc.LIB_PATH)
    assert len(compiled) == tc.MIN_KERNELS == 16
    named, modes, staged = set(), set(), set()
    for S, T in _supported_shapes():
        for mc in (0, 1):
            for H in (1, 16, 64):
                wf, wb = _expected_forward(S, T, mc, H), _expected_backward(S, T, mc, H)
                for n, steps in ((1, 1), (257, 5), (1 << 20, 100)):
                    f = tc.describe_train_forward(_dims(S, T, mc, n), H, steps)
                    assert f["name"] == f"k_train_forward<{S}>" and f["samples"] == n * steps and f["flush_bytes"] == 16 * n * steps
                    assert (f["threads_per_block"], f["lds_bytes"], f["weights_in_lds"], f["grads_in_lds"], f["chunk_steps"]) == wf + (0, 0)
                    assert f["blocks"] == -(-n // wf[0]) and 0 < f["lds_bytes"] <= LDS_LIMIT
                    b = tc.describe_train_backward(_dims(S, T, mc, n), H, steps)
                    assert b["name"] == f"k_train_backward<{S}>" and b["samples"] == n * steps and b["threads_per_block"] == 64
                    assert (b["lds_bytes"], b["weights_in_lds"], b["grads_in_lds"]) == wb[:3], (S, T, mc, H, b)
                    assert b["blocks"] == min(-(-n // 64), wb[3]) and 0 < b["lds_bytes"] <= LDS_LIMIT and b["chunk_steps"] == 4
                    acc = {2: (1 + 2 * T if mc else 3) * S * S, 1: (T if mc else 1) * S * S, 0: 0}[wb[2]]   # w1 rows accumulated in LDS
                    assert b["flush_bytes"] == b["blocks"] * 4 * (5 * H + 4 + acc * H)
                    named.update((f["name"], b["name"]))
                modes.add(wb[2])
                staged.add(wb[1])
    assert sorted(named) == compiled and modes == {0, 1, 2} and staged == {0, 1}
    import train_reference as tr
    assert sorted(tr.OCCUPANCY_CASES) == compiled      # tests/test_gpu_train.py runs one case per kernel at 4,096 waves


def test_where_the_gradients_live_on_both_sides_of_each_boundary():
    """8x8 with eight tiles in multi colour, D = 1,088 and 512 tile slots: a hidden unit costs 548 bytes of fixed LDS, 4,356 of a
    whole w1 accumulator (row stride 1,089), 2,052 of a tile-plane one (513).  13 units keep the whole gradient in LDS (63,784
    bytes), 14 only the tile planes (with the staged weights, 65,104); 25 still do (65,032), 26 keep none.  cfg1's shape keeps everything at every width."""
    from tiler_slider_amd import _train_cabi as tc
    at = lambda H, S=8, T=8, mc=1: tc.describe_train_backward(_dims(S, T, mc, 1 << 16), H, 16)
    pick = lambda d: (d["grads_in_lds"], d["weights_in_lds"], d["lds_bytes"])
    assert pick(at(13)) == (2, 0, 32 + 13 * (548 + 4356))
    assert pick(at(14)) == (1, 1, 32 + 14 * (548 + 2052 + 2048))   # 65,104: the staged weights (2,048 a unit) still fit beside it
    assert pick(at(15)) == (1, 0, 32 + 15 * (548 + 2052))
    assert pick(at(25)) == (1, 0, 32 + 25 * (548 + 2052))
    assert pick(at(26)) == (0, 0, 32 + 26 * 548)                   # 26 units of staged weights would not fit either
    assert pick(at(64)) == (0, 0, 32 + 64 * 548)
    for H in (1, 16, 64):                                          # 4x4 / 2 tiles, single colour: D = 48 (stride 49), 16 slots
        assert pick(at(H, 4, 2, 0)) == (2, 1, 32 + H * (548 + 196 + 64))
    # 5x5 / 3 multi colour: D = 175, 75 slots (19,200 bytes of weights at H = 64): the accumulator is preferred to the staged weights
    assert pick(at(16, 5, 3, 1)) == (2, 1, 32 + 16 * (548 + 700 + 300))
    assert pick(at(64, 5, 3, 1)) == (1, 0, 32 + 64 * (548 + 300))
    # no tiles: no tile planes; the whole accumulator or none
    assert pick(at(16, 4, 0, 1)) == (2, 0, 32 + 16 * (548 + 4 * 17))
    assert at(13)["blocks"] == 512 and at(64, 4, 2, 0)["blocks"] == 768 and at(1, 4, 2, 0)["blocks"] == 1024


def test_every_train_kernel_keeps_its_board_in_registers_and_its_lds_dynamic():
    """The code object's own metadata and instructions: no private segment (scratch), no scratch_ instruction, no static LDS
    (every byte of LDS is the dynamic allocation ts_describe_train_* reports), no accumulation registers (the hazard scan skips
    kernels that use them), and the float adds are single instructions: ds_add_f32 and global_atomic_add_f32 in every backward
    kernel, no compare-and-swap loop anywhere."""
    from tiler_slider_amd import _train_cabi as tc
    kernels = _kernel_metadata(tc.LIB_PATH)
    assert len(kernels) == len([k for k in kernels if "k_train_" in k["name"]]) == tc.MIN_KERNELS
    assert not any(k["group_segment_fixed_size"] or k["private_segment_fixed_size"] or k["agpr_count"] or k["uses_dynamic_stack"] for k in kernels), kernels
    pats = (r"\bscratch_\w+", r"\bs_barrier\b", r"\bds_(read|write|load|store)\w*", r"\bds_add_f32\b", r"\bglobal_atomic_add_f32\b", r"cmpswap")
    mine = {k: v for k, v in _instruction_counts(tc.LIB_PATH, pats).items() if "k_train_" in k}
    assert len(mine) == tc.MIN_KERNELS
    for k, (n_scratch, n_barrier, n_ds, n_ds_add, n_atomic, n_cas) in mine.items():
        assert n_scratch == 0 and n_ds > 0 and n_cas == 0, (k, n_scratch, n_ds, n_cas)
        if "backward" in k:   # one wave per block: the compiler drops the barriers of a block that is a single wave
            assert n_ds_add > 0 and n_atomic > 0 and n_barrier == 0, (k, n_ds_add, n_atomic, n_barrier)
        else:
            assert n_ds_add == 0 and n_atomic == 0 and 1 <= n_barrier <= 2, (k, n_ds_add, n_atomic, n_barrier)


# ---------------------------------------------------------------------------------------------- the yardstick itself
def _random_samples(oracle, S, T, mc, n, seed):
    blk, init, tgt = oracle.generate(S, T, T, 3, n, seed=seed)
    b = oracle.OracleBatch(S, mc, 100, blk, init, tgt)
    b.reset()
    return blk, init, tgt, b.encode_onehot().reshape(n, -1)


def test_the_numpy_planes_are_the_oracles_and_the_closed_form_is_autograds(oracle):
    import train_reference as tr
    for S, T, mc in ((4, 2, False), (5, 3, True), (8, 8, True), (3, 2, False)):
        blk, init, tgt, x = _random_samples(oracle, S, T, mc, 300, 0x7A1 + S)
        np.testing.assert_array_equal(tr.onehot(S, mc, blk, init, tgt), x)
        assert x.shape[1] == tr.features(S, T, T, mc)
    rng = np.random.default_rng(3)
    mlp = tr.pref.random_mlp(rng, x.shape[1], 7)
    dz = rng.standard_normal((300, 4))
    mine, theirs = tr.grads64(x, mlp, dz), tr.torch_grads64(x, mlp, dz)
    for name in ("w1", "b1", "w2", "b2"):
        assert mine[name].shape == theirs[name].shape
        assert np.abs(mine[name] - theirs[name]).max() <= 1e-11 * max(1.0, np.abs(theirs[name]).max()), name
    # a shared cell counts once, and two equal targets are one feature (single colour)
    cells = np.array([[5, 5], [5, 6]], np.uint8)
    tgt2 = np.array([[1, 2], [1, 200]], np.uint8)
    xs = tr.onehot(4, False, np.zeros((1, 2), np.uint32), cells, tgt2)
    assert xs[:, 16:32].sum(axis=1).tolist() == [1.0, 2.0] and xs[:, 32:].sum(axis=1).tolist() == [1.0, 2.0] and xs[1, 32 + 15] == 1.0
    assert tr.onehot(4, False, np.zeros((1, 2), np.uint32), cells, tgt2, sets=False)[0, 16 + 5] == 2.0


def _float32_gradients(x, mlp, dz, rng):
    """Three float32 evaluations of the four gradients: features / actions / samples first to last, last to first, and shuffled
    with pairwise sums over the samples."""
    w1, b1, w2, b2 = mlp
    n, (H, D) = x.shape[0], w1.shape
    f32 = np.float32
    outs = []
    for order in ("forward", "backward", "shuffled"):
        feats = {"forward": np.arange(D), "backward": np.arange(D)[::-1], "shuffled": rng.permutation(D)}[order]
        pre = np.zeros((n, H), f32) if order == "shuffled" else np.broadcast_to(b1, (n, H)).astype(f32)
        for f in feats:
            pre = (pre + x[:, f:f + 1] * w1[None, :, f]).astype(f32)
        if order == "shuffled":
            pre = (pre + b1).astype(f32)
        h = np.maximum(pre, f32(0))
        acts = {"forward": (0, 1, 2, 3), "backward": (3, 2, 1, 0), "shuffled": tuple(rng.permutation(4))}[order]
        dh = np.zeros((n, H), f32)
        for a in acts:
            dh = (dh + (dz[:, a:a + 1] * w2[None, a, :]).astype(f32)).astype(f32)
        dp = np.where(pre > 0, dh, f32(0)).astype(f32)
        rows = {"forward": np.arange(n), "backward": np.arange(n)[::-1], "shuffled": rng.permutation(n)}[order]

        def total(terms):   # [m, ...] float32 -> the sum over axis 0 in this order's way
            terms = np.ascontiguousarray(terms, dtype=f32)
            if terms.shape[0] == 0:
                return np.zeros(terms.shape[1:], f32)
            return terms.sum(axis=0, dtype=f32) if order == "shuffled" else np.cumsum(terms, axis=0, dtype=f32)[-1]

        g = {"b2": total(dz[rows]), "b1": total(dp[rows]),
             "w2": np.stack([total((h[rows] * dz[rows, a:a + 1]).astype(f32)) for a in range(4)], axis=1),
             "w1": np.stack([total(dp[rows][x[rows, f] > 0]) for f in range(D)], axis=0)}
        outs.append(g)
    return outs


@pytest.mark.parametrize("S,T,mc,H", ((4, 2, False, 64), (5, 3, True, 16)))
def test_the_gradient_bound_holds_float32_evaluations_in_three_orders_and_is_not_vacuous(oracle, S, T, mc, H):
    """10,000 random boards, Gaussian weights and dz: every float32 gradient entry lies within its bound of the float64 one, the
    orders do differ, and the bound means something: its median over all entries is below 1 % of the median |g|."""
    import train_reference as tr
    n = 10000
    rng = np.random.default_rng(S * 100 + H)
    _, _, _, x = _random_samples(oracle, S, T, mc, n, 0xB0D + S)
    mlp = tr.pref.random_mlp(rng, x.shape[1], H)
    dz = rng.standard_normal((n, 4)).astype(np.float32)
    want = tr.grads64(x, mlp, dz)
    bounds, ambiguous = tr.grad_bounds(x, mlp, dz)
    outs = _float32_gradients(x, mlp, dz, rng)
    worst = 0.0
    for got in outs:
        for name in ("w1", "b1", "w2", "b2"):
            assert got[name].dtype == np.float32 and got[name].shape == want[name].shape
            err = np.abs(got[name].astype(np.float64) - want[name])
            assert (err <= bounds[name]).all(), (name, float((err / np.maximum(bounds[name], 1e-300)).max()))
            worst = max(worst, float((err / np.maximum(bounds[name], 1e-300)).max()))
    assert any((outs[0][k] != o[k]).any() for o in outs[1:] for k in ("w1", "b1", "w2", "b2"))
    every = lambda d: np.concatenate([np.asarray(d[k], np.float64).ravel() for k in ("w1", "b1", "w2", "b2")])
    ratio = float(np.median(every(bounds)) / np.median(np.abs(every(want))))
    print(f"{S}x{S}/{T} H={H}: worst float32 error / bound {worst:.3f}, median bound / median |g| {ratio:.2e}, "
          f"ambiguous pairs {ambiguous.mean():.2e}")
    assert worst > 1e-4 and ratio < 0.01
    assert ambiguous.mean() <= 1e-4


def test_the_exact_comparison_notices_a_wrong_relu_derivative_and_a_missing_counts_once_rule():
    """Integer weights in [-2, 2], dz in {-1, 0, 1}, random cells in single colour (tiles do share cells): exactness_guard
    passes, and a gradient with relu'(0) = 1, or from planes that count a shared cell twice, differs from the yardstick's."""
    import train_reference as tr
    S, T, n, K, H = 4, 2, 257, 5, 7
    C_ = S * S
    rng = np.random.default_rng(9)
    blk = rng.integers(0, 1 << C_, (1, n)).astype(np.uint32) & rng.integers(0, 1 << C_, (1, n)).astype(np.uint32)
    first, pos_log = rng.integers(0, C_, (T, n)).astype(np.uint8), rng.integers(0, C_, (K, T, n)).astype(np.uint8)
    tgt = rng.integers(0, C_, (T, n)).astype(np.uint8)
    assert tr.shared_cell_share(first, pos_log, K, C_) >= 0.01
    x = tr.samples_onehot(S, False, blk, first, pos_log, tgt, K)
    assert x.shape == (K * n, 3 * C_) and set(np.unique(x)) == {0.0, 1.0}
    mlp = tr.int_mlp(rng, x.shape[1], H)
    dz = rng.integers(-1, 2, (K * n, 4)).astype(np.float32)
    assert tr.exactness_guard(x, mlp, dz)
    want = tr.grads64(x, mlp, dz)
    pre, _, _, _ = tr.forward64(x, mlp)
    dh = dz.astype(np.float64) @ mlp[2].astype(np.float64)
    assert ((pre == 0) & (dh != 0)).mean() >= 0.01
    wrong = tr.grads64(x, mlp, dz, relu_at_zero=1.0)
    assert (wrong["w1"] != want["w1"]).any() and (wrong["b1"] != want["b1"]).any()
    twice = tr.grads64(tr.samples_onehot(S, False, blk, first, pos_log, tgt, K, sets=False), mlp, dz)
    assert any((twice[k] != want[k]).any() for k in ("w1", "b1", "w2"))
    with pytest.raises(AssertionError):
        tr.exactness_guard(x, (mlp[0] * np.float32(2.0 ** 22),) + mlp[1:], dz)
    with pytest.raises(AssertionError):
        tr.exactness_guard(x, (mlp[0] + np.float32(0.5),) + mlp[1:], dz)
