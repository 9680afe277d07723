"""The actor-critic network without a GPU: the actor-critic library's C-ABI (include/tiler_slider_ac.h), its launch plans, its code
object, and the CPU yardstick (tests/ac_reference.py) against float64 autograd and float32 evaluations in several orders."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cabi_harness import _declared, _dims, _instruction_counts, _kernel_metadata, _kernel_names, _struct_fields
from conftest import ROOT
from tiler_slider_amd import _ac_cabi  # noqa: F401  every test here, the yardstick's self-checks included, belongs to the actor-critic library

LDS_LIMIT = 65536
MAX_STEPS = 65535


def test_ac_library_exports_what_its_header_declares():
    from tiler_slider_amd import _ac_cabi as ac, _cabi, _policy_cabi, _train_cabi
    L = ac.lib()
    assert len(_declared("tiler_slider_ac.h")) == 7
    header = open(os.path.join(ROOT, "include", "tiler_slider_ac.h")).read()
    assert '#include "tiler_slider_train.h"' in header
    prose = re.sub(r"[\s*]+", " ", header)
    assert "ORDER OF THE SUMS IS NOT PART OF THE CONTRACT" in prose and "NOT reproducible bit for bit" in prose
    for struct, cls in (("ts_value_head", ac.ValueHead), ("ts_value_head_grad", ac.ValueHeadGrad)):
        fields = _struct_fields(header, struct)
        assert fields == [f for f, _ in cls._fields_] == ["wv", "bv"], struct
        assert C.sizeof(cls) == 16 and all(t is C.c_void_p for _, t in cls._fields_)
    # the samples, the four gradient buffers and the description are the training library's own types
    assert ac.TrainIn is _train_cabi.TrainIn and ac.MlpGrad is _train_cabi.MlpGrad and ac.TrainDesc is _train_cabi.TrainDesc
    assert ac.Mlp is _policy_cabi.Mlp
    # the argument order of the header, argument by argument
    P = C.c_void_p
    assert L.ts_ac_forward.argtypes == [C.POINTER(_cabi.Dims), C.POINTER(_cabi.State), C.POINTER(ac.Mlp), C.POINTER(ac.ValueHead),
                                        C.POINTER(ac.TrainIn), P, P, P]
    assert L.ts_ac_backward.argtypes == [C.POINTER(_cabi.Dims), C.POINTER(_cabi.State), C.POINTER(ac.Mlp), C.POINTER(ac.ValueHead),
                                         C.POINTER(ac.TrainIn), P, P, C.POINTER(ac.MlpGrad), C.POINTER(ac.ValueHeadGrad), P]
    proto = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert ("int32_t ts_ac_forward(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_value_head *head, "
            "const ts_train_in *in, float *logits, float *values, void *stream);") in proto
    assert ("int32_t ts_ac_backward(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_value_head *head, "
            "const ts_train_in *in, const float *dlogits, const float *dvalues, const ts_mlp_grad *grad, "
            "const ts_value_head_grad *head_grad, void *stream);") in proto
    import tiler_slider_amd
    assert tiler_slider_amd.ActorCriticNet is not None and callable(tiler_slider_amd.build_ac_library)
    assert callable(tiler_slider_amd.VecTilerSliderEnv.trajectory_outputs)
    assert {"ActorCriticNet", "build_ac_library"} <= set(tiler_slider_amd.__all__)


def test_ac_supported_is_policy_supported():
    """S 0 .. 10, T -1 .. 10, both colour modes (and an invalid one), H in {0, 1, 64, 65}: the grid of tests/test_policy_cpu.py."""
    from tiler_slider_amd import _ac_cabi as ac, _cabi, _policy_cabi as pc
    L, LP = ac.lib(), pc.lib()
    seen = set()
    for S in range(0, 11):
        for T in range(-1, 11):
            for mc in (0, 1, 2):
                d = _dims(S, T, mc)
                for H in (0, 1, 64, 65):
                    got = L.ts_ac_supported(C.byref(d), H)
                    assert got == LP.ts_policy_supported(C.byref(d), H), (S, T, mc, H)
                    seen.add(got)
                    if got < 0:
                        continue
                    # the calls refuse exactly the unsupported combinations with TS_ERR_LIMIT
                    mlp, tin = pc.Mlp(None, None, None, None, H, 0), ac.TrainIn(None, None, 1, 0)
                    want = _cabi.ERR_NULL if got == 1 else _cabi.ERR_LIMIT
                    assert L.ts_ac_forward(C.byref(d), None, C.byref(mlp), None, C.byref(tin), None, None, None) == want, (S, T, mc, H)
                    assert L.ts_ac_backward(C.byref(d), None, C.byref(mlp), None, C.byref(tin), None, None, None, None, None) == want, (S, T, mc, H)
                    desc = ac.TrainDesc()
                    assert L.ts_describe_ac_forward(C.byref(d), H, 1, C.byref(desc)) == (0 if got == 1 else _cabi.ERR_LIMIT)
                    assert L.ts_describe_ac_backward(C.byref(d), H, 1, C.byref(desc)) == (0 if got == 1 else _cabi.ERR_LIMIT)
    assert seen == {0, 1, _cabi.ERR_DIMS}
    for d, H in ((_dims(4, 2, 0, Tt=8), 64), (_dims(4, 2, 0, Tt=9), 64), (_dims(33, 2), 8)):
        assert L.ts_ac_supported(C.byref(d), H) == LP.ts_policy_supported(C.byref(d), H)
    assert L.ts_ac_supported(None, 8) == _cabi.ERR_NULL
    assert ac.ac_supported(_dims(8, 8), 64) and not ac.ac_supported(_dims(8, 8), 65)
    with pytest.raises(_cabi.TilerSliderLibraryError):
        ac.ac_supported(_dims(0, 1), 8)


def test_argument_validation_precedes_any_launch():
    """Every refusal below returns its own status, in the header's order: a HIP call on a box without a GPU would have answered
    TS_ERR_HIP."""
    from tiler_slider_amd import _ac_cabi as ac, _cabi, _policy_cabi as pc
    L = ac.lib()
    ok = _dims(4, 2)
    buf = (C.c_uint8 * 8192)()
    p = (C.addressof(buf) + 15) & ~15
    full = _cabi.State(p, p, p, p, p, p)
    net, head = pc.Mlp(p, p, p, p, 16, 0), ac.ValueHead(p, p)
    grad, hgrad = ac.MlpGrad(p, p, p, p), ac.ValueHeadGrad(p, p)
    tin = lambda steps=3, first=p, log=p: ac.TrainIn(first, log, steps, 0)
    ref = lambda x: C.byref(x) if x is not None else None
    fwd = lambda d, st, mlp, hd, i, z, v: L.ts_ac_forward(ref(d), ref(st), ref(mlp), ref(hd), ref(i), z, v, None)
    bwd = lambda d, st, mlp, hd, i, dz, dv, g, hg: L.ts_ac_backward(ref(d), ref(st), ref(mlp), ref(hd), ref(i), dz, dv, ref(g), ref(hg), None)
    both = lambda d, st, mlp, i, z=p, v=p, hd=head, g=grad, hg=hgrad: (fwd(d, st, mlp, hd, i, z, v), bwd(d, st, mlp, hd, i, z, v, g, hg))
    same = lambda code: (code, code)
    # 1. dims - its TS_ERR_LIMIT before the NULL checks
    assert both(None, full, net, tin()) == same(_cabi.ERR_NULL)
    assert both(_dims(0, 2), full, None, None) == same(_cabi.ERR_DIMS)
    assert both(_dims(33, 2), full, None, None) == same(_cabi.ERR_LIMIT)
    # 2. mlp / in
    assert both(ok, full, None, tin()) == same(_cabi.ERR_NULL)
    assert both(ok, full, net, None) == same(_cabi.ERR_NULL)
    assert both(_dims(9, 1), full, None, tin(0)) == same(_cabi.ERR_NULL)          # mlp is needed to know the width
    # 3. unsupported shape or width, before the steps - and before the head, which is a pointer like the others
    for S, T, H in ((9, 1, 16), (16, 2, 16), (8, 9, 16), (4, 2, 0), (4, 2, 65), (4, 2, -1)):
        assert both(_dims(S, T), full, pc.Mlp(p, p, p, p, H, 0), tin(0), hd=None) == same(_cabi.ERR_LIMIT)
    assert both(_dims(4, 2, Tt=9), full, net, tin()) == same(_cabi.ERR_LIMIT)
    # 4. steps outside 1 .. 65535, before the empty batch and before any pointer
    empty = _dims(4, 2, 0, 0)
    for steps in (0, -1, MAX_STEPS + 1, 2**31 - 1):
        assert both(ok, None, net, tin(steps), None, None, None, None, None) == same(_cabi.ERR_ARG), steps
        assert both(empty, None, net, tin(steps), None, None, None, None, None) == same(_cabi.ERR_ARG), steps
        assert L.ts_describe_ac_backward(C.byref(ok), 16, steps, C.byref(ac.TrainDesc())) == _cabi.ERR_ARG
        assert L.ts_describe_ac_forward(C.byref(ok), 16, steps, C.byref(ac.TrainDesc())) == _cabi.ERR_ARG
    assert both(ok, None, net, tin(MAX_STEPS), None, None, None, None, None) == same(_cabi.ERR_NULL)     # the edges are arguments
    assert both(ok, None, net, tin(1), None, None, None, None, None) == same(_cabi.ERR_NULL)
    # 5. nothing to do: TS_OK without a launch, no further pointer is looked at
    assert both(empty, None, pc.Mlp(None, None, None, None, 1, 0), ac.TrainIn(None, None, 1, 0), None, None, None, None, None) == same(_cabi.OK)
    # 6. missing pointers, before the alignment (p + 4: a misaligned logits pointer; p + 2: a misaligned values pointer)
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
        assert both(ok, full, mlp, tin(), p + 4, p + 2) == same(_cabi.ERR_NULL), missing
        g = ac.MlpGrad(p, p, p, p)
        setattr(g, missing, None)
        assert bwd(ok, full, net, head, tin(), p + 4, p + 2, g, hgrad) == _cabi.ERR_NULL, missing
    for missing in ("wv", "bv"):
        hd = ac.ValueHead(p, p)
        setattr(hd, missing, None)
        assert both(ok, full, net, tin(), p + 4, p + 2, hd=hd) == same(_cabi.ERR_NULL), missing
        hg = ac.ValueHeadGrad(p, p)
        setattr(hg, missing, None)
        assert bwd(ok, full, net, head, tin(), p + 4, p + 2, grad, hg) == _cabi.ERR_NULL, missing
    assert both(ok, full, net, tin(), p + 4, p + 2, hd=None) == same(_cabi.ERR_NULL)
    assert bwd(ok, full, net, head, tin(), p + 4, p + 2, None, hgrad) == _cabi.ERR_NULL
    assert bwd(ok, full, net, head, tin(), p + 4, p + 2, grad, None) == _cabi.ERR_NULL
    assert both(ok, full, net, tin(), None, p + 2) == same(_cabi.ERR_NULL)              # both outputs / cotangents are required
    assert both(ok, full, net, tin(), p + 4, None) == same(_cabi.ERR_NULL)
    # 7. alignment: 16 bytes for logits / dlogits, 4 for values / dvalues
    for off in (4, 8, 12):
        assert both(ok, full, net, tin(), p + off, p) == same(_cabi.ERR_ARG)
    for off in (1, 2, 3):
        assert both(ok, full, net, tin(), p, p + off) == same(_cabi.ERR_ARG)
    assert L.ts_ac_last_hip_error() == 0
    for fn in (L.ts_describe_ac_forward, L.ts_describe_ac_backward):
        assert fn(None, 16, 1, C.byref(ac.TrainDesc())) == _cabi.ERR_NULL and fn(C.byref(ok), 16, 1, None) == _cabi.ERR_NULL
    for describe in (ac.describe_ac_forward, ac.describe_ac_backward):
        got = describe(empty, 16, 7)
        assert (got["blocks"], got["name"], got["samples"], got["flush_bytes"]) == (0, "", 0, 0)


def _supported_shapes():
    for S in range(1, 9):
        for T in range(0, min(S * S, 8) + 1):
            yield S, T


def _head_bytes(H):
    """w2 [H][4], b2 [4], then wv [H] and bv rounded up to 16 bytes."""
    return 16 * H + 16 + ((4 * (H + 1) + 15) & ~15)


def _expected_forward(S, T, mc, H):
    """The training library's forward block with the value head's bytes behind the second layer."""
    head = _head_bytes(H)
    wt = 0 if T == 0 else (H * (T if mc else 1) * S * S * 4 + 15) & ~15
    for threads in (256, 128, 64):
        if wt and head + wt + H * 4 * threads <= LDS_LIMIT:
            return threads, head + wt + H * 4 * threads, 1
    threads = next(t for t in (256, 128, 64) if head + H * 4 * t <= LDS_LIMIT)
    return threads, head + H * 4 * threads, 0


def _expected_backward(S, T, mc, H):
    """The backward's plan restated from DESIGN.md section 18: one wave; always the second layer with the value head, the hs and
    sd columns (2 x 256 H) and the accumulators of w2, b1, b2, wv, bv (24 H + 20); then the whole w1 accumulator [H][D | 1] if it
    fits (2), else its tile planes [H][slots | 1] (1), else nothing (0); then the staged tile-plane weights if they still fit.
    Returns (lds_bytes, weights_in_lds, grads_in_lds, blocks of a large batch)."""
    C_ = S * S
    D, slots = (1 + 2 * T if mc else 3) * C_, (T if mc else 1) * C_
    fixed = _head_bytes(H) + 2 * 256 * H + (24 * H + 20)
    whole, tiles = 4 * H * (D | 1), 4 * H * (slots | 1)
    mode, acc = (2, whole) if fixed + whole <= LDS_LIMIT else (1, tiles) if T and fixed + tiles <= LDS_LIMIT else (0, 0)
    wt = 0 if T == 0 else (H * slots * 4 + 15) & ~15
    staged = int(wt > 0 and fixed + acc + wt <= LDS_LIMIT)
    lds = fixed + acc + staged * wt
    return lds, staged, mode, 256 * max(1, min(8, 160 * 1024 // lds))


def test_describe_names_exactly_the_compiled_kernels_and_no_block_asks_for_more_than_64_kib():
    from tiler_slider_amd import _ac_cabi as ac
    compiled = _kernel_names(ac.LIB_PATH)
    assert len(compiled) == ac.MIN_KERNELS == 16
    named, modes, staged = set(), set(), set()
    for S, T in _supported_shapes():
        for mc in (0, 1):
            for H in (1, 16, 64):
                wf, wb = _expected_forward(S, T, mc, H), _expected_backward(S, T, mc, H)
                for n, steps in ((1, 1), (257, 5), (1 << 20, 100)):
                    f = ac.describe_ac_forward(_dims(S, T, mc, n), H, steps)
                    assert f["name"] == f"k_ac_forward<{S}>" and f["samples"] == n * steps and f["flush_bytes"] == 20 * n * steps
                    assert (f["threads_per_block"], f["lds_bytes"], f["weights_in_lds"], f["grads_in_lds"], f["chunk_steps"]) == wf + (0, 0)
                    assert f["blocks"] == -(-n // wf[0]) and 0 < f["lds_bytes"] <= LDS_LIMIT
                    b = ac.describe_ac_backward(_dims(S, T, mc, n), H, steps)
                    assert b["name"] == f"k_ac_backward<{S}>" and b["samples"] == n * steps and b["threads_per_block"] == 64
                    assert (b["lds_bytes"], b["weights_in_lds"], b["grads_in_lds"]) == wb[:3], (S, T, mc, H, b)
                    assert b["blocks"] == min(-(-n // 64), wb[3]) and 0 < b["lds_bytes"] <= LDS_LIMIT and b["chunk_steps"] == 4
                    acc = {2: (1 + 2 * T if mc else 3) * S * S, 1: (T if mc else 1) * S * S, 0: 0}[wb[2]]   # w1 rows accumulated in LDS
                    assert b["flush_bytes"] == b["blocks"] * 4 * (6 * H + 5 + acc * H)
                    named.update((f["name"], b["name"]))
                modes.add(wb[2])
                staged.add(wb[1])
    assert sorted(named) == compiled and modes == {0, 1, 2} and staged == {0, 1}
    import ac_reference as ar
    assert sorted(ar.OCCUPANCY_CASES) == compiled      # tests/test_gpu_ac.py runs one case per kernel at 4,096 waves


# (S, T, multi colour) -> the widths H at which grads_in_lds is another value than at H - 1, with that value
BOUNDARIES = {(4, 2, 0): {}, (5, 3, 1): {53: 1}, (8, 8, 1): {14: 1, 26: 0}}


def test_where_the_gradients_live_on_both_sides_of_each_boundary():
    """The describe call is walked over every width 1 .. 64 of 4x4 / 2 single colour, 5x5 / 3 multi colour and 8x8 / 8 multi
    colour: the boundaries it reports are the literal ones above - cfg1's shape keeps the whole gradient at every width, 5x5 / 3
    up to 52 units, 8x8 / 8 up to 13 units and its tile planes up to 25 -, and on both sides of each the whole answer (LDS bytes,
    staged weights, mode, grid) is the restated plan's."""
    from tiler_slider_amd import _ac_cabi as ac
    pick = lambda d: (d["lds_bytes"], d["weights_in_lds"], d["grads_in_lds"], d["blocks"])
    for (S, T, mc), want in BOUNDARIES.items():
        at = lambda H: ac.describe_ac_backward(_dims(S, T, mc, 1 << 16), H, 16)
        modes = {H: at(H)["grads_in_lds"] for H in range(1, 65)}
        assert modes[1] == 2
        reported = {H: modes[H] for H in range(2, 65) if modes[H] != modes[H - 1]}
        assert reported == want, (S, T, mc, reported)
        for H in reported:
            for side in (H - 1, H):
                want_side = _expected_backward(S, T, mc, side)
                assert pick(at(side)) == want_side[:3] + (min(1 << 10, want_side[3]),), (S, T, mc, side)
                assert at(side)["lds_bytes"] <= LDS_LIMIT
    # literal bytes on both sides of 8x8 / 8's boundaries: a unit costs 16 + 512 + 24 bytes of fixed LDS beside the value head's
    # rounded 4 (H + 1), 4,356 of a whole w1 accumulator (row stride 1,089), 2,052 of a tile-plane one (513)
    at = lambda H: ac.describe_ac_backward(_dims(8, 8, 1, 1 << 16), H, 16)
    fixed = lambda H: 36 + 552 * H + ((4 * (H + 1) + 15) & ~15)
    assert (at(13)["grads_in_lds"], at(13)["weights_in_lds"], at(13)["lds_bytes"]) == (2, 0, fixed(13) + 13 * 4356)
    assert (at(14)["grads_in_lds"], at(14)["weights_in_lds"], at(14)["lds_bytes"]) == (1, 1, fixed(14) + 14 * (2052 + 2048))
    assert (at(25)["grads_in_lds"], at(25)["weights_in_lds"], at(25)["lds_bytes"]) == (1, 0, fixed(25) + 25 * 2052)
    assert (at(26)["grads_in_lds"], at(26)["weights_in_lds"], at(26)["lds_bytes"]) == (0, 0, fixed(26))
    assert at(14)["lds_bytes"] == 65228
    # 5x5 / 3 multi colour at 64 units: the tile planes only, and no room left for the staged weights
    d = ac.describe_ac_backward(_dims(5, 3, 1, 1 << 16), 64, 16)
    assert (d["grads_in_lds"], d["weights_in_lds"]) == (1, 0)


def test_every_ac_kernel_keeps_its_board_in_registers_and_its_lds_dynamic():
    """The code object's own metadata and instructions: no private segment (scratch), no scratch_ instruction, no static LDS
    (every byte of LDS is the dynamic allocation ts_describe_ac_* reports), no accumulation registers (the hazard scan skips
    kernels that use them), and the float adds are single instructions: ds_add_f32 and global_atomic_add_f32 in every backward
    kernel, no compare-and-swap loop anywhere."""
    from tiler_slider_amd import _ac_cabi as ac
    kernels = _kernel_metadata(ac.LIB_PATH)
    assert len(kernels) == len([k for k in kernels if "k_ac_" in k["name"]]) == ac.MIN_KERNELS
    assert not any(k["group_segment_fixed_size"] or k["private_segment_fixed_size"] or k["agpr_count"] or k["uses_dynamic_stack"] for k in kernels), kernels
    pats = (r"\bscratch_\w+", r"\bs_barrier\b", r"\bds_(read|write|load|store)\w*", r"\bds_add_f32\b", r"\bglobal_atomic_add_f32\b", r"cmpswap")
    mine = {k: v for k, v in _instruction_counts(ac.LIB_PATH, pats).items() if "k_ac_" in k}
    assert len(mine) == ac.MIN_KERNELS
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
    return b.encode_onehot().reshape(n, -1)


def test_the_closed_form_is_float64_autograd_of_the_dense_five_output_network(oracle):
    """grads64 (train_reference's closed form on the stacked network, split again) against torch autograd written here on SIX
    separate tensors - the head is not stacked on this side -, and the value path is seen to reach the trunk: w1's gradient with
    dv dropped is another one, and the gradients of w2 and b2 do not see dv at all."""
    import torch
    import ac_reference as ar
    import train_reference as tr
    x = _random_samples(oracle, 5, 3, True, 300, 0x7A6)
    rng = np.random.default_rng(3)
    mlp, head = tr.pref.random_mlp(rng, x.shape[1], 7), ar.random_head(rng, 7)
    dz, dv = rng.standard_normal((300, 4)), rng.standard_normal(300)
    mine = ar.grads64(x, mlp, head, dz, dv)
    stacked = ar.torch_grads64(x, mlp, head, dz, dv)
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    w1, b1, w2, b2, wv, bv = (t(a) for a in mlp + head)
    h = torch.relu(torch.tensor(np.asarray(x, np.float64)) @ w1.T + b1)
    z, v = h @ w2.T + b2, h @ wv + bv
    torch.autograd.backward((z, v), (torch.tensor(dz), torch.tensor(dv)))
    theirs = {"w1": w1.grad.T.numpy(), "b1": b1.grad.numpy(), "w2": w2.grad.T.numpy(), "b2": b2.grad.numpy(), "wv": wv.grad.numpy(), "bv": bv.grad.numpy()}
    assert mine["wv"].shape == (7,) and mine["bv"].shape == (1,) and mine["w2"].shape == (7, 4) and mine["b2"].shape == (4,)
    for name in ar.NAMES:
        for other in (theirs, stacked):
            assert mine[name].shape == other[name].shape, name
            assert np.abs(mine[name] - other[name]).max() <= 1e-11 * max(1.0, np.abs(other[name]).max()), name
    z64, _, v64, _ = ar.outputs64(x, mlp, head)
    assert np.abs(z64 - z.detach().numpy()).max() <= 1e-12 and np.abs(v64 - v.detach().numpy()).max() <= 1e-12
    without = ar.grads64(x, mlp, head, dz, np.zeros(300))
    assert (without["w1"] != mine["w1"]).any() and (without["b1"] != mine["b1"]).any()
    assert (without["w2"] == mine["w2"]).all() and (without["b2"] == mine["b2"]).all()
    assert not without["wv"].any() and not without["bv"].any() and mine["wv"].any()
    actor_only = tr.grads64(x, mlp, dz)                  # with dv = 0 the first four are the training library's definition
    for name in ("w1", "b1", "w2", "b2"):
        assert np.abs(without[name] - actor_only[name]).max() <= 1e-12 * max(1.0, np.abs(actor_only[name]).max()), name


def _float32_gradients(x, mlp, head, dz, dv, rng):
    """Three float32 evaluations of the six gradients: features / outputs / samples first to last, last to first, and shuffled
    with pairwise sums over the samples."""
    import ac_reference as ar
    w1, b1, w2, b2 = ar.stack(mlp, head)
    d5 = ar.stack_cotangents(dz, dv).astype(np.float32)
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
        acts = {"forward": (0, 1, 2, 3, 4), "backward": (4, 3, 2, 1, 0), "shuffled": tuple(rng.permutation(5))}[order]
        dh = np.zeros((n, H), f32)
        for a in acts:
            dh = (dh + (d5[:, a:a + 1] * w2[None, a, :]).astype(f32)).astype(f32)
        dp = np.where(pre > 0, dh, f32(0)).astype(f32)
        rows = {"forward": np.arange(n), "backward": np.arange(n)[::-1], "shuffled": rng.permutation(n)}[order]

        def total(terms):   # [m, ...] float32 -> the sum over axis 0 in this order's way
            terms = np.ascontiguousarray(terms, dtype=f32)
            if terms.shape[0] == 0:
                return np.zeros(terms.shape[1:], f32)
            return terms.sum(axis=0, dtype=f32) if order == "shuffled" else np.cumsum(terms, axis=0, dtype=f32)[-1]

        g = {"b2": total(d5[rows]), "b1": total(dp[rows]),
             "w2": np.stack([total((h[rows] * d5[rows, a:a + 1]).astype(f32)) for a in range(5)], axis=1),
             "w1": np.stack([total(dp[rows][x[rows, f] > 0]) for f in range(D)], axis=0)}
        outs.append(ar.split(g))
    return outs


@pytest.mark.parametrize("S,T,mc,H", ((4, 2, False, 64), (5, 3, True, 16)))
def test_the_gradient_bound_holds_float32_evaluations_in_three_orders_and_is_not_vacuous(oracle, S, T, mc, H):
    """10,000 random boards, Gaussian weights, dz and dv: every float32 entry of the six gradients lies within its bound of the
    float64 one, the orders do differ, and the bound means something: its median over all entries is below 1 % of the median |g|."""
    import ac_reference as ar
    import train_reference as tr
    n = 10000
    rng = np.random.default_rng(S * 100 + H + 1)
    x = _random_samples(oracle, S, T, mc, n, 0xB0D + S)
    mlp, head = tr.pref.random_mlp(rng, x.shape[1], H), ar.random_head(rng, H)
    dz, dv = rng.standard_normal((n, 4)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    want = ar.grads64(x, mlp, head, dz, dv)
    bounds, ambiguous = ar.grad_bounds(x, mlp, head, dz, dv)
    outs = _float32_gradients(x, mlp, head, dz, dv, rng)
    worst = 0.0
    for got in outs:
        for name in ar.NAMES:
            assert got[name].dtype == np.float32 and got[name].shape == want[name].shape == bounds[name].shape
            err = np.abs(got[name].astype(np.float64) - want[name])
            assert (err <= bounds[name]).all(), (name, float((err / np.maximum(bounds[name], 1e-300)).max()))
            worst = max(worst, float((err / np.maximum(bounds[name], 1e-300)).max()))
    assert any((outs[0][k] != o[k]).any() for o in outs[1:] for k in ar.NAMES)
    every = lambda d: np.concatenate([np.asarray(d[k], np.float64).ravel() for k in ar.NAMES])
    ratio = float(np.median(every(bounds)) / np.median(np.abs(every(want))))
    print(f"{S}x{S}/{T} H={H}: worst float32 error / bound {worst:.3f}, median bound / median |g| {ratio:.2e}, "
          f"ambiguous pairs {ambiguous.mean():.2e}")
    assert worst > 1e-4 and ratio < 0.01
    assert ambiguous.mean() <= 1e-4
    # the value's own bound: float32 values in two orders of the hidden units
    _, _, v64, vb = ar.outputs64(x, mlp, head)
    w1, b1 = mlp[0], mlp[1]
    h = np.maximum((x.astype(np.float32) @ w1.T + b1).astype(np.float32), np.float32(0))
    for order in (np.arange(H), np.arange(H)[::-1]):
        v = np.full(n, head[1][0], np.float32)
        for j in order:
            v = (v + h[:, j] * head[0][j]).astype(np.float32)
        assert (np.abs(v.astype(np.float64) - v64) <= vb).all()
    assert np.median(vb) < 0.01 * np.median(np.abs(v64))


def test_the_exact_cases_bite_on_the_yardsticks_own_numbers(oracle):
    """One exact case per kind on the CPU: ac_reference.backward_case's own assertions (a non-zero wv gradient, a kink of the ReLU
    with a non-zero five-term dh, a shared cell) hold, exactness_guard refuses inputs whose fifth column is not exact, and a
    gradient computed with relu'(0) = 1 differs."""
    import ac_reference as ar
    for case, H, K in ((0, 7, 5), (1, 64, 2), (2, 20, 1)):
        c = ar.backward_case(oracle, case, H, K)
        assert c["wv_grad"] and c["reaches"] and c["bites"] >= 0.01
        n = c["first"].shape[1]
        flat, dv = c["dz"].reshape(K * n, 4), c["dv"].reshape(-1)
        assert set(np.unique(dv)) <= {-1.0, 0.0, 1.0} and c["values"].shape == (K, n)
        wrong = ar.grads64(c["x"], c["mlp"], c["head"], flat, dv, relu_at_zero=1.0)
        plain = ar.grads64(c["x"], c["mlp"], c["head"], flat, dv)
        assert (wrong["w1"] != plain["w1"]).any()
        with pytest.raises(AssertionError):
            ar.exactness_guard(c["x"], c["mlp"], (c["head"][0] + np.float32(0.5), c["head"][1]), flat, dv)
        with pytest.raises(AssertionError):
            ar.exactness_guard(c["x"], c["mlp"], c["head"], flat, dv * np.float32(2.0 ** 24))
