"""The fused optimiser without a GPU: the optim library's C-ABI (include/tiler_slider_optim.h), its refusals in the header's
order, its launch plan on both sides of the one-block constant, its code object, and the CPU yardstick's own checks
(tests/optim_reference.py): float64 torch AdamW + clip_grad_norm_ over 20 steps, and the one-step bounds on float32 NumPy and
float32 torch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import optim_reference as ref
from cabi_harness import _kernel_metadata, _kernel_names, _struct_fields
from conftest import ROOT
from tiler_slider_amd import _optim_cabi as oc

NAN = float("nan")


@pytest.fixture
def knob():
    """ts_optim_tuning(TS_OPTIM_TUNE_ONE_BLOCK_MAX) as it was, after the test."""
    was = oc.tuning(oc.TUNE_ONE_BLOCK_MAX)
    yield lambda value: oc.tuning(oc.TUNE_ONE_BLOCK_MAX, value)
    oc.tuning(oc.TUNE_ONE_BLOCK_MAX, was)


def test_optim_library_exports_what_its_header_declares():
    header = open(os.path.join(ROOT, "include", "tiler_slider_optim.h")).read()
    assert '#include "tiler_slider.h"' in header and "ts_dims" not in re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for phrase in ("NOT BUILT: amsgrad; L2 (coupled) decay; several parameter groups; bf16", "NO FLOAT ATOMICS ANYWHERE", "ACCUMULATED IN FLOAT64",
                   "reproducible bit for bit", "NOT\n *     PART OF THE CONTRACT", "clip_grad_norm_'s rule"):
        assert phrase in header, phrase
    for struct, cls in (("ts_optim_tensors", oc.OptimTensors), ("ts_adam_cfg", oc.AdamCfg), ("ts_optim_out", oc.OptimOut), ("ts_optim_desc", oc.OptimDesc)):
        fields = _struct_fields(header, struct)
        assert fields == [f for f, _ in cls._fields_], struct
    assert (C.sizeof(oc.OptimTensors), C.sizeof(oc.AdamCfg), C.sizeof(oc.OptimOut), C.sizeof(oc.OptimDesc)) == (8 + 5 * 256, 48, 24, 160)
    assert [(f, getattr(oc.AdamCfg, f).offset) for f, _ in oc.AdamCfg._fields_] == [
        ("beta1", 0), ("beta2", 8), ("lr_dev", 16), ("lr", 24), ("eps", 28), ("weight_decay", 32), ("max_grad_norm", 36), ("skip_nonfinite", 40),
        ("zero_grad", 44)]
    assert [(f, getattr(oc.OptimTensors, f).offset) for f, _ in oc.OptimTensors._fields_] == [
        ("n_tensors", 0), ("reserved", 4), ("numel", 8), ("param", 264), ("grad", 520), ("m", 776), ("v", 1032)]
    assert dict(oc.AdamCfg._fields_)["beta1"] is C.c_double and dict(oc.AdamCfg._fields_)["beta2"] is C.c_double
    for name, value in re.findall(r"#define TS_OPTIM_([A-Z_]+) (0x[0-9a-f]+|\d+)u?", header):
        if name != "ABI_VERSION":
            assert getattr(oc, name) == int(value, 0), name
    import tiler_slider_amd as pkg
    assert callable(pkg.build_optim_library) and issubclass(pkg.FusedAdam, __import__("torch").optim.Optimizer)
    assert {"FusedAdam", "build_optim_library"} <= set(pkg.__all__)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ts_optim.hip" in design and "amsgrad" in design and "optimisers (torch's are used)" not in design


def test_every_refusal_has_its_own_status_in_the_headers_order(knob):
    """No HIP call is made before a refusal: on a box without a GPU one would have answered TS_ERR_HIP."""
    from tiler_slider_amd import _cabi
    L = oc.lib()
    N = 100
    buf = (C.c_uint8 * (1 << 20))()
    base = (C.addressof(buf) + 255) & ~255
    at = lambda k: base + k * 4096         # regions apart: 100 elements are 400 bytes
    ref_ = lambda x: C.byref(x) if x is not None else None

    def tensors(n=3, numel=(N, 0, 7), **kw):
        t = oc.OptimTensors(n_tensors=n)
        for i in range(min(n, 32) if n > 0 else 0):
            t.numel[i] = numel[i % len(numel)]
            t.param[i], t.grad[i], t.m[i], t.v[i] = at(4 * i), at(4 * i + 1), at(4 * i + 2), at(4 * i + 3)
        for name, (i, value) in kw.items():
            getattr(t, name)[i] = value
        return t

    def cfg(**kw):
        a = dict(beta1=0.9, beta2=0.999, lr_dev=None, lr=1e-3, eps=1e-8, weight_decay=0.01, max_grad_norm=1.0, skip_nonfinite=1, zero_grad=1)
        a.update(kw)
        return oc.AdamCfg(**a)

    def out(**kw):
        a = dict(counters=at(200), grad_norm=at(201), workspace=at(202))
        a.update(kw)
        return oc.OptimOut(**a)

    call = lambda t, c, o: L.ts_adam_step(ref_(t), ref_(c), ref_(o), None)
    NULL, ARG, OK = _cabi.ERR_NULL, _cabi.ERR_ARG, _cabi.OK
    nothing = oc.OptimOut()
    knob(0)     # the multi-block form: the one that needs a workspace
    # 1. the struct pointers
    assert call(None, cfg(), out()) == NULL and call(tensors(), None, out()) == NULL and call(tensors(), cfg(), None) == NULL
    # 2. the count and the sizes: before the hyperparameters (lr is bad throughout) and before any pointer
    for t in (tensors(n=-1), tensors(n=33), tensors(numel=(N, -1, 7))):
        assert call(t, cfg(lr=-1.0), nothing) == ARG
    # 3. the hyperparameters: before the empty call and before any pointer (every pointer of `nothing` is NULL)
    bad = (dict(lr=-1e-3), dict(lr=NAN), dict(eps=-1e-8), dict(eps=NAN), dict(weight_decay=-0.1), dict(weight_decay=NAN), dict(beta1=-0.1),
           dict(beta1=1.0), dict(beta1=NAN), dict(beta2=-0.1), dict(beta2=1.0), dict(beta2=NAN), dict(max_grad_norm=-1.0), dict(max_grad_norm=NAN))
    for kw in bad:
        assert call(tensors(), cfg(**kw), nothing) == ARG, kw
        assert call(tensors(n=0), cfg(**kw), nothing) == ARG, kw
    assert call(tensors(), cfg(beta1=0.0, beta2=0.0, lr=0.0, eps=0.0, weight_decay=0.0, max_grad_norm=0.0), nothing) == NULL     # all fine: on to the pointers
    # 4. nothing to do: TS_OK without a launch, no pointer is looked at (grad_norm NULL: nothing to zero)
    assert call(tensors(n=0), cfg(), nothing) == OK and call(tensors(numel=(0,)), cfg(), nothing) == OK
    assert call(tensors(numel=(0,), param=(0, None)), cfg(lr_dev=at(210) + 1), oc.OptimOut(counters=at(200) + 1)) == OK
    # 5. missing pointers, before the alignment (lr_dev is misaligned throughout)
    odd = dict(lr_dev=at(210) + 2)
    for name in ("param", "grad", "m", "v"):
        assert call(tensors(**{name: (0, None)}), cfg(**odd), out()) == NULL, name
        assert call(tensors(**{name: (1, None)}), cfg(**odd), out()) == ARG, name      # tensor 1 is empty: not looked at, on to the alignment
    assert call(tensors(), cfg(**odd), out(counters=None)) == NULL and call(tensors(), cfg(**odd), out(workspace=None)) == NULL
    assert call(tensors(), cfg(**odd), out(grad_norm=None)) == ARG                      # grad_norm may be missing
    knob(1 << 20)                                                                       # the one-block form needs no workspace
    assert call(tensors(), cfg(**odd), out(workspace=None)) == ARG
    knob(0)
    assert call(tensors(), cfg(max_grad_norm=0.0, skip_nonfinite=0, **odd), out(workspace=None, grad_norm=None)) == ARG      # nor does the apply-alone form
    # 6. alignment
    for name in ("param", "grad", "m", "v"):
        for off in (1, 2, 3):
            assert call(tensors(**{name: (2, getattr(tensors(), name)[2] + off)}), cfg(), out()) == ARG, (name, off)
    for off in (1, 2, 3):
        assert call(tensors(), cfg(), out(grad_norm=at(201) + off)) == ARG and call(tensors(), cfg(lr_dev=at(210) + off), out()) == ARG
    for off in (1, 2, 4):
        assert call(tensors(), cfg(), out(counters=at(200) + off)) == ARG and call(tensors(), cfg(), out(workspace=at(202) + off)) == ARG
    # 7. a written range that overlaps another range - by its last byte too
    ws = oc.describe_adam_step([N, 0, 7], oc.NORM)["workspace_bytes"]
    assert ws == 16       # two chunks, two blocks, two partials
    assert call(tensors(m=(0, at(0))), cfg(), out()) == ARG and call(tensors(m=(0, at(0) + 4 * (N - 1))), cfg(), out()) == ARG
    assert call(tensors(v=(2, at(0) + 4 * (N - 1))), cfg(), out()) == ARG              # v of tensor 2: its first float is param 0's last
    assert call(tensors(param=(2, at(1))), cfg(zero_grad=0), out()) == ARG              # a written range over a read one
    assert call(tensors(grad=(2, at(1))), cfg(zero_grad=1), out()) == ARG               # two gradients, once they are written
    assert call(tensors(), cfg(), out(counters=at(0) + 4 * N - 8)) == ARG and call(tensors(), cfg(), out(counters=at(201) - 8)) == ARG
    assert call(tensors(), cfg(), out(grad_norm=at(200) + 12)) == ARG and call(tensors(), cfg(lr_dev=at(3) + 4 * (N - 1)), out()) == ARG
    assert call(tensors(), cfg(), out(workspace=at(3) - ws + 8)) == ARG
    # ... and everything right reaches the launch, which a box without a GPU refuses; one with a GPU is not asked here
    assert L.ts_optim_last_hip_error() == 0
    assert L.ts_optim_workspace_bytes(-1) == ARG and L.ts_optim_workspace_bytes(0) == 0
    with pytest.raises(_cabi.TilerSliderLibraryError):
        oc.workspace_bytes(-5)
    desc = oc.OptimDesc()
    one = (C.c_int64 * 1)(5)
    assert L.ts_describe_adam_step(1, one, 0, None) == NULL and L.ts_describe_adam_step(1, None, 0, C.byref(desc)) == NULL
    assert L.ts_describe_adam_step(33, one, 0, C.byref(desc)) == ARG and L.ts_describe_adam_step(1, one, 4, C.byref(desc)) == ARG
    assert L.ts_describe_adam_step(1, (C.c_int64 * 1)(-5), 0, C.byref(desc)) == ARG
    assert L.ts_optim_tuning(7, 1) == -1


def test_workspace_bytes_is_the_bounded_grids():
    assert [oc.workspace_bytes(n) for n in (0, 1, 1 << 20, 1 << 40)] == [0, 8192, 8192, 8192]
    assert oc.workspace_bytes(1) == 8 * oc.MAX_BLOCKS
    big = oc.describe_adam_step([1 << 30] * 32)
    assert big["workspace_bytes"] == oc.workspace_bytes(1 << 35) and big["blocks"] == oc.MAX_BLOCKS


AC_4x4 = (80 * 32, 32, 32 * 4, 4, 32, 1)


@pytest.mark.parametrize("numels", (AC_4x4, (1,), (1023, 1, 1025), (4096, 4097), (0, 5, 0), (oc.MAX_BLOCKS * oc.CHUNK + 259, 5)))
def test_describe_names_the_form_and_the_launches_on_both_sides_of_the_constant(knob, numels):
    total = sum(numels)
    default = oc.tuning(oc.TUNE_ONE_BLOCK_MAX)
    assert default > sum(AC_4x4)        # the project's own case takes one launch
    for what in range(4):
        norm, zero = what & oc.NORM, what & oc.ZERO_GRAD
        read, written = total * (16 + (4 if norm else 0)), total * (12 + (4 if zero else 0)) + 16 + (4 if norm else 0)
        knob(total)                     # the constant is inclusive
        d = oc.describe_adam_step(numels, what)
        chunks = sum(-(-n // oc.ONE_CHUNK) for n in numels)
        assert (d["form"], d["launches"], d["threads_per_block"], d["blocks"], d["chunks"], d["workspace_bytes"]) == (oc.FORM_ONE, 1, 1024, 1, chunks, 0)
        assert (d["name"], d["norm_name"], d["finish_name"]) == ("k_optim_one", "", "")
        assert (d["total_numel"], d["bytes_read"], d["bytes_written"], d["lds_bytes"]) == (total, read, written, 152)
        knob(total - 1)
        d = oc.describe_adam_step(numels, what)
        chunks = sum(-(-n // 1024) for n in numels)
        blocks = min(chunks, 1024)
        if norm:
            assert (d["form"], d["launches"], d["workspace_bytes"]) == (oc.FORM_MULTI, 3, 8 * blocks)
            assert (d["name"], d["norm_name"], d["finish_name"]) == ("k_optim_apply", "k_optim_norm", "k_optim_finish")
        else:
            assert (d["form"], d["launches"], d["workspace_bytes"]) == (oc.FORM_APPLY, 2, 0)
            assert (d["name"], d["norm_name"], d["finish_name"]) == ("k_optim_apply", "", "k_optim_finish")
        assert (d["threads_per_block"], d["blocks"], d["chunks"], d["lds_bytes"]) == (256, blocks, chunks, 56)
        assert (d["total_numel"], d["bytes_read"], d["bytes_written"]) == (total, read, written)
    knob(default)
    nothing = oc.describe_adam_step((0, 0), 3)
    assert (nothing["form"], nothing["launches"], nothing["blocks"], nothing["name"], nothing["bytes_written"]) == (oc.FORM_NONE, 0, 0, "", 0)
    assert oc.describe_adam_step((), 3)["form"] == oc.FORM_NONE


def test_describe_names_exactly_the_compiled_kernels(knob):
    compiled = _kernel_names(oc.LIB_PATH)
    knob(0)
    d = oc.describe_adam_step([1000], oc.NORM)
    knob(1000)
    one = oc.describe_adam_step([1000], oc.NORM)
    assert len(compiled) == oc.MIN_KERNELS == 4
    assert sorted((one["name"], d["name"], d["norm_name"], d["finish_name"])) == sorted(compiled)


def test_the_optim_kernels_use_no_scratch_no_agprs_and_the_lds_they_report(knob):
    kernels = _kernel_metadata(oc.LIB_PATH)
    assert len(kernels) == len([k for k in kernels if "k_optim_" in k["name"]]) == oc.MIN_KERNELS
    assert not any(k["private_segment_fixed_size"] or k["agpr_count"] or k["uses_dynamic_stack"] for k in kernels), kernels
    by_name = {re.search(r"k_optim_[a-z]+", k["name"]).group(0): k["group_segment_fixed_size"] for k in kernels}
    knob(0)
    assert by_name["k_optim_apply"] == oc.describe_adam_step([5])["lds_bytes"]
    knob(5)
    assert by_name["k_optim_one"] == oc.describe_adam_step([5])["lds_bytes"]
    assert by_name["k_optim_norm"] <= by_name["k_optim_apply"] and by_name["k_optim_finish"] <= by_name["k_optim_apply"]


def test_the_build_goes_through_the_guard_its_scan_is_clean_and_it_touches_nothing_else(tmp_path):
    """The library compiled once more, into a directory of its own (a few seconds): the other libraries and every source are
    what they were, byte for byte."""
    import hashlib
    from tiler_slider_amd import _cabi
    from tiler_slider_amd._libraries import LIBRARIES
    others = [b for b in LIBRARIES if b is not oc]
    watched = [b.LIB_PATH for b in others] + [b.SRC for b in others] + sorted({h for b in others for h in b.HEADERS})
    digest = lambda: [hashlib.sha256(open(p, "rb").read()).hexdigest() for p in watched]
    before = digest()
    report = _cabi.compile_guarded(oc.SRC, str(tmp_path / "libtiler_slider_optim.so"), work=str(tmp_path), min_kernels=oc.MIN_KERNELS)
    assert report["kernels"] == 4 and report["hits_in_final_object"] == {"class_a": 0, "class_b": 0} and report["kernels_with_agprs"] == []
    assert open(tmp_path / "libtiler_slider_optim.so", "rb").read(4) == b"\x7fELF"
    assert digest() == before


# ---------------------------------------------------------------------------------------------- the yardstick itself
SHAPES = ((80, 32), (32,), (32, 4), (4,), (32,), (1,))


def test_the_yardstick_is_float64_torch_adamw_behind_clip_grad_norm_over_twenty_steps():
    """Gradients alternate between a scale that clips (3.0: the norm is near 160) and one that does not (0.001)."""
    import torch
    rng = np.random.default_rng(5)
    cfg = dict(lr=f32(1e-2), beta1=0.9, beta2=0.999, eps=f32(1e-8), weight_decay=f32(0.01), max_grad_norm=0.5)
    p = [rng.standard_normal(s) for s in SHAPES]
    tp = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in p]
    opt = torch.optim.AdamW(tp, lr=cfg["lr"], betas=(0.9, 0.999), eps=cfg["eps"], weight_decay=cfg["weight_decay"])
    m, v = [np.zeros(s) for s in SHAPES], [np.zeros(s) for s in SHAPES]
    clipped = []
    for t in range(20):
        g = [rng.standard_normal(s) * (3.0 if t % 2 == 0 else 0.001) for s in SHAPES]
        for q, a in zip(tp, g):
            q.grad = torch.tensor(a, dtype=torch.float64)
        gn = float(torch.nn.utils.clip_grad_norm_(tp, cfg["max_grad_norm"]))
        opt.step()
        st = ref.adam64(p, g, m, v, t, **cfg)
        assert abs(st.gn - gn) <= 1e-12 * gn and st.t == t + 1 and not st.skipped
        clipped.append(st.c < 1.0)
        p, m, v = st.p, st.m, st.v
        for q, a, mm, vv in zip(tp, p, m, v):
            assert np.abs(q.detach().numpy() - a).max() <= 1e-12
            assert np.abs(opt.state[q]["exp_avg"].numpy() - mm).max() <= 1e-12 and np.abs(opt.state[q]["exp_avg_sq"].numpy() - vv).max() <= 1e-12
    assert clipped == [True, False] * 10


def f32(x):
    return float(np.float32(x))


def test_the_one_step_bounds_hold_float32_numpy_and_float32_torch_and_notice_a_wrong_step():
    """200 random cases at t in {0, 1, 1000}, clip on and off, decay on and off: the worst float32 deviation, in units of
    2^-24 M, is printed and lies below 16 - and above 0.5, so that the bound is a few roundings and not a tolerance anything
    passes; a step with the betas swapped, with the bias correction of another t, or without the clip leaves it by far."""
    import torch
    shapes = (37, 5, 1)
    worst = dict(p=0.0, m=0.0, v=0.0, torch=0.0)
    for case in range(200):
        t = (0, 1, 1000)[case % 3]
        cfg = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01 * (case % 2), max_grad_norm=(0.0, 0.5, 1e6)[case % 5 % 3])
        g = ref.gradients(shapes, case)
        p, m, v = ref.state(shapes, case, t)
        want = ref.adam64(p, g, m, v, t, **cfg)
        P, M, V = ref.adam32(p, g, m, v, t, **cfg)
        assert ref.within(P, want.p, want.Mp) and ref.within(M, want.m, want.Mm) and ref.within(V, want.v, want.Mv)
        worst["p"], worst["m"], worst["v"] = max(worst["p"], ref.worst(P, want.p, want.Mp)), max(worst["m"], ref.worst(M, want.m, want.Mm)), max(worst["v"], ref.worst(V, want.v, want.Mv))
        if t == 0:      # torch's own step count starts at 0: only there is its bias correction this one
            tp = [torch.tensor(a, requires_grad=True) for a in p]
            for q, a in zip(tp, g):
                q.grad = torch.tensor(a)
            if cfg["max_grad_norm"]:
                torch.nn.utils.clip_grad_norm_(tp, cfg["max_grad_norm"])
            torch.optim.AdamW(tp, lr=cfg["lr"], weight_decay=cfg["weight_decay"]).step()
            got = [q.detach().numpy() for q in tp]
            assert ref.within(got, want.p, want.Mp)
            worst["torch"] = max(worst["torch"], ref.worst(got, want.p, want.Mp))
        if case < 12:
            wrong = [ref.adam64(p, g, m, v, t, **dict(cfg, beta1=cfg["beta2"], beta2=cfg["beta1"]))]      # the betas swapped
            if t <= 1:
                wrong.append(ref.adam64(p, g, m, v, t + 1, **cfg))                                        # the bias correction of the wrong t
            if want.c < 1.0:
                wrong.append(ref.adam64(p, g, m, v, t, **dict(cfg, max_grad_norm=0.0)))                   # the clip left out
            for bad in wrong:
                assert max(ref.worst(bad.p, want.p, want.Mp), ref.worst(bad.m, want.m, want.Mm), ref.worst(bad.v, want.v, want.Mv)) > 1000, case
    print("worst float32 deviation in units of 2^-24 M:", {k: round(x, 2) for k, x in worst.items()})
    assert all(0.5 < x < 16 for x in worst.values()), worst


def test_the_exact_case_is_exact_in_float64_and_float32():
    for one in (False, True):
        cfg, p, g, want_p, want_m, want_v = ref.exact_case(one)
        z = [np.zeros_like(a) for a in p]
        st = ref.adam64(p, g, z, z, 0, **cfg)
        P, M, V = ref.adam32(p, g, z, z, 0, **cfg)
        for i in range(2):
            for got64, got32, want in ((st.p, P, want_p), (st.m, M, want_m), (st.v, V, want_v)):
                assert want[i].dtype == np.float32
                np.testing.assert_array_equal(got64[i], want[i].astype(np.float64))
                np.testing.assert_array_equal(got32[i], want[i])
        assert sum(a.size for a in p) == 1024 and st.t == 1 and (st.gn == 32.0 if one else st.gn > 0)
        assert all(np.abs(a - b).max() == 2.0 ** -4 for a, b in zip(want_p, p))
