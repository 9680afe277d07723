"""The fused actor-critic loss without a GPU: the loss library's C-ABI (include/tiler_slider_loss.h), its launch plan, its code
object and kept assembly, and the CPU yardstick's own checks (tests/loss_reference.py): its gradients against float64 torch
autograd of the plain-torch loss, and its bound against float32 NumPy in two evaluation orders."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cabi_harness import _kernel_metadata, _kernel_names, _struct_fields
from conftest import ROOT
from tiler_slider_amd import _loss_cabi as lc

NAN = float("nan")
BLOCK, GRID = lc.THREADS, lc.THREADS * lc.MAX_BLOCKS


def test_loss_library_exports_what_its_header_declares():
    header = open(os.path.join(ROOT, "include", "tiler_slider_loss.h")).read()
    assert '#include "tiler_slider.h"' in header and "ts_dims" not in re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for phrase in ("NOT BUILT: value clipping; an epsilon-mixed behaviour policy in the ratio; per-sample weights; bf16", "NO FLOAT ATOMICS ANYWHERE",
                   "reproducible bit for bit", "NOT PART\n * OF THE CONTRACT", "EXACTLY 0 on a sample that is not live"):
        assert phrase in header, phrase
    for struct, cls in (("ts_loss_in", lc.LossIn), ("ts_loss_out", lc.LossOut), ("ts_loss_desc", lc.LossDesc)):
        fields = _struct_fields(header, struct)
        assert fields == [f for f, _ in cls._fields_], struct
    assert (C.sizeof(lc.LossIn), C.sizeof(lc.LossOut), C.sizeof(lc.LossDesc)) == (80, 32, 192)
    # both structs field by field: offsets and types as the header lays them out
    assert [(f, getattr(lc.LossIn, f).offset) for f, _ in lc.LossIn._fields_] == [
        ("logits", 0), ("old_logits", 8), ("act", 16), ("mask", 24), ("adv", 32), ("values", 40), ("ret", 48), ("n_samples", 56), ("clip", 64),
        ("value_coef", 68), ("entropy_coef", 72), ("normalize_adv", 76)]
    assert [(f, getattr(lc.LossOut, f).offset) for f, _ in lc.LossOut._fields_] == [("dlogits", 0), ("dvalues", 8), ("scalars", 16), ("workspace", 24)]
    assert dict(lc.LossIn._fields_)["n_samples"] is C.c_int64 and dict(lc.LossIn._fields_)["normalize_adv"] is C.c_int32
    assert all(dict(lc.LossIn._fields_)[f] is C.c_float for f in ("clip", "value_coef", "entropy_coef"))
    for name, value in re.findall(r"#define TS_LOSS_([A-Z_]+) (0x[0-9a-f]+|\d+)u?", header):
        if name != "ABI_VERSION":
            assert getattr(lc, name) == int(value, 0), name
    import tiler_slider_amd as pkg
    assert callable(pkg.build_loss_library) and callable(pkg.actor_critic_loss) and callable(pkg.actor_critic_loss_grads)
    assert callable(pkg.VecTilerSliderEnv.trajectory_loss)
    assert pkg.LossInfo._fields == ("loss", "policy", "value", "entropy", "approx_kl", "clip_frac", "count")
    assert {"LossInfo", "actor_critic_loss", "actor_critic_loss_grads", "build_loss_library"} <= set(pkg.__all__)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "value clipping" in design and "ts_loss.hip" in design


def test_every_refusal_has_its_own_status_in_the_headers_order():
    """No HIP call is made before a refusal: on a box without a GPU one would have answered TS_ERR_HIP."""
    from tiler_slider_amd import _cabi
    L = lc.lib()
    M = 100
    buf = (C.c_uint8 * (1 << 20))()
    base = (C.addressof(buf) + 255) & ~255
    at = lambda k: base + k * 16384        # regions apart: 100 samples need at most 1,600 bytes, the workspace 208
    ref = lambda x: C.byref(x) if x is not None else None

    def lin(**kw):
        a = dict(logits=at(0), old_logits=at(1), act=at(2), mask=at(3), adv=at(4), values=at(5), ret=at(6), n_samples=M, clip=0.2, value_coef=0.5,
                 entropy_coef=0.01, normalize_adv=1)
        a.update(kw)
        return lc.LossIn(**a)

    def lout(**kw):
        a = dict(dlogits=at(8), dvalues=at(9), scalars=at(10), workspace=at(11))
        a.update(kw)
        return lc.LossOut(**a)

    call = lambda i, o: L.ts_actor_critic_loss(ref(i), ref(o), None)
    NULL, ARG, OK = _cabi.ERR_NULL, _cabi.ERR_ARG, _cabi.OK
    nothing = lc.LossOut()
    # 1. the struct pointers
    assert call(None, lout()) == NULL and call(lin(), None) == NULL and call(None, None) == NULL
    # 2. bad arguments: before the empty batch and before any pointer (every pointer of `nothing` is NULL)
    bad = (dict(n_samples=-1), dict(clip=-0.1), dict(clip=NAN), dict(clip=0.0), dict(values=None), dict(ret=None), dict(adv=None),
           dict(value_coef=NAN), dict(entropy_coef=NAN))
    for kw in bad:
        for n in (M, 0):
            assert call(lin(**dict(dict(n_samples=n), **kw)), nothing) == ARG, (kw, n)
    assert call(lin(values=None, ret=None), lout()) == ARG          # dvalues given without values
    assert call(lin(old_logits=None, clip=-1.0), nothing) == ARG      # clip is checked with or without old_logits
    assert call(lin(old_logits=None, clip=0.0), nothing) == NULL      # ... and 0 is fine without them: on to the pointers
    assert call(lin(normalize_adv=0, adv=None), nothing) == NULL
    # 3. nothing to do: TS_OK without a launch, no pointer is looked at (scalars NULL: nothing to zero)
    assert call(lc.LossIn(n_samples=0), nothing) == OK
    assert call(lin(n_samples=0, logits=None, act=None, old_logits=at(1) + 1), nothing) == OK
    # 4. missing pointers, before the alignment (old_logits is misaligned throughout)
    odd = dict(old_logits=at(1) + 4)
    assert call(lin(logits=None, **odd), lout()) == NULL and call(lin(act=None, **odd), lout()) == NULL
    for name in ("dlogits", "dvalues", "scalars", "workspace"):
        assert call(lin(**odd), lout(**{name: None})) == NULL, name
    assert call(lin(values=None, ret=None, **odd), lout(dvalues=None)) == ARG       # no value term: no dvalues, on to the alignment
    assert call(lin(mask=None, **odd), lout()) == ARG                               # mask may be missing
    # 5. alignment
    for name in ("logits", "old_logits"):
        for off in (1, 4, 8):
            assert call(lin(**{name: getattr(lin(), name) + off}), lout()) == ARG, (name, off)
    for off in (1, 4, 8):
        assert call(lin(), lout(dlogits=at(8) + off)) == ARG
    for name in ("adv", "values", "ret"):
        for off in (1, 2, 3):
            assert call(lin(**{name: getattr(lin(), name) + off}), lout()) == ARG, (name, off)
    for name in ("dvalues", "scalars", "workspace"):
        for off in (1, 2, 3):
            assert call(lin(), lout(**{name: getattr(lout(), name) + off})) == ARG, (name, off)
    # 6. an output that overlaps an input or another output - by its last byte too
    assert call(lin(), lout(dlogits=at(0))) == ARG and call(lin(), lout(dlogits=at(0) + 16 * (M - 1))) == ARG
    assert call(lin(), lout(dvalues=at(5))) == ARG and call(lin(), lout(dvalues=at(2) + 96)) == ARG     # act's last bytes
    assert call(lin(), lout(scalars=at(8) + 16 * M - 4)) == ARG and call(lin(), lout(workspace=at(10) + 28)) == ARG
    assert call(lin(), lout(workspace=at(9) - lc.workspace_bytes(M) + 4)) == ARG
    assert call(lin(), lout(scalars=at(6) + 4 * (M - 1))) == ARG
    # ... and everything right reaches the launch, which a box without a GPU refuses; one with a GPU is not asked here
    assert L.ts_loss_last_hip_error() == 0
    assert L.ts_loss_workspace_bytes(-1) == ARG and L.ts_loss_workspace_bytes(0) == 0
    desc = lc.LossDesc()
    assert L.ts_describe_loss(1, 0, None) == NULL and L.ts_describe_loss(-1, 0, C.byref(desc)) == ARG and L.ts_describe_loss(1, 0x10, C.byref(desc)) == ARG
    with pytest.raises(_cabi.TilerSliderLibraryError):
        lc.workspace_bytes(-5)


@pytest.mark.parametrize("M", (0, 1, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, GRID - 1, GRID, GRID + 1, 100 * (1 << 20)))
def test_describe_plans_the_bounded_grid_and_counts_the_bytes(M):
    for what in range(16):
        d = lc.describe_loss(M, what)
        old, val, adv, mask = (1 if what & b else 0 for b in (lc.OLD_LOGITS, lc.VALUES, lc.ADV, lc.MASK))
        assert (d["threads_per_block"], d["lds_bytes"], d["samples"]) == (256, 80, M)
        if M == 0:
            assert (d["launches"], d["blocks"], d["partials"], d["workspace_bytes"], d["bytes_read"], d["bytes_written"]) == (0, 0, 0, 0, 0, 0)
            assert d["name"] == d["stats_name"] == d["finish_name"] == ""
            continue
        blocks = min(-(-M // 256), 2048)
        assert (d["launches"], d["blocks"], d["partials"]) == (4, blocks, blocks)
        assert d["workspace_bytes"] == lc.workspace_bytes(M) == 4 * (8 + 11 * blocks)
        first, main = 1 + mask + 4 * adv, 16 + 16 * old + 1 + mask + 4 * adv + 8 * val
        assert 2 <= 1 + 1 + 4 * adv <= 6 and d["bytes_read"] == M * (first + main) and d["bytes_written"] == M * (16 + 4 * val) + 32
        assert (d["name"], d["stats_name"], d["finish_name"]) == ("k_loss_main", "k_loss_stats", "k_loss_finish")
    assert lc.workspace_bytes(GRID + 1) == lc.workspace_bytes(1 << 40)      # the grid is bounded: so is the workspace


def test_describe_names_exactly_the_compiled_kernels():
    compiled = _kernel_names(lc.LIB_PATH)
    d = lc.describe_loss(1000, 15)
    assert len(compiled) == lc.MIN_KERNELS == 3
    assert sorted((d["name"], d["stats_name"], d["finish_name"])) == sorted(compiled)


def test_the_loss_kernels_use_no_scratch_no_agprs_and_the_lds_they_report():
    kernels = _kernel_metadata(lc.LIB_PATH)
    assert len(kernels) == len([k for k in kernels if "k_loss_" in k["name"]]) == lc.MIN_KERNELS
    assert not any(k["private_segment_fixed_size"] or k["agpr_count"] or k["uses_dynamic_stack"] for k in kernels), kernels
    by_name = {re.search(r"k_loss_[a-z]+", k["name"]).group(0): k["group_segment_fixed_size"] for k in kernels}
    assert by_name["k_loss_main"] == lc.describe_loss(1, 0)["lds_bytes"] and max(by_name.values()) <= 256, by_name


def test_the_kept_assembly_has_no_atomic_and_moves_sixteen_bytes_at_a_time(tmp_path):
    """The library compiled once more with its assembly kept (a few seconds): not one atomic instruction of any kind, and the
    logits go in and out as dwordx4."""
    from tiler_slider_amd import _cabi
    _cabi.compile_guarded(lc.SRC, str(tmp_path / "libtiler_slider_loss.so"), work=str(tmp_path), keep_asm=True, min_kernels=lc.MIN_KERNELS)
    asm = open(tmp_path / "libtiler_slider_loss.gfx950.s").read()
    code = "\n".join(line.split(";")[0] for line in asm.splitlines())
    assert len(re.findall(r"atomic", code)) == 0
    assert "global_load_dwordx4" in code and "global_store_dwordx4" in code
    assert "v_exp_f32" in code and "v_log_f32" in code      # __expf, __logf: the hardware's
    assert open(tmp_path / "libtiler_slider_loss.so", "rb").read(4) == b"\x7fELF"


# ---------------------------------------------------------------------------------------------- the yardstick itself
def _yardstick_cases():
    """The three modes as they were, the 24 configurations of the sixteen bodies, and the full normalised body at the three
    coefficient sets off the defaults with a fresh and a stale old policy: id -> (M, seed) -> inputs."""
    import loss_reference as lr
    cases = {mode: (lambda M, seed, mode=mode: lr.case(mode, M, seed)) for mode in lr.MODES}
    for k, (body, nz) in enumerate(lr.CONFIGS):
        cases[lr.body_id(*body, nz)] = lambda M, seed, body=body, nz=nz, k=k: lr.case_of(*body, M, seed + 100 * (k + 1), normalize=nz)
    for k, (clip, vc, ec) in enumerate(lr.COEFFICIENTS):
        for stale in lr.STALES:
            cases[f"clip={clip:g},value={vc:g},entropy={ec:g},stale={stale:g}"] = (
                lambda M, seed, k=k, clip=clip, vc=vc, ec=ec, stale=stale: lr.case_of(1, 1, 1, 1, M, seed + 5000 + k, normalize=True, clip=clip, value_coef=vc,
                                                                                     entropy_coef=ec, stale=stale))
    return cases


YARDSTICK_CASES = _yardstick_cases()


@pytest.mark.parametrize("mode", YARDSTICK_CASES)
def test_the_yardsticks_gradients_are_float64_autograds_of_the_plain_torch_loss(mode):
    """4,000 samples; the coefficients are handed over as the float32 the call receives."""
    import torch
    import loss_reference as lr
    kw = YARDSTICK_CASES[mode](4000, 11)
    want = lr.loss64(**kw)
    t = {}
    for k, v in kw.items():
        if isinstance(v, np.ndarray):
            t[k] = torch.tensor(v if v.dtype == np.uint8 else np.nan_to_num(v).astype(np.float64))
        else:
            t[k] = float(np.float32(v)) if isinstance(v, float) else v
    t["logits"].requires_grad_(True)
    if "values" in t:
        t["values"].requires_grad_(True)
    loss = lr.torch_loss(**t)
    loss.backward()
    assert abs(float(loss.detach()) - want.scalars[0]) <= 1e-13 * max(1.0, abs(want.scalars[0]))
    tol = 1e-16
    if "stale=3" in mode:
        # a far-off old policy: r = exp(log p - log p_old) reaches thousands, and a row of the gradient, r A c (delta - p), is no
        # longer below 1e-3.  log r is four float64 operations on magnitudes below max |z| + log 4 < 32, which the exponential turns
        # into at most 4 * 32 = 128 float64 roundings of r, doubled for the products behind it: 2**-45 of the row's largest entry
        tol = np.maximum(tol, 2.0 ** -45 * np.abs(want.dlogits).max(axis=1, keepdims=True))
        assert np.abs(kw["logits"][want.live]).max() + np.log(4) < 32 and np.abs(kw["old_logits"][want.live]).max() + np.log(4) < 32
    assert (np.abs(t["logits"].grad.numpy() - want.dlogits) <= tol).all() and np.abs(want.dlogits).max() > 1e-6
    assert (t["logits"].grad.numpy()[~want.live] == 0).all() and (want.dlogits[~want.live] == 0).all()
    if "values" in t:
        assert np.abs(t["values"].grad.numpy() - want.dvalues).max() <= 1e-16
        assert np.abs(want.dvalues).max() > 1e-6 if kw["value_coef"] else (want.dvalues == 0).all() and (want.dvalues_bound == 0).all()
    if "old_logits" in kw and kw["clip"] == 0.2:
        assert 0.05 < want.scalars[5] < 0.95 and want.scalars[4] > 0      # the clip cuts some samples, not all
    elif "old_logits" in kw:
        assert (want.scalars[5] == 0) == (kw["clip"] == 1e30) and want.scalars[5] < 0.95 and want.scalars[4] > 0
    else:
        assert want.scalars[4] == 0 and want.scalars[5] == 0
    assert (want.dvalues is None) == ("values" not in kw) and (want.scalars[7] == 0 or "adv" in kw)


@pytest.mark.parametrize("mode", YARDSTICK_CASES)
def test_the_bound_holds_float32_numpy_in_two_orders_and_notices_a_wrong_one(mode):
    """10,000 Gaussian samples: both float32 evaluations lie within the per-entry bound on every sample that is not ambiguous (at
    most 1 % are) and within the scalar bounds, and use more than a thousandth of it; an evaluation whose gradient drops c
    leaves it on nine samples in ten."""
    import loss_reference as lr
    kw = YARDSTICK_CASES[mode](10000, 1)
    want = lr.loss64(**kw)
    ok = want.live & ~want.ambiguous
    assert want.ambiguous.sum() <= 0.01 * want.live.sum() and 0.7 < want.live.mean() < 0.95
    for order in (0, 1):
        dz, dv, sc = lr.loss32(order=order, **kw)
        ratio = np.abs(dz - want.dlogits)[ok] / want.dlogits_bound[ok]
        print(f"{mode} order {order}: worst dlogits error / bound {ratio.max():.3f}")
        assert 1e-3 < ratio.max() <= 1.0
        assert (dz[~want.live] == 0).all()
        if dv is not None:
            rv = lr.worst(np.abs(dv - want.dvalues)[want.live], want.dvalues_bound[want.live])
            assert rv <= 1.0 and (dv[~want.live] == 0).all()
        assert (np.abs(sc - want.scalars) <= want.scalars_bound).all(), (sc, want.scalars, want.scalars_bound)
    dz, _, _ = lr.loss32(**kw)
    wrong = dz * np.float32(want.live.sum())
    assert (np.abs(wrong - want.dlogits)[ok] > want.dlogits_bound[ok]).mean() > 0.9
    # the relative size of the bound: a few ulp of the gradient's own size, not a tolerance that anything passes
    rel = want.dlogits_bound[ok] / np.maximum(np.abs(want.dlogits[ok]).max(axis=1, keepdims=True), 1e-30)
    assert np.median(rel) < 2e-5


def test_the_exact_case_is_exact_in_float64_and_float32():
    import loss_reference as lr
    for log2, extra in ((8, 1), (10, 4), (0, 3)):
        kw, dz, dv, n = lr.exact_case(log2, extra)
        want = lr.loss64(**kw)
        got = lr.loss32(**kw)
        assert want.scalars[6] == n == 1 << log2
        np.testing.assert_array_equal(want.dlogits, dz.astype(np.float64))
        np.testing.assert_array_equal(want.dvalues, dv.astype(np.float64))
        np.testing.assert_array_equal(got[0], dz)
        np.testing.assert_array_equal(got[1], dv)
        assert np.isnan(kw["logits"]).any() and not np.isnan(dz).any() and (np.abs(dz).max() > 0 or n == 1)


def test_the_guard_names_the_samples_at_the_clips_edge():
    """r set to 1 + clip to within a float32 rounding: ambiguous; a tenth of clip away from it: not."""
    import loss_reference as lr
    f32 = np.float32
    z = np.zeros((4, 4), f32)
    old = np.zeros((4, 4), f32)
    # action 0: r = exp(lp0 - lpo0).  Lowering the old policy's logit 0 raises r.
    for i, r_target in enumerate((1.2, 1.2 * (1 + 1e-7), 1.1, 1.3)):
        # softmax of (t, 0, 0, 0) at 0 is e^t / (e^t + 3): solve for the t that gives 0.25 / r_target
        q = 0.25 / r_target
        old[i, 0] = np.log(3 * q / (1 - q))
    kw = dict(logits=z, act=np.zeros(4, np.uint8), adv=np.array([1, 1, 1, -1], f32), old_logits=old, clip=0.2)
    want = lr.loss64(**kw)
    assert want.ambiguous.tolist() == [True, True, False, False]
    assert want.terms["cut"].tolist()[2:] == [0.0, 0.0] and want.dlogits[3].any()     # inside: a tie, unclipped; outside with A < 0: unclipped
