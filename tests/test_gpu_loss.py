"""The fused actor-critic loss on the GPU (lib/libtiler_slider_loss.so) against the float64 yardstick of tests/loss_reference.py:
the exact case bit for bit, the three modes inside the a-priori bound at every size at which the grid takes another shape, each
of the sixteen compiled bodies of k_loss_main (and the four of k_loss_stats) inside it, coefficients off the defaults, the
relations that tie one body to another bit for bit, the edge cases, determinism, raw calls into guarded memory, the autograd
wrapper, the routes of trajectory_loss, and the loss end to end behind an ActorCriticNet against the plain-torch loss."""
import ctypes as C
import functools

import numpy as np
import pytest

import loss_reference as lr
from table_harness import GUARD, guarded as _guarded, payload as _payload

pytestmark = pytest.mark.gpu

BLOCK, GRID = 256, 2048 * 256
SIZES = (1, 63, 64, 65, 1285, BLOCK - 1, BLOCK, BLOCK + 1, 2 * GRID + 3)   # the last: every block strides twice, with a ragged end


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def _case(mode, M, spread=None):
    """The inputs and the yardstick's answer, computed once and shared (never written to)."""
    kw = lr.case(mode, M, 1000 + M % 997, spread=spread)
    return kw, lr.loss64(**kw)


def _seed(body, M):
    return 3000 + 31 * lr.BODIES.index(tuple(body)) + M % 997


@functools.lru_cache(maxsize=None)
def _case_of(body, normalize, M, coefficients=None, stale=0.5):
    """The same for one of the sixteen bodies (M <= 1285: the yardstick is computed)."""
    assert M <= 1285
    co = {} if coefficients is None else dict(zip(("clip", "value_coef", "entropy_coef"), coefficients))
    kw = lr.case_of(*body, M, _seed(body, M), normalize=normalize, stale=stale, **co)
    return kw, lr.loss64(**kw)


# four more bodies for determinism and guarded memory: with the three modes they repeat all four bodies of k_loss_stats
MORE_BODIES = {lr.body_id(*b): b for b in ((1, 0, 1, 0), (0, 1, 0, 1), (1, 1, 0, 0), (0, 0, 1, 1))}


def _to(torch, kw):
    dev = torch.device("cuda", 0)
    return {k: torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v for k, v in kw.items()}


def _run(torch, kw):
    from tiler_slider_amd import loss as loss_mod
    t = _to(torch, kw)
    scalars, dz, dv = loss_mod._run(t["logits"], t.get("values"), t["act"], t.get("mask"), t.get("adv"), t.get("old_logits"), t.get("ret"),
                                    kw.get("clip", 0.0), kw.get("value_coef", 0.5), kw.get("entropy_coef", 0.0), kw.get("normalize_adv", False))
    return scalars.cpu().numpy(), dz.cpu().numpy(), None if dv is None else dv.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _hold(mode, M, want, scalars, dz, dv):
    """Gradients inside the per-entry bound on every live sample that is not ambiguous (at most 1 % are), exact zeros elsewhere;
    scalars inside theirs.  Where a bound is exactly 0 the error must be exactly 0 (lr.worst: infinite otherwise).  Prints each
    figure before it asserts."""
    ok = want.live & ~want.ambiguous
    assert want.ambiguous.sum() <= 0.01 * max(1, want.live.sum()), (mode, M, "ambiguous samples")
    err = np.abs(dz.astype(np.float64) - want.dlogits)
    ratio = lr.worst(err[ok], want.dlogits_bound[ok])
    rv = 0.0
    if dv is not None:
        rv = lr.worst(np.abs(dv.astype(np.float64) - want.dvalues)[want.live], want.dvalues_bound[want.live])
    serr = np.abs(scalars.astype(np.float64) - want.scalars)
    print(f"{mode} M={M}: worst dlogits error / bound {ratio:.3f}, dvalues {rv:.3f}; scalars error / bound "
          f"{[round(float(e / b), 3) if b else float(e) for e, b in zip(serr, want.scalars_bound)]}; ambiguous {int(want.ambiguous.sum())}; "
          f"cut share {float(scalars[5]):.4f} (yardstick {want.scalars[5]:.4f})")
    assert np.isfinite(dz).all() and (dz[~want.live] == 0).all()
    assert ratio <= 1.0, (mode, M, ratio)
    if dv is not None:
        assert np.isfinite(dv).all() and (dv[~want.live] == 0).all() and rv <= 1.0, (mode, M, rv)
    assert np.isfinite(scalars).all() and (serr <= want.scalars_bound).all(), (mode, M, scalars, want.scalars, want.scalars_bound)


# ---------------------------------------------------------------------------------------------- 1. the exact case
@pytest.mark.parametrize("log2, extra", ((8, 1), (10, 4), (0, 3), (19, 2 * GRID + 3 - (1 << 19))))
def test_the_exact_case_holds_bit_for_bit(torch_cuda, log2, extra):
    """All four logits equal, integer adv and values - ret, a power of two of live samples, entropy_coef = 0; NaN in every float
    input of the samples that are not live; the output buffers (the raw call's own, prefilled with NaN) bit-equal to
    -A (delta - 1/4) c and 2 c value_coef (v - ret).  The last case strides every block twice."""
    torch = torch_cuda
    from tiler_slider_amd import _loss_cabi as lc
    kw, want_dz, want_dv, n = lr.exact_case(log2, extra)
    t = _to(torch, kw)
    M = want_dz.shape[0]
    dev = t["logits"].device
    dz = torch.full((M, 4), float("nan"), dtype=torch.float32, device=dev)
    dv = torch.full((M,), float("nan"), dtype=torch.float32, device=dev)
    scalars = torch.full((8,), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.full((lc.workspace_bytes(M),), 0xFF, dtype=torch.uint8, device=dev)      # NaN patterns in the workspace too
    lin = lc.LossIn(t["logits"].data_ptr(), None, t["act"].data_ptr(), t["mask"].data_ptr(), t["adv"].data_ptr(), t["values"].data_ptr(),
                    t["ret"].data_ptr(), M, 0.0, 0.5, 0.0, 0)
    lout = lc.LossOut(dz.data_ptr(), dv.data_ptr(), scalars.data_ptr(), ws.data_ptr())
    assert lc.lib().ts_actor_critic_loss(C.byref(lin), C.byref(lout), torch.cuda.current_stream(dev).cuda_stream) == 0
    np.testing.assert_array_equal(dz.cpu().numpy(), want_dz)
    np.testing.assert_array_equal(dv.cpu().numpy(), want_dv)
    s = scalars.cpu().numpy()
    want = lr.loss64(**kw)
    assert s[6] == n and s[4] == 0 and s[5] == 0
    if log2 <= 10:      # the squared errors are integers whose sum stays below 2**24: exact in any order
        assert s[2] == np.float32(want.scalars[2])
    assert s[7] == np.float32(want.scalars[7])                                                  # mu: an integer sum over a power of two
    assert (np.abs(s - want.scalars) <= want.scalars_bound).all(), (s, want.scalars)


# ---------------------------------------------------------------------------------------------- 2. the three modes at every size
@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("mode", lr.MODES)
def test_gradients_and_scalars_lie_inside_the_bound(torch_cuda, mode, M):
    kw, want = _case(mode, M)
    _hold(mode, M, want, *_run(torch_cuda, kw))


@pytest.mark.parametrize("mode", lr.MODES)
def test_a_logit_spread_of_200_gives_finite_outputs_inside_the_bound(torch_cuda, mode):
    kw, want = _case(mode, 1285, 200.0)
    z = kw["logits"][want.live]
    assert (z.max(axis=1) - z.min(axis=1)).min() > 199
    _hold(mode, 1285, want, *_run(torch_cuda, kw))


# ---------------------------------------------------------------------------------------------- 2b. every compiled body
_CONFIG_IDS = [lr.body_id(*b, nz) for b, nz in lr.CONFIGS]


@pytest.mark.parametrize("M", (1, BLOCK + 1, 1285))
@pytest.mark.parametrize("body, normalize", lr.CONFIGS, ids=_CONFIG_IDS)
def test_every_body_lies_inside_the_bound(torch_cuda, body, normalize, M):
    """k_loss_main picks one of sixteen bodies by which of old_logits, values, adv and mask are given, k_loss_stats one of four by
    adv and mask: each of them, and each body with adv once more with normalize_adv, at one sample, at two blocks and at 1285."""
    old, val, adv, mask = body
    kw, want = _case_of(body, normalize, M)
    assert [k in kw for k in ("old_logits", "values", "adv", "mask")] == [bool(x) for x in body]
    scalars, dz, dv = _run(torch_cuda, kw)
    _hold(lr.body_id(*body, normalize), M, want, scalars, dz, dv)
    assert scalars[6] == want.live.sum() >= 1
    if not adv:
        assert scalars[7] == 0.0
    if not old:
        assert scalars[4] == 0.0 and scalars[5] == 0.0
    assert (dv is None) == (not val)


@pytest.mark.parametrize("stale", lr.STALES)
@pytest.mark.parametrize("coefficients", lr.COEFFICIENTS, ids=lambda c: "clip={:g},value={:g},entropy={:g}".format(*c))
def test_coefficients_off_the_defaults(torch_cuda, coefficients, stale):
    """The full body with normalize_adv at 1285 samples: a narrow clip under a heavy value and entropy term, 1 - clip < 0 with
    no weight on the value term and an entropy penalty, and a clip that never cuts; the old policy close by and far off."""
    clip, value_coef, entropy_coef = coefficients
    kw, want = _case_of((1, 1, 1, 1), True, 1285, coefficients, stale)
    scalars, dz, dv = _run(torch_cuda, kw)
    _hold("clip={:g},value={:g},entropy={:g},stale={:g}".format(*coefficients, stale), 1285, want, scalars, dz, dv)
    if value_coef == 0.0:
        assert (dv == 0).all()
    if clip == 1e30:
        assert scalars[5] == 0.0
    if clip == 1.5 and stale == 3.0:    # the lower edge is negative and r is not: only the upper edge can cut
        assert 0.0 < scalars[5] < 1.0 and 0.0 < want.scalars[5] < 1.0
        assert abs(float(scalars[5]) - want.scalars[5]) <= want.scalars_bound[5]


# ---------------------------------------------------------------------------------------------- 2c. one body against another
# No tolerance and no float64 pass: every block strides twice, with a ragged end.
RELATION_M = 2 * GRID + 3
_EIGHT = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]


def _three_id(names):
    return lambda t: "+".join(n for n, on in zip(names, t) if on) or "none"


def _live(kw):
    return (kw["act"] <= 3) & ((kw["mask"] != 0) if "mask" in kw else True)


def _same(a, b, scalars, what):
    """(scalars, dlogits, dvalues) of two calls: the gradients and the scalars named bit for bit, and neither is empty."""
    assert a[0][6] > 0.7 * RELATION_M and np.abs(a[1]).max() > 0, what
    assert np.array_equal(_bits(a[1]), _bits(b[1])), (what, "dlogits")
    assert np.array_equal(_bits(a[0][list(scalars)]), _bits(b[0][list(scalars)])), (what, a[0], b[0])


@pytest.mark.parametrize("setting", _EIGHT, ids=_three_id(("old", "val", "adv")))
def test_a_mask_of_all_ones_is_no_mask_bit_for_bit(torch_cuda, setting):
    """Each body and each first pass that reads a mask against its twin that does not: all outputs and all eight scalars.
    An edit of ts_loss.hip that fails it, by the source: `m = 0u` as the default of a body without a mask, in either kernel -
    that body then has no live sample (count 0 from k_loss_stats, all-zero gradients from k_loss_main)."""
    old, val, adv = setting
    kw = lr.case_of(old, val, adv, 0, RELATION_M, _seed((old, val, adv, 0), RELATION_M))
    a, b = _run(torch_cuda, kw), _run(torch_cuda, dict(kw, mask=np.ones(RELATION_M, np.uint8)))
    _same(a, b, range(8), setting)
    assert (a[2] is None and b[2] is None) if not val else np.array_equal(_bits(a[2]), _bits(b[2]))


@pytest.mark.parametrize("setting", _EIGHT, ids=_three_id(("old", "val", "mask")))
def test_an_adv_of_all_ones_is_no_adv_bit_for_bit(torch_cuda, setting):
    """Not normalised.  The gradients and scalars 0-6; mu is 1 where there is an adv (the float64 sum of count ones over count)
    and 0 where there is none.  An edit that fails it: `adv = 0.0f` as k_loss_main's default without adv - A is then 0 on one
    side and 1 on the other, and so is g."""
    old, val, mask = setting
    kw = lr.case_of(old, val, 0, mask, RELATION_M, _seed((old, val, 0, mask), RELATION_M))
    ones = np.where(_live(kw), np.float32(1), np.float32(np.nan))
    a, b = _run(torch_cuda, kw), _run(torch_cuda, dict(kw, adv=ones))
    _same(a, b, range(7), setting)
    assert (a[2] is None and b[2] is None) if not val else np.array_equal(_bits(a[2]), _bits(b[2]))
    assert a[0][7] == 0.0 and b[0][7] == 1.0


@pytest.mark.parametrize("setting", _EIGHT, ids=_three_id(("val", "adv", "mask")))
def test_old_logits_of_the_same_bits_are_no_old_logits_bit_for_bit(torch_cuda, setting):
    """log r is an exact 0 and r an exact 1: nothing is cut, the KL is 0 and the gradient is that of -A log p.  The policy scalar is
    not compared (-A on one side, -A log p on the other), nor the loss that contains it.  An edit that fails it: the clamp's
    edges swapped, fmaxf(fminf(r, lo), hi) - it returns hi for r = 1, u2 = 1.2 A, and every sample of negative A is cut (g = 0,
    clip_frac > 0); or `kl = r - d`, which is 1 here."""
    val, adv, mask = setting
    kw = lr.case_of(0, val, adv, mask, RELATION_M, _seed((0, val, adv, mask), RELATION_M))
    a, b = _run(torch_cuda, kw), _run(torch_cuda, dict(kw, old_logits=kw["logits"].copy(), clip=0.2))
    _same(a, b, (2, 3, 6, 7), setting)
    assert (a[2] is None and b[2] is None) if not val else np.array_equal(_bits(a[2]), _bits(b[2]))
    assert b[0][4] == 0.0 and b[0][5] == 0.0


@pytest.mark.parametrize("setting", _EIGHT, ids=_three_id(("old", "adv", "mask")))
def test_a_value_coef_of_zero_is_no_value_term_bit_for_bit(torch_cuda, setting):
    """dlogits and the loss, policy, entropy, KL, cut, count and mu scalars (the loss adds 0 * a finite sum); dvalues all zero; the
    value scalar against the float64 mean of (v - ret)^2 over the live samples, inside 64 * 2**-24 of itself.  An edit that
    fails it: `k2 = 2.0f * c` (the coefficient dropped from dvalues), or `dv` for `dv * dv` in the VAL-only sum."""
    old, adv, mask = setting
    kw = lr.case_of(old, 1, adv, mask, RELATION_M, _seed((old, 1, adv, mask), RELATION_M), value_coef=0.0)
    bare = {k: v for k, v in kw.items() if k not in ("values", "ret", "value_coef")}
    a, b = _run(torch_cuda, bare), _run(torch_cuda, kw)
    _same(a, b, (0, 1, 3, 4, 5, 6, 7), setting)
    assert a[2] is None and (b[2] == 0).all() and a[0][2] == 0.0
    live = _live(kw)
    want = float(((kw["values"][live].astype(np.float64) - kw["ret"][live].astype(np.float64)) ** 2).mean())
    print(f"value scalar {float(b[0][2])!r}, float64 {want!r}, error / bound {abs(float(b[0][2]) - want) / (64 * lr.U * want):.3f}")
    assert want > 0.5 and abs(float(b[0][2]) - want) <= 64 * lr.U * want


# ---------------------------------------------------------------------------------------------- 3. the edges
@pytest.mark.parametrize("mode", lr.MODES)
def test_no_live_sample_gives_zeros_and_no_nan(torch_cuda, mode):
    kw = dict(lr.case(mode, 1285, 3))
    kw["act"] = np.full(1285, 255, np.uint8)
    for name in ("logits", "old_logits", "adv", "values", "ret"):
        if name in kw:
            kw[name] = np.full_like(kw[name], np.nan)
    scalars, dz, dv = _run(torch_cuda, kw)
    assert (_bits(scalars) == 0).all() and (_bits(dz) == 0).all() and (dv is None or (_bits(dv) == 0).all())
    if "mask" in kw:        # ... and by the mask alone
        kw["act"] = np.zeros(1285, np.uint8)
        kw["mask"] = np.zeros(1285, np.uint8)
        scalars, dz, dv = _run(torch_cuda, kw)
        assert (_bits(scalars) == 0).all() and (_bits(dz) == 0).all() and (_bits(dv) == 0).all()


def test_normalize_adv_with_one_live_sample(torch_cuda):
    """sigma is 0 and adv - mu is exactly 0: A = 0 / 1e-8 = 0, so the policy term and its gradient vanish; the entropy and value
    terms remain, and nothing is NaN."""
    kw = dict(lr.case("ppo", 300, 4))
    kw["mask"] = np.zeros(300, np.uint8)
    one = int(np.flatnonzero(kw["act"] <= 3)[7])
    kw["mask"][one] = 1
    for name in ("logits", "old_logits"):
        kw[name][one] = np.float32([0.5, -1.0, 2.0, 0.25]) + (0.3 if name == "old_logits" else 0.0) * np.float32([1, -1, 0, 2])
    kw["adv"][one], kw["values"][one], kw["ret"][one] = 3.75, 1.5, -0.5
    want = lr.loss64(**kw)
    assert want.live.sum() == 1 and want.scalars[1] == 0.0 and want.scalars[7] == 3.75
    scalars, dz, dv = _run(torch_cuda, kw)
    _hold("ppo, one live sample", 300, want, scalars, dz, dv)
    assert scalars[1] == 0 and scalars[6] == 1 and scalars[7] == np.float32(3.75) and dv[one] == np.float32(2 * 0.5 * 2.0)


def test_no_sample_at_all(torch_cuda):
    torch = torch_cuda
    from tiler_slider_amd import actor_critic_loss_grads
    dev = torch.device("cuda", 0)
    info, dz, dv = actor_critic_loss_grads(torch.empty((0, 4), device=dev), torch.empty((0,), dtype=torch.uint8, device=dev))
    assert tuple(dz.shape) == (0, 4) and dv is None and all(float(x) == 0.0 for x in info)


# ---------------------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("mode", lr.MODES + tuple(MORE_BODIES))
def test_two_identical_calls_agree_bit_for_bit_at_the_largest_size(torch_cuda, mode):
    if mode in MORE_BODIES:
        kw = lr.case_of(*MORE_BODIES[mode], SIZES[-1], _seed(MORE_BODIES[mode], SIZES[-1]), normalize=bool(MORE_BODIES[mode][2]))
    else:
        kw, _ = _case(mode, SIZES[-1])
    a, b = _run(torch_cuda, kw), _run(torch_cuda, kw)
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y))


# ---------------------------------------------------------------------------------------------- 5. the raw C-ABI into guarded memory
@pytest.mark.parametrize("M, mode", [(M, mode) for mode in lr.MODES for M in (1, 321, GRID + 259)] + [(321, body) for body in MORE_BODIES])
def test_raw_calls_into_guarded_memory(torch_cuda, mode, M):
    """Every buffer of the call between 256 guard bytes, M no multiple of 4, the outputs prefilled with NaN: the guards and the
    inputs are as they were, the outputs are the yardstick's.  An input the body does not take is NULL, and so is dvalues
    where there is no value term."""
    torch = torch_cuda
    from tiler_slider_amd import _loss_cabi as lc
    dev = torch.device("cuda", 0)
    assert M % 4
    kw, want = _case_of(MORE_BODIES[mode], False, M) if mode in MORE_BODIES else _case(mode, M)
    ins = {k: v for k, v in kw.items() if isinstance(v, np.ndarray)}
    g = {k: _guarded(torch, dev, v) for k, v in ins.items()}
    outs = {"dlogits": np.full((M, 4), np.nan, np.float32), "scalars": np.full(8, np.nan, np.float32),
            "workspace": np.full(lc.workspace_bytes(M), 0xFF, np.uint8)}
    if "values" in ins:
        outs["dvalues"] = np.full(M, np.nan, np.float32)
    g.update({k: _guarded(torch, dev, v) for k, v in outs.items()})
    at = lambda k: g[k].data_ptr() + GUARD if k in g else None
    lin = lc.LossIn(at("logits"), at("old_logits"), at("act"), at("mask"), at("adv"), at("values"), at("ret"), M, kw.get("clip", 0.0),
                    kw.get("value_coef", 0.5), kw.get("entropy_coef", 0.0), int(kw.get("normalize_adv", False)))
    assert ("dvalues" in g) == ("values" in ins) == ("ret" in ins)
    lout = lc.LossOut(at("dlogits"), at("dvalues"), at("scalars"), at("workspace"))
    assert lc.lib().ts_actor_critic_loss(C.byref(lin), C.byref(lout), torch.cuda.current_stream(dev).cuda_stream) == 0
    dz, scalars = _payload(g["dlogits"], np.float32, (M, 4)), _payload(g["scalars"], np.float32, (8,))
    dv = _payload(g["dvalues"], np.float32, (M,)) if "dvalues" in outs else None
    _payload(g["workspace"], np.uint8, (outs["workspace"].size,))
    for k, v in ins.items():
        np.testing.assert_array_equal(_payload(g[k], np.uint8, (v.nbytes,)), np.ascontiguousarray(v).reshape(-1).view(np.uint8), err_msg=k)
    _hold(mode, M, want, scalars, dz, dv)


# ---------------------------------------------------------------------------------------------- 6. autograd
def test_the_loss_carries_one_grad_fn_and_backward_scales(torch_cuda):
    torch = torch_cuda
    from tiler_slider_amd import actor_critic_loss, actor_critic_loss_grads
    kw, want = _case("a2c", 1285)
    t = _to(torch, {k: (np.nan_to_num(v) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in kw.items()})
    z, v = t.pop("logits").reshape(5, 257, 4), t.pop("values").reshape(5, 257)
    rest = {k: (x.reshape(5, 257) if isinstance(x, torch.Tensor) else x) for k, x in t.items()}
    act = rest.pop("act")
    info, dz, dv = actor_critic_loss_grads(z, act, values=v, **rest)
    assert info.loss.dim() == 0 and info.loss.grad_fn is None and dz.shape == z.shape and dv.shape == v.shape
    assert (np.abs(dz.cpu().numpy().reshape(-1, 4).astype(np.float64) - want.dlogits) <= want.dlogits_bound).all()
    # no grad asked for: no grad_fn
    assert actor_critic_loss(z, act, values=v, **rest).loss.grad_fn is None
    zg, vg = z.clone().requires_grad_(True), v.clone().requires_grad_(True)
    with torch.no_grad():
        assert actor_critic_loss(zg, act, values=vg, **rest).loss.grad_fn is None
    out = actor_critic_loss(zg, act, values=vg, **rest)
    assert out.loss.grad_fn is not None and "Loss" in type(out.loss.grad_fn).__name__ and torch.equal(out.loss.detach(), info.loss)
    assert all(getattr(out, f).grad_fn is None and torch.equal(getattr(out, f), getattr(info, f)) for f in out._fields[1:])
    out.loss.backward()
    assert torch.equal(zg.grad, dz) and torch.equal(vg.grad, dv)
    # backward(2.0) doubles the gradients, and a second call accumulates into .grad
    zg.grad = vg.grad = None
    actor_critic_loss(zg, act, values=vg, **rest).loss.backward(torch.tensor(2.0, device=z.device))
    assert torch.equal(zg.grad, 2 * dz) and torch.equal(vg.grad, 2 * dv)
    actor_critic_loss(zg, act, values=vg, **rest).loss.backward()
    assert torch.equal(zg.grad, 2 * dz + dz) and torch.equal(vg.grad, 2 * dv + dv)
    # only the logits require grad: the values get none
    zg.grad = vg.grad = None
    actor_critic_loss(zg, act, values=vg.detach(), **rest).loss.backward()
    assert torch.equal(zg.grad, dz) and vg.grad is None
    # the raw form feeds autograd.backward directly
    w = torch.ones(4, device=z.device, requires_grad=True)
    torch.autograd.backward((z * w,), (dz,))
    assert torch.allclose(w.grad, (z * dz).sum((0, 1)))
    for bad in (dict(values=v[:, :-1]), dict(values=v.double()), dict(values=v.t().contiguous().t()), dict(values=v.cpu())):
        with pytest.raises(ValueError):
            actor_critic_loss(z, act, **{**rest, **bad})
    with pytest.raises(ValueError):
        actor_critic_loss(z, act, values=v, **{**rest, "ret": None})


# ---------------------------------------------------------------------------------------------- 7. end to end
def _boards(torch, oracle, n=257, max_steps=6):
    from tiler_slider_amd import VecTilerSliderEnv
    blk, init, tgt = oracle.generate(4, 2, 2, 2, n, seed=0x715311DE)
    env = VecTilerSliderEnv.from_arrays(4, blk, init, tgt, multi_color=True, max_steps=max_steps, device=torch.device("cuda", 0), auto_reset=True,
                                        obs_dtype=None)
    env.reset()
    return env


def test_end_to_end_the_grads_of_an_actor_critic_net_are_the_plain_torch_losses(torch_cuda, oracle):
    """257 boards of 4x4 with 2 tiles, K = 5, H = 16: the six .grads through trajectory_loss against those of the README's torch
    loss on the same rollout.  Tolerance: 8 x the larger of the torch path's own difference between two runs (its backward adds
    with float atomics), measured here, and float32 epsilon times the gradient's largest magnitude - the two paths round
    log_softmax differently.  Also: PPO's errors for a rollout without its logits, and the ValueErrors of trajectory_loss."""
    torch = torch_cuda
    from tiler_slider_amd import ActorCriticNet, RewardWeights
    env = _boards(torch, oracle)
    dev = env.device
    net = ActorCriticNet(env.onehot_channels * 16, 16, dev, generator=torch.Generator(device=dev).manual_seed(3))
    out = env.rollout_policy(5, net.policy(), select="sample", seed=5, log=("start", "pos", "act", "flags", "logits"))
    names = ("w1", "b1", "w2", "b2", "wv", "bv")

    def grads(fused, clip=0.0):
        net.zero_grad(set_to_none=True)
        logits, v = env.trajectory_outputs(net, out)
        with torch.no_grad():
            last = env.trajectory_outputs(net)[1][0]
        tr = env.trajectory_returns(out, 0.97, 0.9, values=v, last_value=last, reward=RewardWeights(step=-0.01, win=1.0))
        if fused:
            info = env.trajectory_loss(logits, out, tr, values=v, clip=clip)
            loss = info.loss
        else:
            logp = torch.log_softmax(logits, dim=2).gather(2, out.act_log.clamp(max=3).long().unsqueeze(2)).squeeze(2)
            live = tr.mask.float()
            loss = (-(tr.adv * logp * live).sum() + 0.5 * (((v - tr.ret) ** 2) * live).sum()) / live.sum()
        loss.backward()
        return float(loss.detach()), [getattr(net, k).grad.detach().clone() for k in names]

    l1, g1 = grads(False)
    l2, g2 = grads(False)
    lf, gf = grads(True)
    eps = float(np.finfo(np.float32).eps)
    print(f"loss torch {l1!r} fused {lf!r}")
    assert abs(lf - l1) <= 64 * eps * max(1.0, abs(l1))
    for k, a, b, f in zip(names, g1, g2, gf):
        own, top = float((a - b).abs().max()), float(a.abs().max())
        tol = 8 * max(own, eps * top)
        diff = float((f - a).abs().max())
        print(f"{k}: fused - torch {diff:.3e}, torch's own run-to-run {own:.3e}, eps * max |grad| {eps * top:.3e}, tolerance {tol:.3e}")
        assert top > 0 and diff <= tol, (k, diff, tol)
    # PPO against the policy that played: at the first update r = 1 everywhere, nothing is cut and the KL is 0
    info = env.trajectory_loss(*env.trajectory_outputs(net, out)[:1], out, env.trajectory_returns(out), clip=0.2)
    assert float(info.clip_frac) == 0.0 and abs(float(info.approx_kl)) <= 1e-6 and float(info.count) > 0
    bare = env.rollout_policy(5, net.policy(), seed=6, log=("start", "pos", "act", "flags"))
    z = env.trajectory_outputs(net, bare)[0]
    with pytest.raises(ValueError, match="logits"):
        env.trajectory_loss(z, bare, env.trajectory_returns(bare), clip=0.2)
    with pytest.raises(ValueError, match="act"):
        env.trajectory_loss(z, env.rollout_policy(5, net.policy(), seed=6, log=("start", "pos", "flags")))
    with pytest.raises(ValueError):
        env.trajectory_loss(z[:4], bare)
    with pytest.raises(ValueError):
        env.trajectory_loss(z, bare, values=z[..., 0].contiguous())
    env.close()


def test_every_route_of_trajectory_loss_is_the_raw_call_on_the_inputs_it_documents(torch_cuda, oracle):
    """The end-to-end test's setting.  trajectory_loss looks its arguments up - the actions or the labels, the mask and the
    advantages of the targets, the returns where there are values, the rollout's logits where clip > 0 - and each route returns
    the bits of actor_critic_loss_grads called by hand on those: all seven fields, and both gradients after backward()."""
    torch = torch_cuda
    from tiler_slider_amd import ActorCriticNet, LossInfo, RewardWeights, actor_critic_loss_grads
    env = _boards(torch, oracle)
    dev = env.device
    net = ActorCriticNet(env.onehot_channels * 16, 16, dev, generator=torch.Generator(device=dev).manual_seed(3))
    out = env.rollout_policy(5, net.policy(), select="sample", seed=5, log=("start", "pos", "act", "flags", "logits"))
    with torch.no_grad():
        logits, v = env.trajectory_outputs(net, out)
        last = env.trajectory_outputs(net)[1][0]
    tr = env.trajectory_returns(out, 0.97, 0.9, values=v, last_value=last, reward=RewardWeights(step=-0.01, win=1.0))
    labels = env.trajectory_labels(out, env.build_table())[2]
    assert bool((labels != 255).any()) and bool(tr.mask.any())
    targets = dict(mask=tr.mask, adv=tr.adv)
    routes = (("targets", (tr,), {}, dict(targets)),
              ("targets, clip", (tr,), dict(clip=0.2), dict(targets, old_logits=out.logits_log, clip=0.2)),
              ("targets, values, normalised", (tr,), dict(values=v, normalize_adv=True), dict(targets, values=v, ret=tr.ret, normalize_adv=True)),
              ("labels", (), dict(labels=labels), {}),
              ("targets, labels", (tr,), dict(labels=labels), dict(targets)))
    for name, args, kw, by_hand in routes:
        z = logits.clone().requires_grad_(True)
        if "values" in kw:
            kw["values"] = v.clone().requires_grad_(True)
        info = env.trajectory_loss(z, out, *args, **kw)
        want, dz, dv = actor_critic_loss_grads(logits, labels if "labels" in kw else out.act_log, **by_hand)
        assert isinstance(info, LossInfo) and float(want.count) > 0, name
        for field in LossInfo._fields:
            assert torch.equal(getattr(info, field).detach().view(torch.int32), getattr(want, field).view(torch.int32)), (name, field)
        info.loss.backward()
        assert torch.equal(z.grad.view(torch.int32), dz.view(torch.int32)) and bool(dz.any()), name
        assert (dv is None) == ("values" not in kw), name
        if dv is not None:
            assert torch.equal(kw["values"].grad.view(torch.int32), dv.view(torch.int32)) and bool(dv.any()), name
    env.close()


def test_inputs_that_start_one_float_into_a_buffer_give_the_bits_of_aligned_ones(torch_cuda):
    """logits and old_logits 4-byte but not 16-byte aligned: the call reads an aligned copy of them (loss._aligned); adv, values and
    ret one float in are read where they lie.  The result is that of aligned clones, and no buffer changes, inside the view or
    outside it."""
    torch = torch_cuda
    from tiler_slider_amd import actor_critic_loss_grads
    kw, _ = _case_of((1, 1, 1, 1), True, 1285)
    t = _to(torch, kw)
    names = ("logits", "old_logits", "adv", "values", "ret")
    big, views = {}, {}
    for k in names:
        big[k] = torch.full((t[k].numel() + 9,), -7.25, dtype=torch.float32, device=t[k].device)
        views[k] = big[k][1:1 + t[k].numel()].view(t[k].shape)
        views[k].copy_(t[k])
        assert views[k].is_contiguous() and views[k].data_ptr() % 16 == 4
    before = {k: b.clone() for k, b in big.items()}
    rest = {k: x for k, x in t.items() if k not in names}
    act = rest.pop("act")
    call = lambda src: actor_critic_loss_grads(src["logits"], act, **{k: src[k] for k in names[1:]}, **rest)
    got, want = call(views), call({k: t[k].clone() for k in names})
    for a, b in zip(got[0] + got[1:], want[0] + want[1:]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(got[0].count) > 1000 and bool(got[1].any()) and bool(got[2].any())
    for k in names:
        assert torch.equal(big[k].view(torch.int32), before[k].view(torch.int32)), k


def test_fifty_steps_on_the_experts_labels_lower_the_cross_entropy(torch_cuda):
    """The shared-trunk actor-critic step with labels=: 256 solvable 4x4 levels, H = 32, Adam at 1e-2, 50 iterations of
    rollout_policy -> trajectory_labels -> trajectory_loss(labels=...) -> backward.  The cross-entropy after the 50 steps is
    below that at step 0; the curve is printed."""
    torch = torch_cuda
    from tiler_slider_amd import ActorCriticNet, TilerSliderEnvFactory
    dev = torch.device("cuda", 0)
    seeds = TilerSliderEnvFactory.solvable_seeds(256, size=4, num_tiles=2, num_obstacles=2, device=dev)
    env = TilerSliderEnvFactory.create_vec_env_from_seeds(seeds, size=4, num_tiles=2, num_obstacles=2, device=dev, max_steps=16, auto_reset=True,
                                                          obs_dtype=None)
    env.reset()
    table = env.build_table()
    net = ActorCriticNet(env.onehot_channels * 16, 32, dev, generator=torch.Generator(device=dev).manual_seed(0))
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    losses = []
    for it in range(51):
        out = env.rollout_policy(32, net.policy(), select="sample", seed=it, log=("start", "pos"))
        _, _, action = env.trajectory_labels(out, table)
        logits, _ = env.trajectory_outputs(net, out)
        info = env.trajectory_loss(logits, out, labels=action)
        losses.append(info.loss.detach())
        if it < 50:
            opt.zero_grad()
            info.loss.backward()
            opt.step()
    losses = [float(x) for x in losses]
    print("cross-entropy:", [round(x, 3) for x in losses])
    assert losses[-1] < losses[0]
    env.close()
