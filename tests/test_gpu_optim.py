"""The fused optimiser on the GPU (lib/libtiler_slider_optim.so) against the float64 yardstick of tests/optim_reference.py: one
step through the raw C-ABI into guarded memory in both launch forms, beyond the grid, the exact case bit for bit, non-finite
gradients, determinism, twenty steps through FusedAdam, torch's own AdamW on the device, the wrapper's rules, a captured graph,
and fifty iterations of the actor-critic recipe end to end."""
import ctypes as C
import functools

import numpy as np
import pytest

import optim_reference as ref

pytestmark = pytest.mark.gpu

GUARD = 256
AC_SHAPES = ((80, 32), (32,), (32, 4), (4,), (32,), (1,))
FORMS = ("one", "multi")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


@pytest.fixture
def form():
    """form("one") / form("multi"): the knob set so that any size here takes that form; restored after the test."""
    from tiler_slider_amd import _optim_cabi as oc
    was = oc.tuning(oc.TUNE_ONE_BLOCK_MAX)
    yield lambda name: oc.tuning(oc.TUNE_ONE_BLOCK_MAX, {"one": 1 << 40, "multi": 0}[name])
    oc.tuning(oc.TUNE_ONE_BLOCK_MAX, was)


class Arena:
    """Arrays in one device buffer, each between GUARD bytes of 0xA5 (and the padding to the next multiple of 256): the image is
    built on the host, uploaded, and compared byte for byte after the call outside what the call may write."""

    def __init__(self):
        self.items, self.size = {}, 0

    def add(self, name, array, shift=0):
        a = np.ascontiguousarray(array)
        off = self.size + GUARD + shift
        self.items[name] = (off, a)
        self.size = -(-(off + a.nbytes + GUARD) // 256) * 256

    def upload(self, torch):
        self.image = np.full(self.size, 0xA5, np.uint8)
        for off, a in self.items.values():
            self.image[off:off + a.nbytes] = a.view(np.uint8).reshape(-1)
        self.dev = torch.from_numpy(self.image).to(torch.device("cuda", 0))
        assert self.dev.data_ptr() % 256 == 0
        return self

    def ptr(self, name):
        return self.dev.data_ptr() + self.items[name][0]

    def download(self):
        self.after = self.dev.cpu().numpy()

    def get(self, name):
        off, a = self.items[name]
        return self.after[off:off + a.nbytes].view(a.dtype).reshape(a.shape).copy()

    def unchanged_outside(self, written):
        keep = np.ones(self.size, bool)
        for name in written:
            off, a = self.items[name]
            keep[off:off + a.nbytes] = False
        return bool((self.after[keep] == self.image[keep]).all())


def raw_step(torch, p, g, m, v, counters, cfg, *, zero_grad=False, lr_dev=False, norm_out=True, skip=False, shifted=()):
    """One ts_adam_step on arrays in guarded memory: (arena after the call, names the call may have written)."""
    from tiler_slider_amd import _optim_cabi as oc
    n = len(p)
    arena = Arena()
    for i in range(n):
        for name, a in (("p", p[i]), ("g", g[i]), ("m", m[i]), ("v", v[i])):
            arena.add(f"{name}{i}", a, shift=4 if (i in shifted and name in "pg") else 0)
    arena.add("counters", np.asarray(counters, np.int64))
    arena.add("grad_norm", np.array([123.0], np.float32))
    arena.add("lr", np.array([cfg["lr"]], np.float32))
    arena.add("workspace", np.zeros(oc.workspace_bytes(1), np.uint8))
    arena.upload(torch)
    t = oc.OptimTensors(n_tensors=n)
    for i in range(n):
        t.numel[i] = p[i].size
        t.param[i], t.grad[i], t.m[i], t.v[i] = (arena.ptr(f"{k}{i}") for k in "pgmv")
    c = oc.AdamCfg(cfg.get("beta1", 0.9), cfg.get("beta2", 0.999), arena.ptr("lr") if lr_dev else None, 5.0 if lr_dev else cfg["lr"], cfg.get("eps", 1e-8),
                   cfg.get("weight_decay", 0.0), cfg.get("max_grad_norm", 0.0) or 0.0, int(skip), int(zero_grad))
    o = oc.OptimOut(arena.ptr("counters"), arena.ptr("grad_norm") if norm_out else None, arena.ptr("workspace"))
    stream = torch.cuda.current_stream().cuda_stream
    oc.check(oc.lib().ts_adam_step(C.byref(t), C.byref(c), C.byref(o), stream), "ts_adam_step")
    torch.cuda.synchronize()
    arena.download()
    written = [f"{k}{i}" for i in range(n) for k in ("pmvg" if zero_grad else "pmv")] + ["counters", "workspace"] + (["grad_norm"] if norm_out else [])
    return arena, written


def lists(arena, n):
    return tuple([arena.get(f"{k}{i}") for i in range(n)] for k in "pgmv")


# ------------------------------------------------------------------------------------------------------------ 1. one step
TENSOR_LISTS = {
    "1": (1,),
    "3,4,5": (3, 4, 5),
    "255,256,257": (255, 256, 257),
    "1023,1,1025": (1023, 1, 1025),
    "32-tiny": (1, 3, 5, 7) * 8,
    "empty-in-the-middle": (300, 0, 41),
    "view-4-bytes-past-16": (300, 41, 7),
}
OPTIONS = {
    "no-clip": dict(clip=None, wd=0.0, zero=False, lr_dev=False, norm_out=True, skip=True),
    "clip-active": dict(clip=1 / 3, wd=0.01, zero=True, lr_dev=True, norm_out=True, skip=True),
    "clip-inactive": dict(clip=2.0, wd=0.01, zero=False, lr_dev=True, norm_out=True, skip=False),
    "apply-alone": dict(clip=None, wd=0.0, zero=True, lr_dev=False, norm_out=False, skip=False),
    "clip-active-norm-not-wanted": dict(clip=1 / 3, wd=0.0, zero=False, lr_dev=False, norm_out=False, skip=False),
}


@functools.lru_cache(maxsize=None)
def _one_step_case(list_id, t, option):
    """Inputs and the yardstick's answer, computed once and shared by both forms (never written to)."""
    shapes, o = TENSOR_LISTS[list_id], OPTIONS[option]
    seed = 100 * sorted(TENSOR_LISTS).index(list_id) + t % 7
    g = ref.gradients(shapes, seed)
    p, m, v = ref.state(shapes, seed, t)
    gn = float(np.sqrt(sum(float((a.astype(np.float64) ** 2).sum()) for a in g)))
    cfg = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=o["wd"], max_grad_norm=ref.f32(gn * o["clip"]) if o["clip"] else 0.0)
    return p, g, m, v, cfg, ref.adam64(p, g, m, v, t, **cfg)


def _check_step(arena, written, n, inputs, want, counters, *, zero_grad, norm_out):
    p0, g0, m0, v0 = inputs
    P, G, M, V = lists(arena, n)
    assert arena.unchanged_outside(written), "a guard, or an array the call does not write, changed"
    units = (ref.worst(P, want.p, want.Mp), ref.worst(M, want.m, want.Mm), ref.worst(V, want.v, want.Mv))
    assert ref.within(P, want.p, want.Mp) and ref.within(M, want.m, want.Mm) and ref.within(V, want.v, want.Mv), units
    for a, b in zip(G, g0):
        assert not a.any() if zero_grad else np.array_equal(a, b)
    assert arena.get("counters").tolist() == [counters[0] + 1, counters[1]]
    if norm_out:
        assert abs(float(arena.get("grad_norm")[0]) - float(np.float32(want.gn))) <= 2.0 ** -23 * want.gn
    return units


@pytest.mark.parametrize("which", FORMS)
@pytest.mark.parametrize("list_id", TENSOR_LISTS)
def test_one_step_into_guarded_memory_lies_inside_the_bounds(torch_cuda, form, list_id, which):
    from tiler_slider_amd import _optim_cabi as oc
    form(which)
    shapes = TENSOR_LISTS[list_id]
    worst = (0.0, 0.0, 0.0)
    for t in (0, 1, 1000):
        for option, o in OPTIONS.items():
            p, g, m, v, cfg, want = _one_step_case(list_id, t, option)
            norm = bool(o["clip"] or o["skip"] or o["norm_out"])
            d = oc.describe_adam_step(shapes, oc.NORM if norm else 0)
            assert d["form"] == (oc.FORM_ONE if which == "one" else oc.FORM_MULTI if norm else oc.FORM_APPLY), (d, option)
            assert (want.c < 1.0) == (option.startswith("clip-active")) and not want.skipped
            arena, written = raw_step(torch_cuda, p, g, m, v, (t, 3), cfg, zero_grad=o["zero"], lr_dev=o["lr_dev"], norm_out=o["norm_out"], skip=o["skip"],
                                      shifted=(1,) if list_id.startswith("view") else ())
            units = _check_step(arena, written, len(shapes), (p, g, m, v), want, (t, 3), zero_grad=o["zero"], norm_out=o["norm_out"])
            worst = tuple(max(a, b) for a, b in zip(worst, units))
    print(f"{list_id} {which}: worst deviation of p, m, v in units of 2^-24 M: {[round(x, 2) for x in worst]}")


# ------------------------------------------------------------------------------------------------------ 2. beyond the grid
BIG = (1024 * 1024 + 259, 5)      # TS_OPTIM_MAX_BLOCKS x TS_OPTIM_CHUNK + 259: every block strides twice, with a ragged end


@functools.lru_cache(maxsize=None)
def _big_case():
    from tiler_slider_amd import _optim_cabi as oc
    assert BIG[0] == oc.MAX_BLOCKS * oc.CHUNK + 259
    g = ref.gradients(BIG, 77)
    p, m, v = ref.state(BIG, 77, 1)
    gn = float(np.sqrt(sum(float((a.astype(np.float64) ** 2).sum()) for a in g)))
    cfg = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=ref.f32(gn / 3))
    return p, g, m, v, cfg, ref.adam64(p, g, m, v, 1, **cfg)


def test_beyond_the_grid_the_multi_block_form_lies_inside_the_bounds(torch_cuda, form):
    from tiler_slider_amd import _optim_cabi as oc
    form("multi")
    d = oc.describe_adam_step(BIG)
    assert d["blocks"] == oc.MAX_BLOCKS and d["chunks"] == oc.MAX_BLOCKS + 2 and d["form"] == oc.FORM_MULTI
    p, g, m, v, cfg, want = _big_case()
    arena, written = raw_step(torch_cuda, p, g, m, v, (1, 0), cfg, zero_grad=True, lr_dev=True, skip=True)
    print("beyond the grid:", _check_step(arena, written, 2, (p, g, m, v), want, (1, 0), zero_grad=True, norm_out=True))


# ------------------------------------------------------------------------------------------------------- 3. the exact case
@pytest.mark.parametrize("which", FORMS)
@pytest.mark.parametrize("one", (False, True), ids=("powers-of-two", "unit"))
def test_the_exact_case_holds_bit_for_bit(torch_cuda, form, which, one):
    form(which)
    cfg, p, g, want_p, want_m, want_v = ref.exact_case(one)
    z = [np.zeros_like(a) for a in p]
    arena, written = raw_step(torch_cuda, p, g, z, z, (0, 0), cfg, skip=True)
    P, G, M, V = lists(arena, 2)
    for i in range(2):
        assert np.array_equal(P[i], want_p[i]) and np.array_equal(M[i], want_m[i]) and np.array_equal(V[i], want_v[i]) and np.array_equal(G[i], g[i])
    assert arena.get("counters").tolist() == [1, 0] and arena.unchanged_outside(written)
    if one:
        assert float(arena.get("grad_norm")[0]) == 32.0


# --------------------------------------------------------------------------------------------------------- 4. non-finite
NF_SHAPES = (300, 41, 7)


def _nonfinite(kind):
    g = ref.gradients(NF_SHAPES, 9)
    g[0][1] = np.float32(1e30)
    if kind in ("nan", "both"):
        g[-1][-1] = np.nan
    if kind in ("inf", "both"):
        g[0][0] = np.inf
    p, m, v = ref.state(NF_SHAPES, 9, 1)
    return p, g, m, v


@pytest.mark.parametrize("which", FORMS)
@pytest.mark.parametrize("zero", (False, True), ids=("keep-grads", "zero-grads"))
@pytest.mark.parametrize("kind", ("nan", "inf", "both"))
def test_a_nonfinite_norm_skips_the_step_on_the_device(torch_cuda, form, kind, zero, which):
    form(which)
    p, g, m, v = _nonfinite(kind)
    cfg = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=1.0)
    arena, _ = raw_step(torch_cuda, p, g, m, v, (17, 5), cfg, zero_grad=zero, skip=True)
    # p, m and v byte for byte, and every guard: only the counters, the norm, the workspace and - with zero_grad - the gradients
    assert arena.unchanged_outside(["counters", "grad_norm", "workspace"] + ([f"g{i}" for i in range(3)] if zero else []))
    assert arena.get("counters").tolist() == [17, 6] and not np.isfinite(arena.get("grad_norm")[0])
    if zero:
        assert not any(arena.get(f"g{i}").view(np.uint32).any() for i in range(3))
    # without skip_nonfinite the call applies: counters say so, and nothing outside its arrays is touched
    arena, written = raw_step(torch_cuda, p, g, m, v, (17, 5), cfg, zero_grad=zero, skip=False)
    assert arena.unchanged_outside(written) and arena.get("counters").tolist() == [18, 5] and not np.isfinite(arena.get("grad_norm")[0])


@pytest.mark.parametrize("which", FORMS)
def test_a_gradient_of_1e30_is_finite_and_does_not_skip(torch_cuda, form, which):
    """A float32 sum of squares would overflow; the float64 one gives the norm, the clip scales by 1e-30, and the step is the yardstick's."""
    form(which)
    p, g, m, v = _nonfinite("none")
    cfg = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=1.0)
    want = ref.adam64(p, g, m, v, 1, **cfg)
    assert 1e30 <= want.gn < 1.0001e30 and not want.skipped
    arena, written = raw_step(torch_cuda, p, g, m, v, (1, 0), cfg, skip=True)
    _check_step(arena, written, 3, (p, g, m, v), want, (1, 0), zero_grad=False, norm_out=True)


# -------------------------------------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("which", FORMS + ("big",))
def test_two_identical_calls_agree_bit_for_bit(torch_cuda, form, which):
    form("multi" if which == "big" else which)
    if which == "big":
        p, g, m, v, cfg, _ = _big_case()
    else:
        p, g, m, v, cfg, _ = _one_step_case("1023,1,1025", 1000, "clip-active")
    runs = []
    for _ in range(2):
        arena, _ = raw_step(torch_cuda, p, g, m, v, (1, 0), cfg, zero_grad=True, skip=True)
        runs.append(arena)
    for name in list(runs[0].items):
        if name != "workspace":
            assert np.array_equal(runs[0].get(name).view(np.uint8), runs[1].get(name).view(np.uint8)), name


# ------------------------------------------------------------------------------------------------- 6. twenty steps, FusedAdam
def test_twenty_steps_through_fused_adam_stay_within_four_times_torchs_cpu_float32(torch_cuda):
    """The GPU's bound is measured against the reference, never against the code under test: the same 20 steps through torch's
    CPU float32 AdamW + clip_grad_norm_ deviate from the float64 yardstick by at most D units of 2^-24 (|p| + lr t); the GPU
    gets 4 D (another rounding sequence, errors adding like a random walk; a real defect is off by thousands of units)."""
    torch = torch_cuda
    from tiler_slider_amd import FusedAdam
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(6)
    cfg = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, max_grad_norm=0.5)
    p0 = [rng.standard_normal(s).astype(np.float32) for s in AC_SHAPES]
    grads = [[(rng.standard_normal(s) * (3.0 if t % 2 == 0 else 0.01)).astype(np.float32) for s in AC_SHAPES] for t in range(20)]
    gpu = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in p0]
    cpu = [torch.from_numpy(a.copy()).requires_grad_(True) for a in p0]
    opt = FusedAdam(gpu, lr=cfg["lr"], weight_decay=cfg["weight_decay"], max_grad_norm=cfg["max_grad_norm"])
    topt = torch.optim.AdamW(cpu, lr=cfg["lr"], weight_decay=cfg["weight_decay"])
    p, m, v = p0, [np.zeros(s) for s in AC_SHAPES], [np.zeros(s) for s in AC_SHAPES]
    D = G = 0.0
    clipped = []
    for t in range(20):
        for q, c, a in zip(gpu, cpu, grads[t]):
            q.grad, c.grad = torch.from_numpy(a).to(dev), torch.from_numpy(a.copy())
        torch.nn.utils.clip_grad_norm_(cpu, cfg["max_grad_norm"])
        topt.step()
        opt.step()
        st = ref.adam64(p, grads[t], m, v, t, **cfg)
        clipped.append(st.c < 1.0)
        assert abs(float(opt.grad_norm) - st.gn) <= 2.0 ** -23 * st.gn
        p, m, v = st.p, st.m, st.v
        scale = [np.abs(a) + cfg["lr"] * (t + 1) for a in p]
        D = max(D, ref.worst([c.detach().numpy() for c in cpu], p, scale))
        G = max(G, ref.worst([q.detach().cpu().numpy() for q in gpu], p, scale))
    print(f"twenty steps: torch CPU float32 D = {D:.2f}, the GPU {G:.2f} units of 2^-24 (|p| + lr t)")
    assert clipped[0] and int(opt.steps_applied) == 20 and int(opt.steps_skipped) == 0      # (0.01 x sqrt(2757) is 0.525: the small steps clip too, barely)
    assert 1.0 < D < 100.0 and G <= 4 * D


# ------------------------------------------------------------------------------------------------ 7. torch on the device
def test_one_step_of_torchs_adamw_on_the_device_lies_inside_the_same_bounds(torch_cuda):
    torch = torch_cuda
    from tiler_slider_amd import FusedAdam
    dev = torch.device("cuda", 0)
    shapes = [int(np.prod(s)) for s in AC_SHAPES]
    g = ref.gradients(shapes, 12)
    p, m, v = ref.state(shapes, 12, 0)
    cfg = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=0.5)
    want = ref.adam64(p, g, m, v, 0, **cfg)
    assert want.c < 1.0
    ours = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in p]
    theirs = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in p]
    for a, b, gi in zip(ours, theirs, g):
        a.grad, b.grad = torch.from_numpy(gi).to(dev), torch.from_numpy(gi).to(dev)
    opt = FusedAdam(ours, **cfg)
    opt.step()
    torch.nn.utils.clip_grad_norm_(theirs, cfg["max_grad_norm"])
    topt = torch.optim.AdamW(theirs, lr=cfg["lr"], weight_decay=cfg["weight_decay"])
    topt.step()
    for params, o, keys in ((ours, opt, ("exp_avg", "exp_avg_sq")), (theirs, topt, ("exp_avg", "exp_avg_sq"))):
        assert ref.within([q.detach().cpu().numpy() for q in params], want.p, want.Mp)
        assert ref.within([o.state[q][keys[0]].cpu().numpy() for q in params], want.m, want.Mm)
        assert ref.within([o.state[q][keys[1]].cpu().numpy() for q in params], want.v, want.Mv)


# ------------------------------------------------------------------------------------------------------------ 8. the wrapper
def _params(torch, shapes, seed=0, grads=True):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(seed)
    ps = [torch.randn(s, device=dev, generator=gen).requires_grad_(True) for s in shapes]
    if grads:
        for q in ps:
            q.grad = torch.randn(q.shape, device=dev, generator=gen)
    return ps


def test_the_wrapper_refuses_what_the_call_cannot_take(torch_cuda):
    torch = torch_cuda
    from tiler_slider_amd import FusedAdam
    dev = torch.device("cuda", 0)
    with pytest.raises(ValueError):
        FusedAdam([torch.zeros(3, dtype=torch.float64, device=dev, requires_grad=True)])
    with pytest.raises(ValueError):
        FusedAdam([torch.zeros(4, 6, device=dev).t().requires_grad_(True)])
    with pytest.raises(ValueError):
        FusedAdam([torch.zeros(3, requires_grad=True)])
    a, b = _params(torch, ((3,), (4,)))
    with pytest.raises(ValueError):
        FusedAdam([{"params": [a]}, {"params": [b], "lr": 1e-3}])
    many = _params(torch, ((2,),) * 33)
    opt = FusedAdam(many)
    with pytest.raises(ValueError):
        opt.step()
    many[0].grad = None     # 32 with a gradient: fine
    opt.step()
    assert int(opt.steps_applied) == 1
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [torch.zeros(2, device=dev, requires_grad=True)]})
    for kw in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(eps=-1.0), dict(weight_decay=-1.0), dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            FusedAdam([a], **kw)


def test_a_parameter_without_a_gradient_sits_out_and_nothing_in_step_reads_the_device(torch_cuda, monkeypatch):
    torch = torch_cuda
    from tiler_slider_amd import FusedAdam
    ps = _params(torch, AC_SHAPES)
    ps[2].grad = None
    before = [q.detach().clone() for q in ps]
    opt = FusedAdam(ps, lr=1e-2, max_grad_norm=1.0)
    for t in (opt.grad_norm, opt.steps_applied, opt.steps_skipped):
        assert t.is_cuda and t.dim() == 0
    assert opt.steps_applied.dtype == opt.steps_skipped.dtype == torch.int64 and opt.grad_norm.dtype == torch.float32

    def no_item(self):
        raise AssertionError("step() read a device scalar")
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "item", no_item)
        opt.step(zero_grad=True)
    assert torch.equal(ps[2], before[2]) and ps[2] not in opt.state and ps[2].grad is None
    for i in (0, 1, 3, 4, 5):
        assert not torch.equal(ps[i], before[i]) and not ps[i].grad.any() and set(opt.state[ps[i]]) == {"exp_avg", "exp_avg_sq"}
    assert int(opt.steps_applied) == 1 and int(opt.steps_skipped) == 0
    assert float(opt.grad_norm) > 0
    # a NaN gradient: the step is skipped on the device, and the view says so
    for q in ps:
        if q.grad is not None:
            q.grad.normal_()
    ps[0].grad[3, 3] = float("nan")
    held = [q.detach().clone() for q in ps]
    opt.step()
    assert all(torch.equal(a, b) for a, b in zip(ps, held)) and int(opt.steps_applied) == 1 and int(opt.steps_skipped) == 1
    # no parameter has a gradient: nothing is launched, the counters stay, and the norm of nothing is 0 (the call's one memset)
    assert not np.isfinite(float(opt.grad_norm))
    for q in ps:
        q.grad = None
    opt.step(zero_grad=True)
    assert float(opt.grad_norm) == 0.0 and int(opt.steps_applied) == 1 and int(opt.steps_skipped) == 1
    assert all(torch.equal(a, b) for a, b in zip(ps, held))


def test_an_lr_tensor_is_read_by_the_launch(torch_cuda):
    torch = torch_cuda
    from tiler_slider_amd import FusedAdam
    dev = torch.device("cuda", 0)
    results = []
    for lr_tensor in (True, False):
        ps = _params(torch, AC_SHAPES, seed=3)
        lr = torch.tensor(1e-2, device=dev) if lr_tensor else 1e-2
        opt = FusedAdam(ps, lr=lr)
        opt.step()
        if lr_tensor:
            lr.fill_(2.5e-3)      # in place: the next launch reads it
        else:
            opt.param_groups[0]["lr"] = 2.5e-3
        opt.step()
        results.append([q.detach().clone() for q in ps])
    assert all(torch.equal(a, b) for a, b in zip(*results))
    ps = _params(torch, AC_SHAPES, seed=3)
    other = FusedAdam(ps, lr=1e-2)
    other.step(), other.step()
    assert not all(torch.equal(a, b) for a, b in zip(ps, results[0]))


def test_state_dict_round_trips_to_the_same_bits(torch_cuda):
    torch = torch_cuda
    from tiler_slider_amd import FusedAdam
    kw = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=0.5)
    ps = _params(torch, AC_SHAPES, seed=4)
    opt = FusedAdam(ps, **kw)
    for _ in range(3):
        opt.step()
    sd = opt.state_dict()
    assert sd["fused_adam"]["counters"].tolist() == [3, 0] and len(sd["state"]) == 6
    copies = [q.detach().clone().requires_grad_(True) for q in ps]
    fresh = FusedAdam(copies, lr=1.0)
    fresh.load_state_dict(sd)
    assert fresh.param_groups[0]["lr"] == 1e-2 and int(fresh.steps_applied) == 3
    gen = torch.Generator(device=ps[0].device).manual_seed(99)
    for a, b in zip(ps, copies):
        a.grad = torch.randn(a.shape, device=a.device, generator=gen)
        b.grad = a.grad.clone()
    opt.step(), fresh.step()
    for a, b in zip(ps, copies):
        assert torch.equal(a, b) and torch.equal(opt.state[a]["exp_avg"], fresh.state[b]["exp_avg"])
        assert torch.equal(opt.state[a]["exp_avg_sq"], fresh.state[b]["exp_avg_sq"])
    assert int(fresh.steps_applied) == 4 and torch.equal(fresh.grad_norm, opt.grad_norm)


# ---------------------------------------------------------------------------------------------------------- 9. graph replay
def test_three_replays_of_a_captured_step_are_three_eager_steps(torch_cuda):
    """Captured the way capture_steps captures - a side stream, one linear chain - with lr a tensor and the gradients in fixed
    buffers that are refilled between replays.  The bias correction comes from the device counter, so every replay is the next
    step."""
    torch = torch_cuda
    from tiler_slider_amd import FusedAdam
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(8)
    feeds = [[torch.randn(s, device=dev, generator=gen) for s in AC_SHAPES] for _ in range(3)]
    lrs = (1e-2, 5e-3, 2.5e-3)
    finals = []
    for captured in (False, True):
        ps = _params(torch, AC_SHAPES, seed=5, grads=False)
        for q in ps:
            q.grad = torch.zeros_like(q)
        lr = torch.tensor(lrs[0], device=dev)
        opt = FusedAdam(ps, lr=lr, weight_decay=0.01, max_grad_norm=0.5)
        opt.init_state()      # the moments exist before the capture: nothing is allocated inside it
        graph = None
        if captured:
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream(dev)
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):
                    opt.step(zero_grad=True)
            assert int(opt.steps_applied) == 0      # a capture runs nothing
        for k in range(3):
            lr.fill_(lrs[k])
            for q, f in zip(ps, feeds[k]):
                q.grad.copy_(f)
            graph.replay() if captured else opt.step(zero_grad=True)
        torch.cuda.synchronize(dev)
        assert int(opt.steps_applied) == 3 and int(opt.steps_skipped) == 0 and not any(bool(q.grad.any()) for q in ps)
        finals.append([q.detach().clone() for q in ps] + [opt.state[q]["exp_avg"].clone() for q in ps] + [opt.state[q]["exp_avg_sq"].clone() for q in ps]
                      + [opt.grad_norm.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*finals))


# ------------------------------------------------------------------------------------------------------------ 10. end to end
def test_fifty_iterations_of_the_actor_critic_recipe_driven_by_fused_adam(torch_cuda):
    """256 solvable 4x4 levels, ActorCriticNet H = 32, the expert's labels as a cross-entropy plus the value term through
    trajectory_loss, FusedAdam(lr=1e-2, max_grad_norm=1.0), 50 iterations.  Both loss terms end below where they started, the
    next rollout plays the updated weights, no step was skipped; and the recorded gradients fed to a second FusedAdam over a copy
    of the starting weights give the same final bits (the backward's float atomics are not this optimiser's business)."""
    torch = torch_cuda
    from tiler_slider_amd import ActorCriticNet, FusedAdam, RewardWeights, TilerSliderEnvFactory
    dev = torch.device("cuda", 0)
    seeds = TilerSliderEnvFactory.solvable_seeds(256, size=4, num_tiles=2, num_obstacles=2, device=dev)
    env = TilerSliderEnvFactory.create_vec_env_from_seeds(seeds, size=4, num_tiles=2, num_obstacles=2, device=dev, max_steps=16, auto_reset=True,
                                                          obs_dtype=None)
    env.reset()
    table = env.build_table()
    net = ActorCriticNet(env.onehot_channels * 16, 32, dev, generator=torch.Generator(device=dev).manual_seed(0))
    params = list(net.parameters())
    start = [q.detach().clone() for q in params]
    opt = FusedAdam(params, lr=1e-2, max_grad_norm=1.0)
    policy_losses, value_losses, recorded = [], [], []
    for it in range(51):
        out = env.rollout_policy(32, net.policy(), select="sample", seed=it, log=("start", "pos", "flags"))
        _, _, action = env.trajectory_labels(out, table)
        logits, values = env.trajectory_outputs(net, out)
        # the value target: the discounted cost of the steps left in the episode.  A better policy only shortens episodes, so the
        # target does not run away from the critic while the actor learns (the return of wins does: it grows with the policy)
        tr = env.trajectory_returns(out, gamma=0.97, reward=RewardWeights(step=-0.05, win=0.0))
        tr = tr._replace(adv=torch.ones_like(tr.adv))      # labels with advantage 1: a cross-entropy over the steps that played
        info = env.trajectory_loss(logits, out, tr, values=values, labels=action)
        policy_losses.append(info.policy.detach())
        value_losses.append(info.value.detach())
        if it < 50:
            opt.zero_grad(set_to_none=False)
            info.loss.backward()
            recorded.append([q.grad.clone() for q in params])
            opt.step()
    policy_losses, value_losses = [float(x) for x in policy_losses], [float(x) for x in value_losses]
    print("cross-entropy:", [round(x, 3) for x in policy_losses[::10]], "value:", [round(x, 4) for x in value_losses[::10]])
    assert policy_losses[-1] < policy_losses[0] and value_losses[-1] < value_losses[0]
    assert int(opt.steps_applied) == 50 and int(opt.steps_skipped) == 0
    # the next rollout plays the updated weights: its logged logits are the network's as it stands now, not as it started
    out = env.rollout_policy(2, net.policy(), select="greedy", seed=99, log=("start", "pos", "logits"))
    now, _ = env.trajectory_outputs(net, out)
    assert torch.equal(now.detach(), out.logits_log)
    with torch.no_grad():
        for q, a in zip(params, start):
            q_now = q.detach().clone()
            q.copy_(a)
            a.copy_(q_now)      # `start` now holds the trained weights, the network the starting ones
    was, _ = env.trajectory_outputs(net, out)
    assert not torch.equal(was.detach(), out.logits_log)
    # the optimiser's side is reproducible: the same gradients, the same bits
    again = FusedAdam(params, lr=1e-2, max_grad_norm=1.0)
    for grads in recorded:
        for q, gq in zip(params, grads):
            q.grad = gq
        again.step()
    assert all(torch.equal(q.detach(), a) for q, a in zip(params, start)) and int(again.steps_applied) == 50
    env.close()
