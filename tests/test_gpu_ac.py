"""The actor-critic network on the GPU (lib/libtiler_slider_ac.so, VecTilerSliderEnv.trajectory_outputs, ActorCriticNet) against
the CPU yardstick tests/ac_reference.py - the definition of include/tiler_slider_ac.h on NumPy -, against the rollout's own logged
logits, and against the training library's backward on the same inputs."""
import ctypes as C

import numpy as np
import pytest

import ac_reference as ar
import policy_reference as pref
import rollout_reference as rref
import train_reference as tr
from table_harness import GUARD, guarded as _guarded, payload as _payload

pytestmark = pytest.mark.gpu

STRICT, AUTORESET = 0, 1
NAMES = ar.NAMES


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _env(S, mc, blk, init, tgt, max_steps=100, mode=AUTORESET, **kw):
    from tiler_slider_amd import VecTilerSliderEnv
    kw.setdefault("obs_dtype", None)
    env = VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=mc, max_steps=max_steps, auto_reset=mode == AUTORESET, **kw)
    env.reset()
    return env


def _put(env, name, a):
    torch = __import__("torch")
    t = getattr(env, name)
    assert tuple(t.shape) == a.shape, (name, t.shape, a.shape)
    if a.size:
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(t.device))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _params(net):
    return net.w1, net.b1, net.w2, net.b2, net.wv, net.bv


def _net(torch, env, mlp, head, requires_grad=True):
    """An ActorCriticNet holding `mlp` (torch.nn.Linear's layout, as the yardsticks keep it) and `head`."""
    from tiler_slider_amd import ActorCriticNet
    H, D = mlp[0].shape
    net = ActorCriticNet(D, H, env.device)
    with torch.no_grad():
        for p, a in zip(_params(net), ar.kernel_layout(mlp, head)):
            p.copy_(torch.from_numpy(a))
    for p in net.parameters():
        p.requires_grad_(requires_grad)
    return net


def _given(torch, env, first, pos_log):
    """A Rollout that holds given cells: what rollout_policy(..., log=("start", "pos")) returns, with cells of our choosing."""
    from tiler_slider_amd import Rollout
    dev = env.device
    return Rollout(pos_log.shape[0], start_pos=torch.from_numpy(first).to(dev), pos_log=torch.from_numpy(pos_log).to(dev))


def _raw_backward(torch, env, kl, first, pos_log, K, dz, dv, grads):
    """ts_ac_backward itself: kl (six), first, pos_log, dz, dv, grads (six) are device tensors (pos_log may be None)."""
    from tiler_slider_amd import _ac_cabi as ac
    mlp = ac.Mlp(*(t.data_ptr() for t in kl[:4]), kl[0].shape[1], 0)
    head = ac.ValueHead(kl[4].data_ptr(), kl[5].data_ptr())
    tin = ac.TrainIn(first.data_ptr() if first.numel() else None, pos_log.data_ptr() if pos_log is not None and pos_log.numel() else None, K, 0)
    grad = ac.MlpGrad(*(g.data_ptr() for g in grads[:4]))
    hgrad = ac.ValueHeadGrad(grads[4].data_ptr(), grads[5].data_ptr())
    return ac.lib().ts_ac_backward(C.byref(env._dims), C.byref(env._state), C.byref(mlp), C.byref(head), C.byref(tin), dz.data_ptr(),
                                   dv.data_ptr(), C.byref(grad), C.byref(hgrad), torch.cuda.current_stream(env.device).cuda_stream)


def _raw_train_backward(torch, env, kl, first, pos_log, K, dz, grads):
    """ts_train_backward of the training library on the same inputs: four parameters, four gradients."""
    from tiler_slider_amd import _train_cabi as tc
    mlp = tc.Mlp(*(t.data_ptr() for t in kl[:4]), kl[0].shape[1], 0)
    tin = tc.TrainIn(first.data_ptr() if first.numel() else None, pos_log.data_ptr() if pos_log is not None and pos_log.numel() else None, K, 0)
    grad = tc.MlpGrad(*(g.data_ptr() for g in grads[:4]))
    return tc.lib().ts_train_backward(C.byref(env._dims), C.byref(env._state), C.byref(mlp), C.byref(tin), dz.data_ptr(), C.byref(grad),
                                      torch.cuda.current_stream(env.device).cuda_stream)


# ---------------------------------------------------------------------------------------------- 1. the forward
@pytest.mark.parametrize("K", (1, 2, 5))
@pytest.mark.parametrize("mode", (STRICT, AUTORESET))
def test_logits_equal_the_rollouts_own_bit_for_bit_and_values_lie_within_their_bound(torch_cuda, oracle, mode, K):
    """257 boards four random steps into their episodes, a quarter of the steps explored, GAUSSIAN weights (every rounding
    counts) and an arbitrary non-zero value head: the logits of the logged trajectory are the rollout's logits_log bit for bit -
    the head does not disturb z - and the training library's; every value within the yardstick's per-value bound of float64."""
    torch = torch_cuda
    S, T, Ko, mc, n, max_steps, H = 4, 2, 2, False, 257, 6, 16
    blk, init, tgt = oracle.generate_mt19937(S, T, T, Ko, np.arange(n, dtype=np.uint32))
    rng = np.random.default_rng(40 + K)
    mlp = pref.random_mlp(rng, tr.features(S, T, T, mc), H)
    head = ar.random_head(rng, H)
    assert np.abs(head[0]).min() > 0 and head[1][0] != 0
    start = rref.rollout(oracle, S, mc, max_steps, blk, init, tgt, 4, rref.RANDOM, mode, seed=1)
    env = _env(S, mc, blk, init, tgt, max_steps, mode)
    for name in ("pos", "step_count", "done"):
        _put(env, "_" + name, start[name])
    net = _net(torch, env, mlp, head)
    now_z, now_v = env.trajectory_outputs(net)                   # the boards as they stand: K = 1
    assert tuple(now_z.shape) == (1, n, 4) and tuple(now_v.shape) == (1, n) and now_z.grad_fn is not None and now_v.grad_fn is not None
    assert torch.equal(now_z.detach()[0], env.policy_logits(net.policy()))
    out = env.rollout_policy(K, net.policy(), select="greedy", epsilon=0.25, seed=77, log=("start", "pos", "logits", "flags"))
    np.testing.assert_array_equal(out.start_pos.cpu().numpy(), start["pos"])
    if K == 5:
        flags = out.flags_log.cpu().numpy()
        assert ((flags & (rref.FLAG_AUTORESET if mode == AUTORESET else rref.FLAG_STEPPED_DONE)) != 0).any()
    z, v = env.trajectory_outputs(net, out)
    assert z.dtype == torch.float32 and tuple(z.shape) == (K, n, 4) and v.dtype == torch.float32 and tuple(v.shape) == (K, n)
    assert z.is_contiguous() and v.is_contiguous()
    np.testing.assert_array_equal(_bits(z.detach().cpu().numpy()), _bits(out.logits_log.cpu().numpy()))
    assert torch.equal(env.trajectory_logits(net.policy(), out), z.detach())       # the existing library on the same tensors
    first, pos_log = out.start_pos.cpu().numpy(), out.pos_log.cpu().numpy()
    x = tr.samples_onehot(S, mc, blk, first, pos_log, tgt, K)
    z64, zb, v64, vb = ar.outputs64(x, mlp, head)
    err = np.abs(v.detach().cpu().numpy().reshape(-1).astype(np.float64) - v64)
    print(f"mode {mode} K={K}: worst value error / bound {float((err / vb).max()):.3f}, median |v| {float(np.median(np.abs(v64))):.3f}")
    assert (err <= vb).all() and np.median(vb) < 0.01 * np.median(np.abs(v64))
    assert (np.abs(z.detach().cpu().numpy().reshape(-1, 4).astype(np.float64) - z64) <= zb).all()
    # another head: other values, the same logits
    with torch.no_grad():
        net.wv.mul_(-3.0)
        net.bv.add_(1.0)
    z2, v2 = env.trajectory_outputs(net, out)
    assert torch.equal(z2.detach(), z.detach()) and not torch.equal(v2.detach(), v.detach())
    env.close()


# ---------------------------------------------------------------------------------------------- 2. backward exactness
def _exact(torch, oracle, case, H, K):
    """One exact case through the raw call with prefilled buffers: all six gradients bit-equal to the yardstick; the forward on
    the same cells; and with dv = 0 the first four gradients bit-equal to ts_train_backward's on the same inputs."""
    from tiler_slider_amd import _ac_cabi as ac
    S, T, Tt, Ko, mc, what, _ = ar.BACKWARD_CASES[case]
    c = ar.backward_case(oracle, case, H, K)                       # asserts on the yardstick's own numbers that the case bites
    assert c["wv_grad"] and c["reaches"]
    n = c["first"].shape[1]
    env = _env(S, mc, c["blk"], np.zeros((T, n), np.uint8), c["tgt"])
    dev = env.device
    d = ac.describe_ac_backward(env._dims, H, K)
    kl = [torch.from_numpy(a).to(dev) for a in ar.kernel_layout(c["mlp"], c["head"])]
    first, pos_log = torch.from_numpy(c["first"]).to(dev), torch.from_numpy(c["pos_log"]).to(dev)
    log = pos_log if K > 1 else None
    dz, dv = torch.from_numpy(c["dz"]).to(dev), torch.from_numpy(c["dv"]).to(dev)
    grads = [torch.from_numpy(c["prefill"][k]).to(dev) for k in NAMES]
    assert _raw_backward(torch, env, kl, first, log, K, dz, dv, grads) == 0
    for name, g in zip(NAMES, grads):
        np.testing.assert_array_equal(_bits(g.cpu().numpy()), _bits(c["want"][name]), err_msg=f"case {case} {what} H={H} K={K}: {name}")
    assert torch.equal(grads[0][torch.from_numpy(c["untouched"]).to(dev)], torch.from_numpy(c["prefill"]["w1"][c["untouched"]]).to(dev))
    # dv = 0: the actor's four gradients are the training library's, the head's buffers keep their prefill
    mine = [torch.from_numpy(c["prefill"][k]).to(dev) for k in NAMES]
    theirs = [torch.from_numpy(c["prefill"][k]).to(dev) for k in NAMES[:4]]
    assert _raw_backward(torch, env, kl, first, log, K, dz, torch.zeros_like(dv), mine) == 0
    assert _raw_train_backward(torch, env, kl, first, log, K, dz, theirs) == 0
    for name, a, b in zip(NAMES, mine, theirs):
        np.testing.assert_array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()), err_msg=f"case {case} H={H} K={K}: {name} with dv = 0")
    np.testing.assert_array_equal(mine[4].cpu().numpy(), c["prefill"]["wv"])
    np.testing.assert_array_equal(mine[5].cpu().numpy(), c["prefill"]["bv"])
    assert any((a != b).any() for a, b in zip(mine[:2], grads[:2]))                 # and dv did matter above
    if T:
        z, v = env.trajectory_outputs(_net(torch, env, c["mlp"], c["head"], requires_grad=False), _given(torch, env, c["first"], c["pos_log"]))
        np.testing.assert_array_equal(_bits(z.cpu().numpy()), _bits(c["logits"]), err_msg=f"case {case} H={H} K={K}: logits")
        np.testing.assert_array_equal(_bits(v.cpu().numpy()), _bits(c["values"]), err_msg=f"case {case} H={H} K={K}: values")
    print(f"case {case} {what} H={H} K={K}: grads_in_lds {d['grads_in_lds']}, pre == 0 with dh != 0 {c['bites']:.3f}, shared cells {c['shared']:.3f}")
    env.close()
    return d


@pytest.mark.parametrize("case", range(len(ar.BACKWARD_CASES)))
def test_integer_gradients_equal_the_yardstick_bit_for_bit(torch_cuda, oracle, case):
    """train_reference.BACKWARD_CASES x H in {1, 7, 64} x K in {1, 2, 5} at 257 boards (more than four waves of boards and a
    ragged last one; K = 5 is one chunk plus a remainder), integer weights in [-2, 2], dz and dv in {-1, 0, 1}, cells drawn at
    random, the six buffers prefilled with integers in [-3, 3] (the call adds)."""
    for H, K in ar.BACKWARD_HK:
        _exact(torch_cuda, oracle, case, H, K)


# the widths on each side of the boundaries of grads_in_lds that tests/test_ac_cpu.py pins: case 2 is 8x8 / 8 multi colour
# (2 up to 13 units, 1 up to 25, then 0), case 1 is 5x5 / 3 multi colour (2 up to 52 units, then 1)
@pytest.mark.parametrize("case,H,mode", ((2, 13, 2), (2, 14, 1), (2, 25, 1), (2, 26, 0), (1, 52, 2), (1, 53, 1)))
def test_integer_gradients_on_each_side_of_the_boundaries_of_grads_in_lds(torch_cuda, oracle, case, H, mode):
    assert ar.BACKWARD_CASES[case][:5] == ((8, 8, 8, 6, True) if case == 2 else (5, 3, 3, 3, True))
    assert _exact(torch_cuda, oracle, case, H, 2)["grads_in_lds"] == mode


# ---------------------------------------------------------------------------------------------- 3. Gaussian weights and cotangents
# (S, T, obstacles, multi colour, H, K)
GAUSS = ((4, 2, 2, False, 64, 5), (5, 3, 3, True, 16, 2), (8, 8, 6, True, 64, 5), (8, 8, 6, True, 7, 1), (8, 8, 6, True, 20, 2))
AMBIGUOUS_CAP = 1e-4


@pytest.mark.parametrize("S,T,Ko,mc,H,K", GAUSS)
def test_gaussian_gradients_lie_within_the_per_entry_bound(torch_cuda, oracle, S, T, Ko, mc, H, K):
    """257 boards played for K steps by the network itself, Gaussian weights, dz and dv, through autograd (the buffers start from
    zero): every entry of the six gradients within the yardstick's bound of its float64 value."""
    torch = torch_cuda
    n = 257
    rng = np.random.default_rng(S * 100 + H + K + 1)
    blk, init, tgt = oracle.generate_mt19937(S, T, T, Ko, np.arange(3000, 3000 + n, dtype=np.uint32))
    mlp, head = pref.random_mlp(rng, tr.features(S, T, T, mc), H), ar.random_head(rng, H)
    env = _env(S, mc, blk, init, tgt, 30, AUTORESET)
    env.rollout(3, "random", seed=S)
    net = _net(torch, env, mlp, head)
    out = env.rollout_policy(K, net.policy(), select="sample", epsilon=0.1, seed=5, log=("start", "pos"))
    z, v = env.trajectory_outputs(net, out)
    dz, dv = rng.standard_normal((K, n, 4)).astype(np.float32), rng.standard_normal((K, n)).astype(np.float32)
    torch.autograd.backward((z, v), (torch.from_numpy(dz).to(env.device), torch.from_numpy(dv).to(env.device)))
    first, pos_log = out.start_pos.cpu().numpy(), out.pos_log.cpu().numpy()
    x = tr.samples_onehot(S, mc, blk, first, pos_log, tgt, K)
    flat, flat_v = dz.reshape(K * n, 4), dv.reshape(-1)
    want = ar.grads64(x, mlp, head, flat, flat_v)
    bounds, ambiguous = ar.grad_bounds(x, mlp, head, flat, flat_v)
    assert ambiguous.mean() <= AMBIGUOUS_CAP, ambiguous.mean()
    worst = {}
    for name, p in zip(NAMES, _params(net)):
        got = p.grad.cpu().numpy().astype(np.float64)
        assert got.shape == want[name].shape and np.isfinite(got).all() and np.abs(want[name]).max() > 0
        err = np.abs(got - want[name])
        worst[name] = float((err / np.maximum(bounds[name], 1e-300)).max())
        assert (err <= bounds[name]).all(), (name, worst[name])
    print(f"{S}x{S}/{T} mc={mc} H={H} K={K}: worst error / bound {worst}, ambiguous pairs {ambiguous.mean():.2e}")
    env.close()


# ---------------------------------------------------------------------------------------------- 4. the raw C-ABI into guarded memory
@pytest.mark.parametrize("case,H,mode", ((1, 7, 2), (2, 20, 1), (2, 64, 0)))
def test_raw_calls_into_guarded_memory(torch_cuda, oracle, case, H, mode):
    """Every buffer of a call between 256 guard bytes that the test owns; the outputs prefilled with the complement of the
    expected bytes, the gradient buffers with integers; pos_log holds K - 1 rows only (its last row is never read: a read past it
    would meet guard bytes, a cell id of 165); steps = 1 with pos_log = NULL.  Once per answer of grads_in_lds."""
    torch = torch_cuda
    from tiler_slider_amd import _ac_cabi as ac, _cabi
    K = 5
    c = ar.backward_case(oracle, case, H, K)
    S, T, mc, n = c["S"], c["T"], c["mc"], c["first"].shape[1]
    env = _env(S, mc, c["blk"], np.zeros((T, n), np.uint8), c["tgt"])
    dev = env.device
    assert ac.describe_ac_backward(env._dims, H, K)["grads_in_lds"] == mode
    stream = torch.cuda.current_stream(dev).cuda_stream
    kl = ar.kernel_layout(c["mlp"], c["head"])
    comp = lambda a: (~_bits(a)).view(np.float32)

    def run(steps):
        x = c["x"][:steps * n]
        dz, dv = c["dz"][:steps], c["dv"][:steps]
        want = ar.grads64(x, c["mlp"], c["head"], dz.reshape(steps * n, 4), dv.reshape(-1))
        logits, values = c["logits"][:steps], c["values"][:steps]
        bufs = {"blk": c["blk"], "tgt": c["tgt"], "first": c["first"], "pos_log": c["pos_log"][:steps - 1], "dz": dz, "dv": dv,
                "logits": comp(logits), "values": comp(values)}
        bufs.update({"net_" + k: a for k, a in zip(NAMES, kl)})
        bufs.update({"grad_" + k: c["prefill"][k] for k in NAMES})
        g = {k: _guarded(torch, dev, v) for k, v in bufs.items()}
        at = lambda k: g[k].data_ptr() + GUARD
        st = _cabi.State(None, None, at("tgt"), at("blk"), None, None, None)
        mlp = ac.Mlp(*(at("net_" + k) for k in NAMES[:4]), H, 0)
        head = ac.ValueHead(at("net_wv"), at("net_bv"))
        tin = ac.TrainIn(at("first"), at("pos_log") if steps > 1 else None, steps, 0)
        grad = ac.MlpGrad(*(at("grad_" + k) for k in NAMES[:4]))
        hgrad = ac.ValueHeadGrad(at("grad_wv"), at("grad_bv"))
        assert ac.lib().ts_ac_forward(C.byref(env._dims), C.byref(st), C.byref(mlp), C.byref(head), C.byref(tin), at("logits"), at("values"),
                                      stream) == 0
        assert ac.lib().ts_ac_backward(C.byref(env._dims), C.byref(st), C.byref(mlp), C.byref(head), C.byref(tin), at("dz"), at("dv"),
                                       C.byref(grad), C.byref(hgrad), stream) == 0
        np.testing.assert_array_equal(_bits(_payload(g["logits"], np.float32, logits.shape)), _bits(logits))
        np.testing.assert_array_equal(_bits(_payload(g["values"], np.float32, values.shape)), _bits(values))
        for k in NAMES:
            expect = (c["prefill"][k].astype(np.float64) + want[k]).astype(np.float32)
            np.testing.assert_array_equal(_bits(_payload(g["grad_" + k], np.float32, expect.shape)), _bits(expect), err_msg=f"steps {steps}: {k}")
        for k, v in bufs.items():      # the inputs: guards intact, bytes as they were
            if not k.startswith("grad_") and k not in ("logits", "values"):
                np.testing.assert_array_equal(_payload(g[k], np.uint8, (np.ascontiguousarray(v).nbytes,)), np.ascontiguousarray(v).reshape(-1).view(np.uint8))

    run(K)
    run(2)
    run(1)
    env.close()


# ---------------------------------------------------------------------------------------------- 5. every compiled kernel at occupancy
OCC_WAVES, OCC_STEPS, OCC_H = 4096, 2, 64


@pytest.mark.parametrize("name", sorted(ar.OCCUPANCY_CASES))
def test_every_compiled_ac_kernel_at_occupancy(torch_cuda, oracle, name):
    """Every kernel of the library on 262,144 boards (4,096 waves of boards: the forward launches them all, the backward's bounded
    grid strides over the 4,096 groups), two steps, 64 hidden units, on 128 distinct (level, cells, dz, dv) in turn, exactly:
    integer weights in [-1, 1]; the gradient of the batch is the gradient of the 128 with each cotangent times the number of boards
    that repeat it, held by exactness_guard to sums below 2**24."""
    torch = torch_cuda
    from tiler_slider_amd import _ac_cabi as ac
    S, T, Ko = ar.OCCUPANCY_CASES[name]
    backward = "backward" in name
    distinct, n, K, H = 128, OCC_WAVES * 64, OCC_STEPS, OCC_H
    mc = S % 2 == 0
    Cc = S * S
    rng = np.random.default_rng(S + 50 * backward + 1000)
    blk, tgt = tr.random_levels(oracle, S, T, T, Ko, distinct, 0x0CC + S)
    first, pos_log = rng.integers(0, Cc, (T, distinct)).astype(np.uint8), rng.integers(0, Cc, (K, T, distinct)).astype(np.uint8)
    mlp, head = tr.int_mlp(rng, tr.features(S, T, T, mc), H, -1, 1), ar.int_head(rng, H, -1, 1)
    level = (np.arange(n) % distinct).astype(np.int64)
    count = np.bincount(level, minlength=distinct).astype(np.float32)
    tile = lambda a: np.ascontiguousarray(a[..., level])
    env = _env(S, mc, tile(blk), np.zeros((T, n), np.uint8), tile(tgt))
    dev = env.device
    d = (ac.describe_ac_backward if backward else ac.describe_ac_forward)(env._dims, H, K)
    assert d["name"] == name and d["samples"] == K * n
    x = tr.samples_onehot(S, mc, blk, first, pos_log, tgt, K)
    if not backward:
        assert d["blocks"] * (d["threads_per_block"] // 64) >= OCC_WAVES
        z, v = env.trajectory_outputs(_net(torch, env, mlp, head, requires_grad=False), _given(torch, env, tile(first), tile(pos_log)))
        z64, _, v64, _ = ar.outputs64(x, mlp, head)
        ar.exactness_guard(x, mlp, head, np.zeros((K * distinct, 4)), np.zeros(K * distinct))
        want_z, want_v = z64.astype(np.float32).reshape(K, distinct, 4), v64.astype(np.float32).reshape(K, distinct)
        assert np.abs(want_v).max() > 0
        np.testing.assert_array_equal(_bits(z.cpu().numpy()), _bits(np.ascontiguousarray(want_z[:, level])), err_msg=name)
        np.testing.assert_array_equal(_bits(v.cpu().numpy()), _bits(np.ascontiguousarray(want_v[:, level])), err_msg=name)
    else:
        assert d["blocks"] == min(OCC_WAVES, 256 * max(1, min(8, 160 * 1024 // d["lds_bytes"])))     # a bounded grid striding over 4,096 groups
        dz, dv = rng.integers(-1, 2, (K, distinct, 4)).astype(np.float32), rng.integers(-1, 2, (K, distinct)).astype(np.float32)
        wz, wv = (dz * count[None, :, None]).reshape(K * distinct, 4), (dv * count[None, :]).reshape(-1)
        ar.exactness_guard(x, mlp, head, wz, wv)
        want = ar.grads64(x, mlp, head, wz, wv)
        kl = [torch.from_numpy(a).to(dev) for a in ar.kernel_layout(mlp, head)]
        grads = [torch.zeros_like(t) for t in kl]
        dz_t, dv_t = torch.from_numpy(np.ascontiguousarray(dz[:, level])).to(dev), torch.from_numpy(np.ascontiguousarray(dv[:, level])).to(dev)
        assert _raw_backward(torch, env, kl, torch.from_numpy(tile(first)).to(dev), torch.from_numpy(tile(pos_log)).to(dev), K, dz_t, dv_t, grads) == 0
        for k, g in zip(NAMES, grads):
            assert np.abs(want[k]).max() > 0
            np.testing.assert_array_equal(g.cpu().numpy(), want[k].astype(np.float32), err_msg=f"{name}: {k}")
    env.close()


# ---------------------------------------------------------------------------------------------- 6. autograd
def test_autograd_one_function_for_both_outputs(torch_cuda, oracle):
    torch = torch_cuda
    from tiler_slider_amd import ActorCriticNet, MlpPolicy, PolicyNet
    S, T, Ko, mc, n, H, K = 4, 2, 2, False, 257, 16, 5
    blk, init, tgt = oracle.generate_mt19937(S, T, T, Ko, np.arange(n, dtype=np.uint32))
    env = _env(S, mc, blk, init, tgt, 20, AUTORESET)
    D = tr.features(S, T, T, mc)
    gen = torch.Generator(device=env.device)
    gen.manual_seed(3)
    net = ActorCriticNet(D, H, env.device, generator=gen)
    assert [tuple(p.shape) for p in net.parameters()] == [(D, H), (H,), (H, 4), (4,), (H,), (1,)]
    bound = 1.0 / np.sqrt(H)                                       # wv and bv as w2 and b2: uniform in +- 1 / sqrt(hidden)
    assert float(net.wv.detach().abs().max()) <= bound and float(net.bv.detach().abs().max()) <= bound and float(net.wv.detach().abs().max()) > bound / 4
    shared = net.policy()
    assert isinstance(shared, MlpPolicy) and shared.w1.data_ptr() == net.w1.data_ptr() and shared.b2.data_ptr() == net.b2.data_ptr()
    out = env.rollout_policy(K, shared, select="sample", seed=1, log=("start", "pos", "act"))
    labels = out.act_log.long()
    target = torch.from_numpy(np.random.default_rng(1).standard_normal((K, n)).astype(np.float32)).to(env.device)

    def numpy_net():
        w1, b1, w2, b2, wv, bv = (p.detach().cpu().numpy() for p in _params(net))
        return (np.ascontiguousarray(w1.T), b1, np.ascontiguousarray(w2.T), b2), (wv, bv)

    first, pos_log = out.start_pos.cpu().numpy(), out.pos_log.cpu().numpy()
    x = tr.samples_onehot(S, mc, blk, first, pos_log, tgt, K)

    def check(grads, dz, dv, slack):
        mlp, head = numpy_net()
        want = ar.grads64(x, mlp, head, dz, dv)
        bounds, _ = ar.grad_bounds(x, mlp, head, dz, dv)
        # dz and dv were computed by torch in float32 from float32 outputs: 2**-17 of the sums of absolute terms covers that
        # (the reasoning of tests/test_gpu_train.py's autograd test)
        d5 = np.abs(ar.stack_cotangents(dz, dv))
        adh = d5 @ np.abs(ar.stack(mlp, head)[2]).astype(np.float64)
        h = np.abs(tr.forward64(x, mlp)[1])
        scale = ar.split({"w1": np.abs(x).T @ adh, "b1": adh.sum(axis=0), "w2": h.T @ d5, "b2": d5.sum(axis=0)})
        for name, g in zip(NAMES, grads):
            err = np.abs(g.cpu().numpy().astype(np.float64) - want[name])
            assert (err <= bounds[name] + slack * scale[name] + 1e-12).all(), name
        return want

    # both outputs carry a grad, of ONE function
    z, v = env.trajectory_outputs(net, out)
    assert z.grad_fn is not None and v.grad_fn is not None and z.grad_fn is v.grad_fn
    assert "TrajectoryOutputs" in type(z.grad_fn).__name__
    # a loss on the values alone: autograd passes None for dlogits, the layer zero-fills it
    loss_v = 0.5 * ((v - target) ** 2).mean()
    loss_v.backward()
    only_v = [p.grad.clone() for p in _params(net)]
    dv = ((v.detach() - target) / (K * n)).cpu().numpy().reshape(-1).astype(np.float64)
    check(only_v, np.zeros((K * n, 4)), dv, 2.0 ** -17)
    assert not bool(only_v[2].any()) and not bool(only_v[3].any())                # w2 and b2 never see dv
    assert all(float(g.abs().sum()) > 0 for g in (only_v[0], only_v[1], only_v[4], only_v[5]))
    # a loss on the logits alone, into fresh grads
    net.zero_grad(set_to_none=True)
    z, v = env.trajectory_outputs(net, out)
    torch.nn.functional.cross_entropy(z.reshape(-1, 4), labels.reshape(-1)).backward()
    only_z = [p.grad.clone() for p in _params(net)]
    zt = torch.tensor(ar.outputs64(x, *numpy_net())[0], requires_grad=True)
    torch.nn.functional.cross_entropy(zt, labels.reshape(-1).cpu()).backward()
    check(only_z, zt.grad.numpy(), np.zeros(K * n), 2.0 ** -17)
    assert not bool(only_z[4].any()) and not bool(only_z[5].any())
    assert all(float(g.abs().sum()) > 0 for g in only_z[:4])
    # the actor's four gradients are trajectory_logits()' on a PolicyNet of the same storage values
    twin = PolicyNet(D, H, env.device)
    with torch.no_grad():
        for p, q in zip(twin.parameters(), _params(net)[:4]):
            p.copy_(q)
    torch.nn.functional.cross_entropy(env.trajectory_logits(twin, out).reshape(-1, 4), labels.reshape(-1)).backward()
    for p, g in zip(twin.parameters(), only_z[:4]):
        assert torch.allclose(p.grad, g, rtol=1e-4, atol=1e-6)
    # gradients accumulate across two calls: the second backward, of both losses at once, adds to the first
    z, v = env.trajectory_outputs(net, out)
    (torch.nn.functional.cross_entropy(z.reshape(-1, 4), labels.reshape(-1)) + 0.5 * ((v - target) ** 2).mean()).backward()
    for p, a, b in zip(_params(net), only_z, only_v):
        assert torch.allclose(p.grad, 2 * a + b, rtol=1e-4, atol=1e-6)
    # no_grad gives no graph
    with torch.no_grad():
        qz, qv = env.trajectory_outputs(net, out)
    assert qz.grad_fn is None and qv.grad_fn is None and not qz.requires_grad and not qv.requires_grad
    assert torch.equal(qz, z.detach()) and torch.equal(qv, v.detach())
    # an optimiser step is played by the next rollout_policy(..., net.policy()), without a fresh MlpPolicy
    before = env.policy_logits(shared).clone()
    torch.optim.SGD(net.parameters(), lr=0.5).step()
    x_now = tr.onehot(S, mc, blk, env._pos.cpu().numpy(), tgt)
    z64, zb, v64, vb = ar.outputs64(x_now, *numpy_net())
    play = env.rollout_policy(2, net.policy(), select="greedy", seed=2, log=("logits",), advance=False)
    now_z, now_v = env.trajectory_outputs(net)
    assert tuple(now_v.shape) == (1, n)
    for got in (play.logits_log[0], env.policy_logits(shared), now_z[0].detach()):
        assert (np.abs(got.cpu().numpy().astype(np.float64) - z64) <= zb).all()
    assert (np.abs(now_v[0].detach().cpu().numpy().astype(np.float64) - v64) <= vb).all()
    assert not torch.equal(env.policy_logits(shared), before)
    # values feed trajectory_returns as they are; row 0 of the standing boards' values is its last_value
    flags = env.rollout_policy(K, shared, select="sample", seed=9, log=("start", "pos", "flags"))
    with torch.no_grad():
        _, vals = env.trajectory_outputs(net, flags)
        _, last = env.trajectory_outputs(net)
    ret = env.trajectory_returns(flags, gamma=0.9, lam=0.8, values=vals, last_value=last[0])
    assert tuple(ret.adv.shape) == (K, n) and bool(torch.isfinite(ret.adv).all()) and torch.allclose(ret.ret, ret.adv + vals * ret.mask, rtol=1e-4, atol=1e-4)
    # the host's checks are trajectory_logits()'
    with pytest.raises(TypeError):
        env.trajectory_outputs(twin, out)                                                                 # not an ActorCriticNet
    with pytest.raises(TypeError):
        env.trajectory_outputs(net, "rollout")
    with pytest.raises(ValueError):
        env.trajectory_outputs(net, env.rollout_policy(2, shared, log=("pos",), advance=False))          # no start_pos
    other = _env(S, mc, blk[:, :100], init[:, :100], tgt[:, :100], 20, AUTORESET)
    with pytest.raises(ValueError):
        other.trajectory_outputs(net, out)                                                                # another N
    with pytest.raises(ValueError):
        env.trajectory_outputs(ActorCriticNet(D + 16, H, env.device), out)
    # to_linear / from_linear / the dense forward
    l1, l2, lv = net.to_linear()
    again = ActorCriticNet.from_linear(l1, l2, lv)
    assert all(torch.equal(a, b) for a, b in zip(again.parameters(), net.parameters()))
    with torch.no_grad():
        planes = env.encode_onehot().flatten(1)
        hidden = torch.relu(l1(planes))
        dense_z, dense_v = net(planes)
        now_z, now_v = env.trajectory_outputs(net)                 # the boards have moved since the last such call
    assert torch.allclose(dense_z, l2(hidden), rtol=1e-4, atol=1e-4) and torch.allclose(dense_v, lv(hidden)[:, 0], rtol=1e-4, atol=1e-4)
    assert torch.allclose(now_z[0], dense_z, rtol=1e-4, atol=1e-4) and torch.allclose(now_v[0], dense_v, rtol=1e-4, atol=1e-4)
    # the backward of a closed environment raises instead of launching
    z, v = env.trajectory_outputs(net, out)
    env.close()
    with pytest.raises(RuntimeError):
        v.sum().backward()


# ---------------------------------------------------------------------------------------------- 7. one actor-critic step
def test_fifty_adam_steps_lower_both_terms_of_the_actor_critic_loss(torch_cuda):
    """256 solvable 4x4 levels (section 16's learning check) played for 8 steps by the distance table's expert with a third of
    the steps explored; on the samples the expert has a move for, the loss is cross-entropy against trajectory_labels' expert
    plus 0.5 (v - (-moves))**2.  After 50 Adam steps, fixed seeds, each of the two terms is lower than at the start."""
    torch = torch_cuda
    from tiler_slider_amd import ActorCriticNet, TilerSliderEnvFactory, VecTilerSliderEnv
    dev = torch.device("cuda", 0)
    seeds = TilerSliderEnvFactory.solvable_seeds(256, size=4, num_tiles=2, num_obstacles=2, device=dev)
    env = VecTilerSliderEnv.from_seeds(seeds, size=4, num_tiles=2, num_obstacles=2, device=dev, obs_dtype=None, auto_reset=True)
    env.reset()
    table = env.build_table()
    out = env.rollout(8, "table", table=table, epsilon=1 / 3, seed=4, log=("start", "pos"))
    moves, _, action = env.trajectory_labels(out, table)
    labelled = action != 255
    assert int(labelled.sum()) >= 256
    labels, cost = action[labelled].long(), -moves[labelled].float()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    net = ActorCriticNet(env.onehot_channels * 16, 32, dev, generator=gen)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    terms = []
    for _ in range(50):
        opt.zero_grad(set_to_none=True)
        z, v = env.trajectory_outputs(net, out)
        ce = torch.nn.functional.cross_entropy(z[labelled], labels)
        mse = 0.5 * ((v[labelled] - cost) ** 2).mean()
        (ce + mse).backward()
        opt.step()
        terms.append(torch.stack([ce.detach(), mse.detach()]))
    terms = torch.stack(terms).cpu().numpy()
    print(f"actor-critic step: cross-entropy {terms[0, 0]:.4f} -> {terms[-1, 0]:.4f}, value loss {terms[0, 1]:.4f} -> {terms[-1, 1]:.4f}")
    assert np.isfinite(terms).all() and terms[-1, 0] < terms[0, 0] and terms[-1, 1] < terms[0, 1]
