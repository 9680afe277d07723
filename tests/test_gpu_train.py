"""The trainable policies on the GPU (lib/libtiler_slider_train.so, VecTilerSliderEnv.trajectory_logits, PolicyNet) against the
CPU yardstick tests/train_reference.py - the definition of include/tiler_slider_train.h on NumPy -, against the rollout's own
logged logits, and against float64 torch autograd on the oracle twin's dense planes."""
import ctypes as C

import numpy as np
import pytest

import policy_reference as pref
import rollout_reference as rref
import train_reference as tr
from table_harness import GUARD, guarded as _guarded, payload as _payload

pytestmark = pytest.mark.gpu

STRICT, AUTORESET = 0, 1
NAMES = ("w1", "b1", "w2", "b2")


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


def _net(torch, env, mlp, requires_grad=True):
    """A PolicyNet holding `mlp` (torch.nn.Linear's layout, as the yardsticks keep it)."""
    from tiler_slider_amd import PolicyNet
    H, D = mlp[0].shape
    net = PolicyNet(D, H, env.device)
    with torch.no_grad():
        for p, a in zip((net.w1, net.b1, net.w2, net.b2), tr.kernel_layout(mlp)):
            p.copy_(torch.from_numpy(a))
    for p in net.parameters():
        p.requires_grad_(requires_grad)
    return net


def _given(torch, env, first, pos_log):
    """A Rollout that holds given cells: what rollout_policy(..., log=("start", "pos")) returns, with cells of our choosing."""
    from tiler_slider_amd import Rollout
    dev = env.device
    return Rollout(pos_log.shape[0], start_pos=torch.from_numpy(first).to(dev), pos_log=torch.from_numpy(pos_log).to(dev))


def _raw_backward(torch, env, kl, first, pos_log, K, dz, grads):
    """ts_train_backward itself: kl, first, pos_log, dz, grads are device tensors (pos_log may be None)."""
    from tiler_slider_amd import _train_cabi as tc
    mlp = tc.Mlp(*(t.data_ptr() for t in kl), kl[0].shape[1], 0)
    tin = tc.TrainIn(first.data_ptr() if first.numel() else None, pos_log.data_ptr() if pos_log is not None and pos_log.numel() else None, K, 0)
    grad = tc.MlpGrad(*(g.data_ptr() for g in grads))
    return tc.lib().ts_train_backward(C.byref(env._dims), C.byref(env._state), C.byref(mlp), C.byref(tin), dz.data_ptr(), C.byref(grad),
                                      torch.cuda.current_stream(env.device).cuda_stream)


# ---------------------------------------------------------------------------------------------- 1. forward exactness
@pytest.mark.parametrize("K", (1, 2, 5))
@pytest.mark.parametrize("mode", (STRICT, AUTORESET))
def test_trajectory_logits_equal_the_rollouts_own_logits_bit_for_bit(torch_cuda, oracle, mode, K):
    """257 boards four random steps into their episodes, integer weights in [-2, 2], a quarter of the steps explored: the
    logits of the logged trajectory are the rollout's logits_log, and the yardstick's, bit for bit - in strict mode with boards
    that stand done, in auto-reset mode with boards that are reset; in both, boards win."""
    torch = torch_cuda
    S, T, Ko, mc, n, max_steps, H = 4, 2, 2, False, 257, 6, 16
    blk, init, tgt = oracle.generate_mt19937(S, T, T, Ko, np.arange(n, dtype=np.uint32))
    mlp = tr.int_mlp(np.random.default_rng(40 + K), tr.features(S, T, T, mc), H)
    start = rref.rollout(oracle, S, mc, max_steps, blk, init, tgt, 4, rref.RANDOM, mode, seed=1)
    kw = dict(pos=start["pos"], step_count=start["step_count"], done=start["done"])
    want = pref.rollout(oracle, S, mc, max_steps, blk, init, tgt, mlp, K, pref.GREEDY, mode, threshold=rref.threshold_of(0.25), seed=77,
                        exact32=True, **kw)
    if K == 5:
        assert want["won"].any()
        assert ((want["flags_log"] & (rref.FLAG_AUTORESET if mode == AUTORESET else rref.FLAG_STEPPED_DONE)) != 0).any()
    env = _env(S, mc, blk, init, tgt, max_steps, mode)
    for name in ("pos", "step_count", "done"):
        _put(env, "_" + name, start[name])
    net = _net(torch, env, mlp)
    now = env.trajectory_logits(net)                            # the boards as they stand: K = 1
    assert tuple(now.shape) == (1, n, 4) and now.grad_fn is not None
    assert torch.equal(now.detach()[0], env.policy_logits(net.policy()))
    out = env.rollout_policy(K, net.policy(), select="greedy", epsilon=0.25, seed=77, log=("start", "pos", "logits", "flags"))
    np.testing.assert_array_equal(out.start_pos.cpu().numpy(), start["pos"])
    np.testing.assert_array_equal(out.flags_log.cpu().numpy(), want["flags_log"])
    z = env.trajectory_logits(net, out)
    assert z.dtype == torch.float32 and tuple(z.shape) == (K, n, 4) and z.grad_fn is not None
    np.testing.assert_array_equal(_bits(z.detach().cpu().numpy()), _bits(out.logits_log.cpu().numpy()))
    np.testing.assert_array_equal(_bits(z.detach().cpu().numpy()), _bits(want["logits_log"]))
    assert torch.equal(env.trajectory_logits(net.policy(), out), z.detach())     # an MlpPolicy: the forward only
    assert env.trajectory_logits(net.policy(), out).grad_fn is None
    env.close()


# ---------------------------------------------------------------------------------------------- 2. backward exactness
@pytest.mark.parametrize("case", range(len(tr.BACKWARD_CASES)))
def test_integer_gradients_equal_the_yardstick_bit_for_bit(torch_cuda, oracle, case):
    """257 boards (one wave and a tail whose dead lanes must add nothing), H in {1, 7, 64} x K in {1, 2, 5}, integer weights in
    [-2, 2], dz in {-1, 0, 1}, cells drawn at random, the four buffers prefilled with integers in [-3, 3] (the call adds):
    tr.backward_case asserts on the yardstick's own numbers that the case bites, exactness_guard that every order is exact."""
    torch = torch_cuda
    from tiler_slider_amd import _train_cabi as tc
    S, T, Tt, Ko, mc, what, _ = tr.BACKWARD_CASES[case]
    modes = set()
    # 8x8 / 8 multi colour keeps only the tile planes in LDS from H = 14 to 25: a width the three above do not reach
    for H, K in tr.BACKWARD_HK + (((20, 2),) if what == "not in LDS" else ()):
        c = tr.backward_case(oracle, case, H, K)
        n = c["first"].shape[1]
        env = _env(S, mc, c["blk"], np.zeros((T, n), np.uint8), c["tgt"])
        dev = env.device
        d = tc.describe_train_backward(env._dims, H, K)
        modes.add(d["grads_in_lds"])
        if what == "not in LDS":
            assert d["grads_in_lds"] == (2 if H <= 13 else 1 if H <= 25 else 0), d
        kl = [torch.from_numpy(a).to(dev) for a in tr.kernel_layout(c["mlp"])]
        first, pos_log = torch.from_numpy(c["first"]).to(dev), torch.from_numpy(c["pos_log"]).to(dev)
        grads = [torch.from_numpy(c["prefill"][k]).to(dev) for k in NAMES]
        assert _raw_backward(torch, env, kl, first, pos_log if K > 1 else None, K, torch.from_numpy(c["dz"]).to(dev), grads) == 0
        for name, g in zip(NAMES, grads):
            np.testing.assert_array_equal(_bits(g.cpu().numpy()), _bits(c["want"][name]), err_msg=f"case {case} {what} H={H} K={K}: {name}")
        assert torch.equal(grads[0][torch.from_numpy(c["untouched"]).to(dev)], torch.from_numpy(c["prefill"]["w1"][c["untouched"]]).to(dev))
        # the forward on the same cells (shared, beyond the board), through the host: a Rollout that holds them
        if T:
            z = env.trajectory_logits(_net(torch, env, c["mlp"], requires_grad=False), _given(torch, env, c["first"], c["pos_log"]))
            np.testing.assert_array_equal(_bits(z.cpu().numpy()), _bits(c["logits"]), err_msg=f"case {case} H={H} K={K}: logits")
        print(f"case {case} {what} H={H} K={K}: grads_in_lds {d['grads_in_lds']}, pre == 0 with dh != 0 {c['bites']:.3f}, shared cells {c['shared']:.3f}, "
              f"untouched rows {int(c['untouched'].sum())}")
        env.close()
    if what == "not in LDS":
        assert modes == {0, 1, 2}


# ---------------------------------------------------------------------------------------------- 3. Gaussian weights and dz
# (S, T, obstacles, multi colour, H, K)
GAUSS = ((4, 2, 2, False, 64, 5), (5, 3, 3, True, 16, 2), (8, 8, 6, True, 64, 5), (8, 8, 6, True, 7, 1), (8, 8, 6, True, 20, 2))
AMBIGUOUS_CAP = 1e-4


@pytest.mark.parametrize("S,T,Ko,mc,H,K", GAUSS)
def test_gaussian_gradients_lie_within_the_per_entry_bound(torch_cuda, oracle, S, T, Ko, mc, H, K):
    """257 boards played for K steps by the network itself, Gaussian weights and dz, through autograd (the buffers start from
    zero): every entry of the four gradients within the yardstick's bound of its float64 value, and of float64 torch autograd on
    the oracle twin's dense planes; the ambiguous (sample, unit) pairs - where the bound must carry a whole |dh| - at most 1e-4."""
    torch = torch_cuda
    n = 257
    rng = np.random.default_rng(S * 100 + H + K)
    blk, init, tgt = oracle.generate_mt19937(S, T, T, Ko, np.arange(3000, 3000 + n, dtype=np.uint32))
    mlp = pref.random_mlp(rng, tr.features(S, T, T, mc), H)
    env = _env(S, mc, blk, init, tgt, 30, AUTORESET)
    env.rollout(3, "random", seed=S)
    net = _net(torch, env, mlp)
    out = env.rollout_policy(K, net.policy(), select="sample", epsilon=0.1, seed=5, log=("start", "pos", "logits"))
    z = env.trajectory_logits(net, out)
    dz = rng.standard_normal((K, n, 4)).astype(np.float32)
    z.backward(torch.from_numpy(dz).to(env.device))
    # the oracle twin's planes of every logged board
    twin = oracle.OracleBatch(S, mc, 30, blk, init, tgt)
    first, pos_log = out.start_pos.cpu().numpy(), out.pos_log.cpu().numpy()
    xs = []
    for k in range(K):
        twin.pos[...] = first if k == 0 else pos_log[k - 1]
        xs.append(twin.encode_onehot().reshape(n, -1).copy())
    x = np.concatenate(xs, axis=0)
    np.testing.assert_array_equal(x, tr.samples_onehot(S, mc, blk, first, pos_log, tgt, K))
    flat = dz.reshape(K * n, 4)
    zr, zb = tr.logits64(x, mlp)
    assert (np.abs(z.detach().cpu().numpy().reshape(K * n, 4).astype(np.float64) - zr) <= zb).all()
    want, dense = tr.grads64(x, mlp, flat), tr.torch_grads64(x, mlp, flat)
    bounds, ambiguous = tr.grad_bounds(x, mlp, flat)
    assert ambiguous.mean() <= AMBIGUOUS_CAP, ambiguous.mean()
    worst = {}
    for name, p in zip(NAMES, (net.w1, net.b1, net.w2, net.b2)):
        got = p.grad.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all() and np.abs(want[name]).max() > 0
        for ref in (want[name], dense[name]):
            err = np.abs(got - ref)
            slack = 1e-12 * np.abs(ref)                        # the two float64 references agree to this
            assert (err <= bounds[name] + slack).all(), (name, float((err / np.maximum(bounds[name], 1e-300)).max()))
        worst[name] = float((np.abs(got - want[name]) / np.maximum(bounds[name], 1e-300)).max())
    print(f"{S}x{S}/{T} mc={mc} H={H} K={K}: worst error / bound {worst}, ambiguous pairs {ambiguous.mean():.2e}")
    env.close()


# ---------------------------------------------------------------------------------------------- 4. the raw C-ABI into guarded memory
@pytest.mark.parametrize("case,H,mode", ((1, 7, 2), (2, 20, 1), (2, 64, 0)))
def test_raw_calls_into_guarded_memory(torch_cuda, oracle, case, H, mode):
    """Every buffer of a call between 256 guard bytes; the logits prefilled with the complement of the expected bytes, the
    gradient buffers with integers; pos_log holds K - 1 rows only (its last row is never read: a read past it would meet guard
    bytes, a cell id of 165); steps = 1 with pos_log = NULL.  5x5 / 3 multi colour at H = 7 flushes the whole gradient of w1 from
    LDS; 8x8 / 8 multi colour adds the obstacle and target rows (H = 20) or every row (H = 64) of it with global atomics."""
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _train_cabi as tc
    K = 5
    c = tr.backward_case(oracle, case, H, K)
    S, T, mc, n = c["S"], c["T"], c["mc"], c["first"].shape[1]
    env = _env(S, mc, c["blk"], np.zeros((T, n), np.uint8), c["tgt"])
    dev = env.device
    assert tc.describe_train_backward(env._dims, H, K)["grads_in_lds"] == mode
    stream = torch.cuda.current_stream(dev).cuda_stream
    kl = tr.kernel_layout(c["mlp"])
    comp = lambda a: (~_bits(a)).view(np.float32)

    def run(steps):
        x = c["x"][:steps * n]
        dz = c["dz"][:steps]
        want = tr.grads64(x, c["mlp"], dz.reshape(steps * n, 4))
        logits = c["logits"][:steps]
        bufs = {"blk": c["blk"], "tgt": c["tgt"], "first": c["first"], "pos_log": c["pos_log"][:steps - 1], "dz": dz, "logits": comp(logits)}
        bufs.update({"net_" + k: a for k, a in zip(NAMES, kl)})
        bufs.update({"grad_" + k: c["prefill"][k] for k in NAMES})
        g = {k: _guarded(torch, dev, v) for k, v in bufs.items()}
        at = lambda k: g[k].data_ptr() + GUARD
        st = _cabi.State(None, None, at("tgt"), at("blk"), None, None, None)
        mlp = tc.Mlp(*(at("net_" + k) for k in NAMES), H, 0)
        tin = tc.TrainIn(at("first"), at("pos_log") if steps > 1 else None, steps, 0)
        grad = tc.MlpGrad(*(at("grad_" + k) for k in NAMES))
        assert tc.lib().ts_train_forward(C.byref(env._dims), C.byref(st), C.byref(mlp), C.byref(tin), at("logits"), stream) == 0
        assert tc.lib().ts_train_backward(C.byref(env._dims), C.byref(st), C.byref(mlp), C.byref(tin), at("dz"), C.byref(grad), stream) == 0
        np.testing.assert_array_equal(_bits(_payload(g["logits"], np.float32, logits.shape)), _bits(logits))
        for k in NAMES:
            expect = (c["prefill"][k].astype(np.float64) + want[k]).astype(np.float32)
            np.testing.assert_array_equal(_bits(_payload(g["grad_" + k], np.float32, expect.shape)), _bits(expect), err_msg=f"steps {steps}: {k}")
        for k, v in bufs.items():      # the inputs: guards intact, bytes as they were
            if not k.startswith("grad_") and k != "logits":
                np.testing.assert_array_equal(_payload(g[k], np.uint8, (np.ascontiguousarray(v).nbytes,)), np.ascontiguousarray(v).reshape(-1).view(np.uint8))

    run(K)
    run(2)
    run(1)
    env.close()


# ---------------------------------------------------------------------------------------------- 5. every compiled kernel at occupancy
OCC_WAVES, OCC_STEPS, OCC_H = 4096, 2, 64


@pytest.mark.parametrize("name", sorted(tr.OCCUPANCY_CASES))
def test_every_compiled_train_kernel_at_occupancy(torch_cuda, oracle, name):
    """Every kernel of the training library on 262,144 boards (4,096 waves of boards: the forward launches them all, the backward's
    bounded grid strides over the 4,096 groups), two steps, 64 hidden units, on 128 distinct (level, cells, dz) in turn, exactly: integer weights in [-1, 1]; the gradient of the batch is the gradient of the 128
    with each dz times the number of boards that repeat it, held by exactness_guard to sums below 2**24."""
    torch = torch_cuda
    from tiler_slider_amd import _train_cabi as tc
    S, T, Ko = tr.OCCUPANCY_CASES[name]
    backward = "backward" in name
    distinct, n, K, H = 128, OCC_WAVES * 64, OCC_STEPS, OCC_H
    mc = S % 2 == 0
    Cc = S * S
    rng = np.random.default_rng(S + 50 * backward)
    blk, tgt = tr.random_levels(oracle, S, T, T, Ko, distinct, 0x0CC + S)
    first, pos_log = rng.integers(0, Cc, (T, distinct)).astype(np.uint8), rng.integers(0, Cc, (K, T, distinct)).astype(np.uint8)
    mlp = tr.int_mlp(rng, tr.features(S, T, T, mc), H, -1, 1)
    level = (np.arange(n) % distinct).astype(np.int64)
    count = np.bincount(level, minlength=distinct).astype(np.float32)
    tile = lambda a: np.ascontiguousarray(a[..., level])
    env = _env(S, mc, tile(blk), np.zeros((T, n), np.uint8), tile(tgt))
    dev = env.device
    d = (tc.describe_train_backward if backward else tc.describe_train_forward)(env._dims, H, K)
    assert d["name"] == name and d["samples"] == K * n
    x = tr.samples_onehot(S, mc, blk, first, pos_log, tgt, K)
    if not backward:
        assert d["blocks"] * (d["threads_per_block"] // 64) >= OCC_WAVES
        z = env.trajectory_logits(_net(torch, env, mlp, requires_grad=False), _given(torch, env, tile(first), tile(pos_log)))
        want = tr.forward64(x, mlp)[2].astype(np.float32).reshape(K, distinct, 4)
        tr.exactness_guard(x, mlp, np.zeros((K * distinct, 4)))
        np.testing.assert_array_equal(_bits(z.cpu().numpy()), _bits(np.ascontiguousarray(want[:, level])), err_msg=name)
    else:
        assert d["blocks"] == min(OCC_WAVES, 256 * max(1, min(8, 160 * 1024 // d["lds_bytes"])))     # a bounded grid striding over 4,096 groups
        dz = rng.integers(-1, 2, (K, distinct, 4)).astype(np.float32)
        weighted = (dz * count[None, :, None]).reshape(K * distinct, 4)
        tr.exactness_guard(x, mlp, weighted)
        want = tr.grads64(x, mlp, weighted)
        kl = [torch.from_numpy(a).to(dev) for a in tr.kernel_layout(mlp)]
        grads = [torch.zeros_like(t) for t in kl]
        dz_t = torch.from_numpy(np.ascontiguousarray(dz[:, level])).to(dev)
        assert _raw_backward(torch, env, kl, torch.from_numpy(tile(first)).to(dev), torch.from_numpy(tile(pos_log)).to(dev), K, dz_t, grads) == 0
        for k, g in zip(NAMES, grads):
            assert np.abs(want[k]).max() > 0
            np.testing.assert_array_equal(g.cpu().numpy(), want[k].astype(np.float32), err_msg=f"{name}: {k}")
    env.close()


# ---------------------------------------------------------------------------------------------- 6. autograd
def test_autograd_fills_accumulates_and_the_next_call_plays_the_stepped_weights(torch_cuda, oracle):
    torch = torch_cuda
    from tiler_slider_amd import MlpPolicy, PolicyNet, Rollout
    S, T, Ko, mc, n, H, K = 4, 2, 2, False, 257, 16, 5
    blk, init, tgt = oracle.generate_mt19937(S, T, T, Ko, np.arange(n, dtype=np.uint32))
    env = _env(S, mc, blk, init, tgt, 20, AUTORESET)
    D = tr.features(S, T, T, mc)
    gen = torch.Generator(device=env.device)
    gen.manual_seed(3)
    net = PolicyNet(D, H, env.device, generator=gen)
    assert [tuple(p.shape) for p in net.parameters()] == [(D, H), (H,), (H, 4), (4,)]
    shared = net.policy()
    assert isinstance(shared, MlpPolicy) and shared.w1.data_ptr() == net.w1.data_ptr() and shared.b2.data_ptr() == net.b2.data_ptr()
    out = env.rollout_policy(K, shared, select="sample", seed=1, log=("start", "pos", "act"))
    assert isinstance(out, Rollout) and out.logits_log is None and tuple(out.start_pos.shape) == (T, n)
    labels = out.act_log.long()

    def loss_of():
        z = env.trajectory_logits(net, out)
        return torch.nn.functional.cross_entropy(z.reshape(-1, 4), labels.reshape(-1))

    def numpy_mlp():
        w1, b1, w2, b2 = (p.detach().cpu().numpy() for p in (net.w1, net.b1, net.w2, net.b2))
        return np.ascontiguousarray(w1.T), b1, np.ascontiguousarray(w2.T), b2

    loss = loss_of()
    assert loss.grad_fn is not None
    loss.backward()
    once = [p.grad.clone() for p in net.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0 for g in once)
    # the same gradient from float64 autograd on dense planes, within the yardstick's bound
    first, pos_log = out.start_pos.cpu().numpy(), out.pos_log.cpu().numpy()
    x = tr.samples_onehot(S, mc, blk, first, pos_log, tgt, K)
    zt = torch.tensor(tr.forward64(x, numpy_mlp())[2], requires_grad=True)
    torch.nn.functional.cross_entropy(zt, labels.reshape(-1).cpu()).backward()
    dz = zt.grad.numpy()
    want = tr.grads64(x, numpy_mlp(), dz)
    bounds, _ = tr.grad_bounds(x, numpy_mlp(), dz)
    for name, g in zip(NAMES, once):
        # the kernel's dz was computed by torch in float32 from float32 logits, this one in float64 from float64 logits: the logits
        # differ by at most their bound (~1e-6 here) and softmax-cross-entropy is 1-Lipschitz in them, float32 softmax adds a few
        # 2**-24: dz differs by a few 1e-7 of its size, and the gradients are linear in dz.  2**-17 of the sums of absolute terms
        # leaves a factor of about thirty over that
        err = np.abs(g.cpu().numpy().astype(np.float64) - want[name])
        scale = {"w1": np.abs(x).T @ np.abs(dz @ numpy_mlp()[2].astype(np.float64)), "b1": np.abs(dz @ numpy_mlp()[2].astype(np.float64)).sum(axis=0),
                 "w2": np.abs(tr.forward64(x, numpy_mlp())[1]).T @ np.abs(dz), "b2": np.abs(dz).sum(axis=0)}[name]
        assert (err <= bounds[name] + 2.0 ** -17 * scale + 1e-12).all(), name
    loss_of().backward()                                           # a second backward accumulates
    for p, g in zip(net.parameters(), once):
        assert torch.allclose(p.grad, 2 * g, rtol=1e-4, atol=1e-6)
    with torch.no_grad():
        quiet = env.trajectory_logits(net, out)
    assert quiet.grad_fn is None and not quiet.requires_grad
    assert env.trajectory_logits(net.policy(), out).grad_fn is None
    # a step of SGD: the next call plays the new weights, without a fresh MlpPolicy
    before = env.policy_logits(shared).clone()
    opt = torch.optim.SGD(net.parameters(), lr=0.5)
    opt.step()
    x_now = tr.onehot(S, mc, blk, env._pos.cpu().numpy(), tgt)
    zr, zb = tr.logits64(x_now, numpy_mlp())
    after = env.policy_logits(shared)
    assert (np.abs(after.cpu().numpy().astype(np.float64) - zr) <= zb).all()
    assert not torch.equal(after, before)
    play = env.rollout_policy(2, net.policy(), select="greedy", seed=2, log=("logits",), advance=False)
    for got in (env.trajectory_logits(net)[0].detach(), play.logits_log[0]):
        assert (np.abs(got.cpu().numpy().astype(np.float64) - zr) <= zb).all()
    # the host's checks
    with pytest.raises(TypeError):
        env.trajectory_logits("net", out)
    with pytest.raises(TypeError):
        env.trajectory_logits(net, "rollout")
    with pytest.raises(ValueError):
        env.trajectory_logits(net, env.rollout_policy(2, shared, log=("pos",), advance=False))          # no start_pos
    with pytest.raises(ValueError):
        env.trajectory_logits(net, env.rollout_policy(2, shared, log=("start",), advance=False))        # no pos_log
    other = _env(S, mc, blk[:, :100], init[:, :100], tgt[:, :100], 20, AUTORESET)
    with pytest.raises(ValueError):
        other.trajectory_logits(net, out)                                                                # another N
    with pytest.raises(ValueError):
        env.trajectory_logits(net, Rollout(K, start_pos=out.start_pos.cpu(), pos_log=out.pos_log.cpu()))  # a foreign device
    with pytest.raises(ValueError):
        env.trajectory_logits(PolicyNet(D + 16, H, env.device), out)
    with pytest.raises(ValueError):
        MlpPolicy.from_kernel_layout(net.w1.t(), net.b1, net.w2, net.b2)                                  # not [D, H] contiguous
    with pytest.raises(TypeError):
        MlpPolicy.from_kernel_layout(net.w1.double(), net.b1, net.w2, net.b2)
    mapped = _env(S, mc, blk[:, :64], init[:, :64], tgt[:, :64], 20, AUTORESET, host_mapped=True)
    with pytest.raises(ValueError):
        mapped.trajectory_logits(net)
    l1, l2 = net.to_linear()
    again = PolicyNet.from_linear(l1, l2)
    assert all(torch.equal(a, b) for a, b in zip(again.parameters(), net.parameters()))
    with torch.no_grad():
        dense = l2(torch.relu(l1(env.encode_onehot().flatten(1))))
    assert torch.allclose(env.trajectory_logits(net)[0].detach(), dense, rtol=1e-4, atol=1e-4)
    assert torch.allclose(net(env.encode_onehot().flatten(1)), dense, rtol=1e-4, atol=1e-4)
    # the backward of a closed environment raises instead of launching
    z = env.trajectory_logits(net, out)
    env.close()
    with pytest.raises(RuntimeError):
        z.sum().backward()


def test_a_call_on_a_stream_of_its_own_ordered_after_a_step(torch_cuda, oracle):
    """2**18 boards, one extra stream, no host synchronisation until the end: the forward and the backward are enqueued while
    the step still runs.  A launch that ignored its `stream` argument would read cells the step has not written yet.  Integer
    weights and dz = 1: exact."""
    torch = torch_cuda
    S, T, Ko, mc, n, H = 4, 2, 2, False, 1 << 18, 16
    blk, init, tgt = oracle.generate_mt19937(S, T, T, Ko, np.arange(n, dtype=np.uint32))
    mlp = tr.int_mlp(np.random.default_rng(2), tr.features(S, T, T, mc), H)
    act = oracle.fill_actions(n, seed=0x57EA, step_index=0)
    twin = oracle.OracleBatch(S, mc, 30, blk, init, tgt)
    twin.reset()
    x0 = twin.encode_onehot().reshape(n, -1).copy()
    twin.step(act, mode=AUTORESET, obs=False)
    x1 = twin.encode_onehot().reshape(n, -1).copy()
    assert (x0 != x1).any(axis=1).sum() >= 1000                  # the step matters
    dz = np.ones((n, 4), np.float32)
    tr.exactness_guard(x1, mlp, dz)
    want = tr.grads64(x1, mlp, dz)
    assert any((tr.grads64(x0, mlp, dz)[k] != want[k]).any() for k in NAMES)
    env = _env(S, mc, blk, init, tgt, 30, AUTORESET)
    net = _net(torch, env, mlp)
    actions = torch.from_numpy(act).to(env.device)
    side = torch.cuda.Stream(device=env.device)
    assert side.cuda_stream != torch.cuda.current_stream(env.device).cuda_stream
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        env.step(actions)
        z = env.trajectory_logits(net)
        z.sum().backward()
    side.synchronize()
    np.testing.assert_array_equal(_bits(z.detach().cpu().numpy()[0]), _bits(pref.logits_exact32(x1, mlp)))
    for name, p in zip(NAMES, (net.w1, net.b1, net.w2, net.b2)):
        np.testing.assert_array_equal(p.grad.cpu().numpy(), want[name].astype(np.float32), err_msg=name)


# ---------------------------------------------------------------------------------------------- 7. one learning check
def test_fifty_adam_steps_of_behaviour_cloning_lower_the_loss(torch_cuda):
    """256 solvable 4x4 levels, labels from the distance table's expert, cross-entropy on trajectory_logits, 50 Adam steps, fixed
    seeds: the only claim is a direction - the final loss is below the first."""
    torch = torch_cuda
    from tiler_slider_amd import PolicyNet, TilerSliderEnvFactory, VecTilerSliderEnv
    dev = torch.device("cuda", 0)
    seeds = TilerSliderEnvFactory.solvable_seeds(256, size=4, num_tiles=2, num_obstacles=2, device=dev)
    env = VecTilerSliderEnv.from_seeds(seeds, size=4, num_tiles=2, num_obstacles=2, device=dev, obs_dtype=None)
    env.reset()
    table = env.build_table()
    labels = env.expert_actions_from(table).long()
    assert bool((labels <= 3).all())                               # every level can be solved: the expert has a move
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    net = PolicyNet(env.onehot_channels * 16, 32, dev, generator=gen)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    losses = []
    for _ in range(50):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(env.trajectory_logits(net)[0], labels)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in torch.stack(losses).cpu()]
    agree = float((env.policy_logits(net.policy()).argmax(dim=1) == labels).float().mean())
    print(f"behaviour cloning: loss {losses[0]:.4f} -> {losses[-1]:.4f} (every tenth: {[round(v, 4) for v in losses[::10]]}), expert agreement {agree:.3f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
