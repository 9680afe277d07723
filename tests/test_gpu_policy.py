"""The neural-policy rollouts on the GPU (lib/libtiler_slider_policy.so, VecTilerSliderEnv.policy_logits / rollout_policy)
against the CPU yardstick tests/policy_reference.py - the definition of include/tiler_slider_policy.h on NumPy and the oracle -,
against the environment's own one-hot planes, and against the shipped rollout(policy="given") and step()."""
import ctypes as C

import numpy as np
import pytest

import policy_reference as pref
import rollout_reference as rref
from table_harness import GUARD, guarded as _guarded, payload as _payload

pytestmark = pytest.mark.gpu

ALL_LOGS = ("act", "flags", "pos", "logits")
STRICT, AUTORESET = 0, 1


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


def _policy(torch, env, mlp):
    from tiler_slider_amd import MlpPolicy
    return MlpPolicy(*(torch.from_numpy(a).to(env.device) for a in mlp))


def _features(S, T, Tt, mc):
    return (1 + T + Tt if mc else 3) * S * S


def _levels(oracle, S, T, Tt, K, n, seed=0x6171):
    """n random levels of any shape: the reference's seeded levels where obstacles, tiles and targets fit side by side, else tiles
    and obstacles drawn apart from the targets (which may then lie under tiles)."""
    if T == Tt and 2 * T + K <= S * S:
        return oracle.generate_mt19937(S, T, T, K, np.arange(2000, 2000 + n, dtype=np.uint32))
    blk, init, _ = oracle.generate(S, T, 0, K, n, seed=seed)
    _, _, tgt = oracle.generate(S, 0, Tt, 0, n, seed=seed + 1)
    return blk, init, tgt


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(got, env, want, ctx, outputs=pref.OUTPUTS, state=True):
    """Every output of a Rollout, and the environment's state after an advancing call, against the yardstick's dict; the logits
    bit for bit."""
    for name in outputs:
        t = getattr(got, name)
        assert t is not None, (ctx, name)
        g, w = t.cpu().numpy(), want[name]
        if name == "logits_log":
            g, w = _bits(g), _bits(w)
        np.testing.assert_array_equal(g, w, err_msg=f"{ctx}: {name}")
    if state:
        for name in ("pos", "step_count", "done"):
            np.testing.assert_array_equal(getattr(env, "_" + name).cpu().numpy(), want[name], err_msg=f"{ctx}: {name} after the call")
        np.testing.assert_array_equal(env._flags.cpu().numpy(), want["flags"], err_msg=f"{ctx}: the environment's flag byte")


# ---------------------------------------------------------------------------------------------- 1. logits against the planes
# (S, T, Tt, obstacles, multi colour, what)
LOGIT_SHAPES = ((4, 2, 2, 2, False, ""), (5, 3, 3, 3, True, ""), (8, 2, 2, 10, False, ""), (8, 2, 2, 10, True, ""), (8, 8, 8, 6, True, "gather"),
                (3, 4, 4, 1, False, ""), (3, 4, 4, 1, True, ""), (1, 1, 1, 0, True, ""), (1, 1, 1, 0, False, ""), (4, 3, 2, 2, True, ""),
                (5, 2, 4, 3, False, ""), (4, 3, 3, 2, False, "repeated targets"), (4, 0, 0, 3, True, ""), (5, 0, 2, 3, False, ""),
                (4, 2, 2, 2, False, "beyond"), (8, 3, 3, 10, True, "beyond"))


@pytest.mark.parametrize("S,T,Tt,K,mc,what", LOGIT_SHAPES)
def test_logits_lie_within_the_float32_bound_of_the_networks_answer_on_the_environments_own_planes(torch_cuda, oracle, S, T, Tt, K, mc, what):
    """257 boards (a ragged last wave) a few random steps into their episodes, Gaussian weights, H in {1, 7, 16, 64}:
    relu(encode_onehot().flatten(1) @ w1^T + b1) @ w2^T + b2 in float64 torch, and the yardstick's bound around it."""
    torch = torch_cuda
    from tiler_slider_amd import _policy_cabi as pc
    n, Cc = 257, S * S
    rng = np.random.default_rng(S * 1000 + T * 10 + Tt + mc)
    blk, init, tgt = _levels(oracle, S, T, Tt, K, n)
    if what == "repeated targets":
        tgt[2] = tgt[0]
    raw_init, raw_tgt = init.copy(), tgt.copy()
    if what == "beyond":   # ids S*S .. 255: clamped to S*S - 1, as the step kernels and ts_encode_onehot clamp them
        some = rng.random(n) < 0.4
        raw_init[0, some] = rng.integers(Cc, 256, int(some.sum()))
        raw_tgt[Tt - 1, rng.random(n) < 0.3] = 255
    env = _env(S, mc, blk, raw_init, raw_tgt, 50, AUTORESET)
    if what == "beyond":
        _put(env, "_pos", raw_init)
    elif T:
        env.rollout(3, "random", seed=S)
    x = env.encode_onehot().flatten(1)
    D = _features(S, T, Tt, mc)
    assert x.shape == (n, D)
    xs = x.cpu().numpy()
    assert set(np.unique(xs)) <= {0.0, 1.0}
    if what == "repeated targets":
        assert (xs[:, 2 * Cc:].sum(axis=1) == np.array([len(set(c)) for c in tgt.T])).all() and (xs[:, 2 * Cc:].sum(axis=1) < Tt).any()
    for H in (1, 7, 16, 64):
        d = pc.describe_policy_logits(env._dims, H)
        fits = T > 0 and 16 * H + 16 + ((H * (T if mc else 1) * Cc * 4 + 15) & ~15) + 256 * H <= 65536   # beside one wave's hs and the second layer
        assert d["weights_in_lds"] == int(fits) and (what != "gather" or fits == (H <= 28)), (H, d)
        mlp = pref.random_mlp(rng, D, H)
        w1, b1, w2, b2 = (torch.from_numpy(a).to(env.device).double() for a in mlp)
        z = torch.relu(x.double() @ w1.T + b1) @ w2.T + b2
        z_ref, bound = pref.logits64(xs, mlp)
        assert np.abs(z.cpu().numpy() - z_ref).max() <= 1e-9 * max(1.0, np.abs(z_ref).max())
        got = env.policy_logits(_policy(torch, env, mlp))
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, 4)
        err = np.abs(got.cpu().numpy().astype(np.float64) - z.cpu().numpy())
        print(f"{S}x{S} T={T} Tt={Tt} mc={mc} {what} H={H}: worst error / bound {float((err / bound).max()):.3f}, worst error {err.max():.3g}")
        assert (err <= bound).all(), (H, float((err / bound).max()))
    env.close()


# ---------------------------------------------------------------------------------------------- 2. exact, free-running
@pytest.mark.parametrize("case", range(len(pref.EXACT_CASES)))
def test_integer_weights_free_running_equal_the_numpy_loop_byte_for_byte(torch_cuda, oracle, case):
    torch = torch_cuda
    S, T, K, mc, n, max_steps, steps, eps, H, mode, _ = pref.EXACT_CASES[case]
    (blk, init, tgt), mlp, want = pref.exact_case(oracle, case)
    env = _env(S, mc, blk, init, tgt, max_steps, mode)
    got = env.rollout_policy(steps, _policy(torch, env, mlp), select="greedy", epsilon=eps, seed=0x9011C7 + case, step_index=case * 100,
                             board_offset=case * 31, log=ALL_LOGS)
    _check(got, env, want, ("exact", case))
    assert got.steps == steps and tuple(got.logits_log.shape) == (steps, n, 4)


# ---------------------------------------------------------------------------------------------- 3. teacher-forced
# (S, T, obstacles, multi colour, boards, max_steps, steps, H, mode)
FORCED = ((4, 2, 2, False, 3000, 8, 30, 64, AUTORESET), (5, 3, 3, True, 2000, 12, 30, 16, AUTORESET), (8, 8, 6, True, 600, 10, 12, 64, AUTORESET),
          (4, 2, 2, True, 3000, 8, 30, 7, STRICT))
SLACK, CAP = 2.0 ** -16, 1e-3


@pytest.mark.parametrize("select", ("greedy", "sample"))
@pytest.mark.parametrize("case", range(len(FORCED)))
def test_gaussian_weights_teacher_forced(torch_cuda, oracle, case, select):
    """Every logged logit within the bound of the float64 logits of the board before its step (rebuilt from the cells), every
    logged action the rule applied to the kernel's own logged logits and the restated draw (SAMPLE: except within 2**-16 of a
    boundary of the float64 CDF, at most 1 in 1,000), and the logged actions replayed through rollout(policy="given") on a twin
    leave byte-equal state, statistics and logs."""
    torch = torch_cuda
    S, T, K, mc, n, max_steps, steps, H, mode = FORCED[case]
    sel = pref.GREEDY if select == "greedy" else pref.SAMPLE
    eps, seed, step_index, offset = 0.1, 0x7EAC + case, 17, 5
    blk, init, tgt = _levels(oracle, S, T, T, K, n)
    mlp = pref.random_mlp(np.random.default_rng(50 + case), _features(S, T, T, mc), H)
    env, twin = _env(S, mc, blk, init, tgt, max_steps, mode), _env(S, mc, blk, init, tgt, max_steps, mode)
    pos0 = env._pos.cpu().numpy().copy()
    got = env.rollout_policy(steps, _policy(torch, env, mlp), select=select, epsilon=eps, seed=seed, step_index=step_index, board_offset=offset,
                             log=ALL_LOGS)
    logits_log, act_log, pos_log = got.logits_log.cpu().numpy(), got.act_log.cpu().numpy(), got.pos_log.cpu().numpy()
    b = oracle.OracleBatch(S, mc, max_steps, blk, init, tgt)
    b.reset()
    left_out = explored = 0
    worst = 0.0
    for k in range(steps):
        b.pos[...] = pos0 if k == 0 else pos_log[k - 1]
        z, bound = pref.board_logits(b, mlp)
        err = np.abs(logits_log[k].astype(np.float64) - z)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (k, float((err / bound).max()))
        r = rref.draws(n, seed, step_index + k, offset)
        a, explore = pref.choose(logits_log[k], r, sel, rref.threshold_of(eps))
        explored += int(explore.sum())
        differ = a != act_log[k]
        if sel == pref.GREEDY:
            assert not differ.any(), (k, int(differ.sum()))
        else:
            near = ~explore & (pref.sample_margin(logits_log[k], r) < SLACK)
            assert not (differ & ~near).any(), (k, int((differ & ~near).sum()))
            left_out += int(near.sum())
        assert (act_log[k] <= 3).all()
    print(f"forced case {case} {select}: worst logit error / bound {worst:.3f}, explored {explored / (n * steps):.3f}, "
          f"left out near a CDF boundary {left_out / (n * steps):.2e}")
    assert left_out <= CAP * n * steps and explored >= 0.01 * n * steps
    assert len(np.unique(act_log)) == 4
    replay = twin.rollout(steps, "given", actions=got.act_log, log=("act", "flags", "pos"))
    for name in rref.OUTPUTS:
        assert torch.equal(getattr(got, name), getattr(replay, name)), name
    for name in ("_pos", "_step_count", "_done", "_flags"):
        assert torch.equal(getattr(env, name), getattr(twin, name)), name
    flags_log = got.flags_log.cpu().numpy()
    assert (flags_log & rref.FLAG_TIMEOUT).any() and ((flags_log & (rref.FLAG_AUTORESET if mode == AUTORESET else rref.FLAG_STEPPED_DONE)) != 0).any()


# ---------------------------------------------------------------------------------------------- 4. sampling frequencies
def test_sample_draws_the_softmax_frequencies(torch_cuda, oracle):
    """Zero w1 and w2, b2 = log([0.1, 0.2, 0.3, 0.4]): over 2**20 boards x 8 steps every action's frequency lies within five
    standard deviations of its probability."""
    torch = torch_cuda
    S, T, n, steps, H = 4, 2, 1 << 20, 8, 16
    p = np.array([0.1, 0.2, 0.3, 0.4])
    blk, init, tgt = oracle.generate(S, T, T, 2, n, seed=0xF4E0)
    env = _env(S, False, blk, init, tgt, 20, AUTORESET)
    D = _features(S, T, T, False)
    mlp = (np.zeros((H, D), np.float32), np.zeros(H, np.float32), np.zeros((4, H), np.float32), np.log(p).astype(np.float32))
    got = env.rollout_policy(steps, _policy(torch, env, mlp), select="sample", seed=0xF4E0, log=("act",), stats=False)
    counts = torch.bincount(got.act_log.flatten().to(torch.int64), minlength=4).cpu().numpy()
    total = n * steps
    assert counts.sum() == total and len(counts) == 4
    freq = counts / total
    tol = 5 * np.sqrt(p * (1 - p) / total)
    print("frequencies", freq.tolist(), "tolerance", tol.tolist())
    assert (np.abs(freq - p) <= tol).all(), (freq, p, tol)


# ---------------------------------------------------------------------------------------------- 5. advance
def test_advance_false_leaves_the_environment_untouched_and_true_equals_a_twin_stepped(torch_cuda, oracle):
    torch = torch_cuda
    S, T, K, mc, n, max_steps, steps, H = 5, 2, 3, False, 1500, 7, 25, 16
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    env = _env(S, mc, blk, init, tgt, max_steps, AUTORESET, obs_dtype="float32")
    twin = _env(S, mc, blk, init, tgt, max_steps, AUTORESET, obs_dtype="float32")
    policy = _policy(torch, env, pref.random_mlp(np.random.default_rng(5), _features(S, T, T, mc), H))
    for e in (env, twin):   # somewhere in the middle of their episodes
        e.rollout(5, "random", seed=3)
    names = ("_pos", "_step_count", "_done", "_flags", "_obs", "_init", "_tgt", "_blk")
    before = {k: getattr(env, k).clone() for k in names}
    for select in ("greedy", "sample"):
        play = env.rollout_policy(steps, policy, select=select, epsilon=0.2, seed=9, advance=False, log=ALL_LOGS)
        for k in names:
            assert torch.equal(getattr(env, k), before[k]), (select, k)
        saved = {k: getattr(twin, k).clone() for k in ("_pos", "_step_count", "_done", "_flags")}
        adv = twin.rollout_policy(steps, policy, select=select, epsilon=0.2, seed=9, log=ALL_LOGS)
        for name in pref.OUTPUTS:
            assert torch.equal(getattr(play, name), getattr(adv, name)), (select, name)
        assert not torch.equal(twin._pos, saved["_pos"])
        assert torch.equal(twin._obs, twin.encode(torch.empty_like(twin._obs)))      # the observation was re-encoded
        assert torch.equal(twin._flags, adv.flags)
        # a third environment stepped with the logged actions ends where the advancing call ended
        third = _env(S, mc, blk, init, tgt, max_steps, AUTORESET, obs_dtype="float32")
        for k, v in saved.items():
            getattr(third, k).copy_(v)
        for k in range(steps):
            obs, _, info = third.step(adv.act_log[k])
            assert torch.equal(info["flags"], adv.flags_log[k]), (select, k)
        for k in ("_pos", "_step_count", "_done", "_flags"):
            assert torch.equal(getattr(third, k), getattr(twin, k)), (select, k)
        assert torch.equal(obs, twin._obs)
        for k, v in saved.items():   # the twin goes back to where the playout started
            getattr(twin, k).copy_(v)
    only = env.rollout_policy(steps, policy, seed=9, advance=False, stats=("wins", "reward_sum"))
    assert only.finished is None and only.flags is None and only.act_log is None and only.logits_log is None and only.wins is not None
    none = env.rollout_policy(steps, policy, seed=9, advance=False, stats=False)
    assert all(getattr(none, f) is None for f in pref.OUTPUTS)
    for k in names:
        assert torch.equal(getattr(env, k), before[k]), k
    # the host's checks
    from tiler_slider_amd import MlpPolicy
    w = [torch.zeros(s, device=env.device) for s in ((H, _features(S, T, T, mc)), (H,), (4, H), (4,))]
    with pytest.raises(TypeError):
        env.rollout_policy(3, "random")
    with pytest.raises(TypeError):
        MlpPolicy(w[0].double(), *w[1:])
    with pytest.raises(ValueError):
        MlpPolicy(w[0], w[1], w[2].t().contiguous(), w[3])
    with pytest.raises(ValueError):
        MlpPolicy(torch.zeros((65, 75), device=env.device), torch.zeros(65, device=env.device), torch.zeros((4, 65), device=env.device), w[3])
    with pytest.raises(ValueError):
        MlpPolicy(*(t.cpu() for t in w))
    with pytest.raises(ValueError):
        env.policy_logits(MlpPolicy(torch.zeros((H, 74), device=env.device), *w[1:]))
    with pytest.raises(ValueError):
        env.rollout_policy(3, policy, select="argmax")
    with pytest.raises(ValueError):
        env.rollout_policy(70000, policy)
    with pytest.raises(ValueError):
        env.rollout_policy(3, policy, epsilon=1.5)
    with pytest.raises(ValueError):
        env.rollout_policy(3, policy, log=("values",))
    big = _env(9, False, *oracle.generate(9, 2, 2, 3, 4, seed=1))
    with pytest.raises(ValueError, match="8x8"):
        big.rollout_policy(3, MlpPolicy(torch.zeros((H, 243), device=env.device), *w[1:]))
    l1, l2 = torch.nn.Linear(_features(S, T, T, mc), H).to(env.device), torch.nn.Linear(H, 4).to(env.device)
    net = MlpPolicy.from_linear(l1, l2)
    with torch.no_grad():
        z = l2(torch.relu(l1(env.encode_onehot().flatten(1))))
    assert torch.allclose(env.policy_logits(net), z, rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------------------------------------- 6. the raw C-ABI into guarded memory
@pytest.mark.parametrize("select", (pref.GREEDY, pref.SAMPLE))
def test_raw_calls_into_guarded_memory(torch_cuda, oracle, select):
    """Every buffer of a call between 256 guard bytes, outputs prefilled with the complement of the expected bytes: no guard byte
    changes, outputs not asked for keep their fill, write_state = 0 touches no state byte, steps = 0 writes nothing.  Integer
    weights whose logits are multiples of 128 (exp is exactly 0 or 1), so that SAMPLE is exact as well."""
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _policy_cabi as pc
    S, T, K, mc, n, max_steps, steps, H = 5, 2, 3, True, 257, 6, 17, 16
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    mlp = pref.random_mlp(np.random.default_rng(select), _features(S, T, T, mc), H, "int128")
    env = _env(S, mc, blk, init, tgt, max_steps, AUTORESET)
    start = rref.rollout(oracle, S, mc, max_steps, blk, init, tgt, 4, rref.RANDOM, AUTORESET, seed=1)     # somewhere mid-episode
    kw = dict(pos=start["pos"], step_count=start["step_count"], done=start["done"])
    want = pref.rollout(oracle, S, mc, max_steps, blk, init, tgt, mlp, steps, select, AUTORESET, threshold=rref.threshold_of(0.3), seed=21,
                        step_index=3, exact32=True, **kw)
    assert len(np.unique(want["act_log"])) >= 3
    dev = env.device
    net = [_guarded(torch, dev, a) for a in (np.ascontiguousarray(mlp[0].T), mlp[1], np.ascontiguousarray(mlp[2].T), mlp[3])]
    comp = lambda a: (~_bits(a)).view(np.float32) if a.dtype == np.float32 else ~a

    def fresh():
        bufs = {"pos": start["pos"], "init": init, "tgt": tgt, "blk": blk, "step_count": start["step_count"], "done": start["done"]}
        bufs.update({f: comp(want[f]) for f in pref.OUTPUTS})
        bufs["logits"] = comp(want["logits_log"][0])
        return {k: _guarded(torch, dev, v) for k, v in bufs.items()}

    def call(bufs, ask, steps=steps, write_state=1):
        st = _cabi.State(*(bufs[k].data_ptr() + GUARD for k in ("pos", "init", "tgt", "blk", "step_count", "done")), None)
        m = pc.Mlp(*(t.data_ptr() + GUARD for t in net), H, 0)
        out = pc.PolicyOut(*(bufs[f].data_ptr() + GUARD if f in ask else None for f in pc.OUT_FIELDS))
        cfg = pc.PolicyCfg(steps, AUTORESET, select, write_state, 21, 3, 0, rref.threshold_of(0.3))
        return pc.lib().ts_policy_rollout(C.byref(env._dims), C.byref(st), C.byref(m), C.byref(cfg), C.byref(out),
                                          torch.cuda.current_stream(dev).cuda_stream)

    def read(bufs, name, like):
        a = _payload(bufs[name], like.dtype, like.shape)
        return _bits(a) if like.dtype == np.float32 else a

    def same(bufs, f, expect):
        np.testing.assert_array_equal(read(bufs, f, expect), _bits(expect) if expect.dtype == np.float32 else expect, err_msg=f)

    # everything asked for
    bufs = fresh()
    assert call(bufs, pref.OUTPUTS) == 0
    for f in pref.OUTPUTS + ("pos", "step_count", "done"):
        same(bufs, f, want[f])
    for f, v in (("init", init), ("tgt", tgt), ("blk", blk)):
        same(bufs, f, v)
    for t in net:
        _payload(t, np.uint8, (t.numel() - 2 * GUARD,))
    # a subset, no state written: the rest keeps its fill, the state its bytes
    for ask in (("wins", "pos_log"), ("logits_log",), ("flags",), ("reward_sum", "act_log", "first_win")):
        bufs = fresh()
        assert call(bufs, ask, write_state=0) == 0
        for f in pref.OUTPUTS:
            same(bufs, f, want[f] if f in ask else comp(want[f]))
        for f in ("pos", "step_count", "done"):
            same(bufs, f, start[f])
    # no output, the state alone
    bufs = fresh()
    assert call(bufs, ()) == 0
    for f in pref.OUTPUTS:
        same(bufs, f, comp(want[f]))
    for f in ("pos", "step_count", "done"):
        same(bufs, f, want[f])
    # steps = 0: nothing at all
    bufs = fresh()
    assert call(bufs, pref.OUTPUTS, steps=0) == 0
    for f in pref.OUTPUTS:
        same(bufs, f, comp(want[f]))
    for f in ("pos", "step_count", "done"):
        same(bufs, f, start[f])
    # the logits call: its output and nothing else
    bufs = fresh()
    st = _cabi.State(*(bufs[k].data_ptr() + GUARD for k in ("pos", "init", "tgt", "blk")), None, None, None)
    m = pc.Mlp(*(t.data_ptr() + GUARD for t in net), H, 0)
    assert pc.lib().ts_policy_logits(C.byref(env._dims), C.byref(st), C.byref(m), bufs["logits"].data_ptr() + GUARD,
                                     torch.cuda.current_stream(dev).cuda_stream) == 0
    same(bufs, "logits", want["logits_log"][0])
    for f in pref.OUTPUTS:
        same(bufs, f, comp(want[f]))
    for f in ("pos", "step_count", "done"):
        same(bufs, f, start[f])


# ---------------------------------------------------------------------------------------------- 7. every compiled kernel at occupancy
OCC_WAVES, OCC_STEPS, OCC_MAX_STEPS, OCC_H = 4096, 4, 3, 64


@pytest.mark.parametrize("name", sorted(pref.OCCUPANCY_CASES))
def test_every_compiled_policy_kernel_at_occupancy(torch_cuda, oracle, name):
    """Every kernel of the policy library at 4,096 waves and a ragged last one, 64 hidden units, on 128 distinct levels in turn,
    exactly: integer weights, the second layer scaled by 128 so that SAMPLE is exact too (exp is 0 or 1)."""
    torch = torch_cuda
    from tiler_slider_amd import _policy_cabi as pc
    S, T, K, select = pref.OCCUPANCY_CASES[name]
    distinct, n = 128, OCC_WAVES * 64 - 3
    level = (np.arange(n) % distinct).astype(np.int32)
    mc = S % 2 == 0
    if S == 1:
        blk, init, tgt = np.zeros((1, distinct), np.uint32), np.zeros((1, distinct), np.uint8), np.zeros((1 if mc else 0, distinct), np.uint8)
    else:
        blk, init, tgt = _levels(oracle, S, T, T, K, distinct, seed=0x50F7)
    tile = lambda a: np.ascontiguousarray(a[:, level])
    blk, init, tgt = tile(blk), tile(init), tile(tgt)
    Tt = tgt.shape[0]
    mlp = pref.random_mlp(np.random.default_rng(S), _features(S, T, Tt, mc), OCC_H, "int128")
    env = _env(S, mc, blk, init, tgt, OCC_MAX_STEPS, AUTORESET)
    policy = _policy(torch, env, mlp)
    if select is None:
        d = pc.describe_policy_logits(env._dims, OCC_H)
        assert d["name"] == name and d["blocks"] * (d["threads_per_block"] // 64) >= OCC_WAVES
        if T:
            env.rollout(2, "random", seed=S)
        b = oracle.OracleBatch(S, mc, OCC_MAX_STEPS, blk, init, tgt)
        b.pos[...] = env._pos.cpu().numpy()
        want = pref.logits_exact32(b.encode_onehot().reshape(n, -1), mlp)
        np.testing.assert_array_equal(_bits(env.policy_logits(policy).cpu().numpy()), _bits(want), err_msg=name)
    else:
        cfg = pc.PolicyCfg(OCC_STEPS, AUTORESET, select, 1, 0, 0, 0, 0)
        d = pc.describe_policy_rollout(env._dims, OCC_H, cfg, 0x3ff)
        assert d["name"] == name and d["blocks"] * (d["threads_per_block"] // 64) >= OCC_WAVES
        want = pref.rollout(oracle, S, mc, OCC_MAX_STEPS, blk, init, tgt, mlp, OCC_STEPS, select, AUTORESET, threshold=rref.threshold_of(0.25),
                            seed=S, exact32=True)
        assert want["timed_out"].any() and want["reset"].any()
        got = env.rollout_policy(OCC_STEPS, policy, select=("greedy", "sample")[select], epsilon=0.25, seed=S, log=ALL_LOGS)
        _check(got, env, want, name)
    env.close()


def test_a_quarter_of_a_million_boards_for_32_steps(torch_cuda, oracle):
    torch = torch_cuda
    S, T, K, mc, n, max_steps, steps, H = 4, 2, 2, False, 262144, 20, 32, 16
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    mlp = pref.random_mlp(np.random.default_rng(1), _features(S, T, T, mc), H, "int")
    want = pref.rollout(oracle, S, mc, max_steps, blk, init, tgt, mlp, steps, pref.GREEDY, AUTORESET, threshold=rref.threshold_of(0.1),
                        seed=0x5CA1E, exact32=True)
    assert want["won"].mean() > 0.01 and want["timed_out"].any() and want["reset"].any()
    env = _env(S, mc, blk, init, tgt, max_steps, AUTORESET)
    got = env.rollout_policy(steps, _policy(torch, env, mlp), select="greedy", epsilon=0.1, seed=0x5CA1E, log=ALL_LOGS)
    _check(got, env, want, "scale")


# ---------------------------------------------------------------------------------------------- 8. streams
def test_a_policy_rollout_on_a_stream_of_its_own_ordered_after_a_step(torch_cuda, oracle):
    """2**18 boards, one extra stream, no host synchronisation until the end: the rollout is enqueued while the step still runs.
    A launch that ignored its `stream` argument would play from cells the step has not written yet."""
    torch = torch_cuda
    S, T, K, mc, n, max_steps, steps, H = 4, 2, 2, False, 1 << 18, 30, 12, 16
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    mlp = pref.random_mlp(np.random.default_rng(2), _features(S, T, T, mc), H, "int")
    act = oracle.fill_actions(n, seed=0x57EA, step_index=0)
    twin = oracle.OracleBatch(S, mc, max_steps, blk, init, tgt)
    twin.reset()
    twin.step(act, mode=AUTORESET, obs=False)
    kw = dict(threshold=rref.threshold_of(0.1), seed=8, exact32=True)
    want = pref.rollout(oracle, S, mc, max_steps, blk, init, tgt, mlp, steps, pref.GREEDY, AUTORESET, pos=twin.pos, step_count=twin.step_count,
                        done=twin.done, **kw)
    from_start = pref.rollout(oracle, S, mc, max_steps, blk, init, tgt, mlp, steps, pref.GREEDY, AUTORESET, **kw)
    assert (want["pos"] != from_start["pos"]).any(axis=0).sum() >= 1000      # the step matters
    env = _env(S, mc, blk, init, tgt, max_steps, AUTORESET)
    policy = _policy(torch, env, mlp)
    actions = torch.from_numpy(act).to(env.device)
    side = torch.cuda.Stream(device=env.device)
    assert side.cuda_stream != torch.cuda.current_stream(env.device).cuda_stream
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        env.step(actions)
        got = env.rollout_policy(steps, policy, select="greedy", epsilon=0.1, seed=8, log=ALL_LOGS)
    side.synchronize()
    _check(got, env, want, "stream")
