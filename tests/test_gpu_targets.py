"""The trajectory targets on the GPU (lib/libtiler_slider_targets.so, VecTilerSliderEnv.trajectory_returns / trajectory_labels)
against the CPU yardstick tests/targets_reference.py - the definitions of include/tiler_slider_targets.h on NumPy and the CPU
oracle -, against the rollout's own reward_sum, and against a twin environment stepped through the logged actions."""
import ctypes as C

import numpy as np
import pytest

import table_reference as tref
import targets_reference as gr
from table_harness import GUARD, guarded as _guarded, payload as _payload

pytestmark = pytest.mark.gpu

STRICT, AUTORESET = 0, 1
KS = (1, 2, 5, 24)


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


def _case_env(c):
    return _env(c["S"], c["mc"], c["blk"], c["init"], c["tgt"], c["max_steps"], c["mode"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _log(torch, env, first=None, pos_log=None, flags_log=None):
    """A Rollout that holds given logs (numpy, or None), on the environment's device."""
    from tiler_slider_amd import Rollout
    put = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(env.device)
    steps = next(a for a in (flags_log, pos_log) if a is not None).shape[0]
    return Rollout(steps, start_pos=put(first), pos_log=put(pos_log), flags_log=put(flags_log))


def _weights(w):
    from tiler_slider_amd import RewardWeights
    return RewardWeights(*w)


def _returns(torch, env, c, K, gamma, lam, w, V=None, VL=None, **kw):
    """trajectory_returns on the first K steps of case c's log (a prefix of a log is a log), as numpy."""
    log = _log(torch, env, c["first"], c["log"]["pos_log"][:K], c["log"]["flags_log"][:K])
    dev = env.device
    got = env.trajectory_returns(log, gamma, lam, None if V is None else torch.from_numpy(V[:K]).to(dev),
                                 None if VL is None else torch.from_numpy(VL).to(dev), _weights(w), **kw)
    assert got.mask.dtype == torch.bool and all(t.dtype == torch.float32 and tuple(t.shape) == (K, c["n"]) for t in got[:3])
    return {k: t.cpu().numpy() for k, t in zip(("reward", "adv", "ret", "mask"), got)}


def _want(c, K, gamma, lam, w, V=None, VL=None, exact=False):
    return gr.returns64(c["log"]["flags_log"][:K], c["m_before"][:K], c["m_after"][:K], None if V is None else V[:K], VL, gamma, lam, w, exact=exact)


def _assert_exact(got, want, what):
    for key in ("reward", "adv", "ret"):
        np.testing.assert_array_equal(_bits(got[key]), _bits(want[key].astype(np.float32)), err_msg=f"{what}: {key}")
    np.testing.assert_array_equal(got["mask"], want["mask"] != 0, err_msg=f"{what}: mask")


# ---------------------------------------------------------------------------------------------- 1. returns: exact
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", ("auto", "strict", "given"))
def test_integer_returns_equal_the_yardstick_bit_for_bit(torch_cuda, oracle, name, K):
    """Integer weights (every one set), integer values in -8 .. 8, gamma 1 and 0.5, lambda 1, max_steps 6: the yardstick asserts
    that every intermediate is a float32, so every order of evaluation gives these bits.  Auto-reset (episodes end and restart
    inside the log), strict (boards stand done) and given actions with bytes above 3; with and without last_value."""
    c = gr.trajectory(oracle, name)
    env = _case_env(c)
    V, VL = gr.integer_values(c["K"], c["n"])
    for gamma in (1.0, 0.5):
        for last in (VL, None):
            want = _want(c, K, gamma, 1.0, gr.INT_WEIGHTS, V, last, exact=True)
            _assert_exact(_returns(torch_cuda, env, c, K, gamma, 1.0, gr.INT_WEIGHTS, V, last), want, f"{name} K={K} gamma={gamma}")
            assert K < 5 or (0 < want["mask"].mean() < 1 and np.abs(want["adv"]).max() > 0)
    if K > 1 and not (name == "strict" and K > 6):   # last_value matters wherever the last step neither ends an episode nor is void
        a, b = (_want(c, K, 1.0, 1.0, gr.INT_WEIGHTS, V, last)["adv"] for last in (VL, None))
        assert (a != b).any()
    env.close()


@pytest.mark.parametrize("field", gr.Weights._fields)
def test_each_weight_alone(torch_cuda, oracle, field):
    """One weight 3, the others 0 (the default's win = 1 included), no values, gamma = 1: reward is 3 times the weight's own term
    and nothing else."""
    c = gr.trajectory(oracle, "auto")
    env = _case_env(c)
    w = gr.Weights(**{**dict.fromkeys(gr.Weights._fields, 0.0), field: 3.0})
    got, want = _returns(torch_cuda, env, c, 24, 1.0, 1.0, w), _want(c, 24, 1.0, 1.0, w, exact=True)
    _assert_exact(got, want, field)
    f, live = c["log"]["flags_log"], want["mask"] != 0
    term = {"step": np.ones_like(f, np.float64), "win": (f & gr.FLAG_SUCCESS) != 0, "timeout": (f & gr.FLAG_TIMEOUT) != 0,
            "invalid": (f & gr.FLAG_INVALID_MOVE) != 0, "dist": c["m_after"], "progress": c["m_after"] - c["m_before"]}[field]
    np.testing.assert_array_equal(got["reward"], np.where(live, 3.0 * term, 0.0).astype(np.float32))
    assert (got["reward"] != 0).any()
    env.close()


# ---------------------------------------------------------------------------------------------- 2. returns: the bound
@pytest.mark.parametrize("K", KS)
def test_gaussian_returns_lie_within_the_bound(torch_cuda, oracle, K):
    """gamma = 0.97, lambda = 0.9, Gaussian values and last_value, every weight set: |got - float64| <= gamma(3 (K - k) + 10) Abar_k
    on every sample (targets_reference's docstring derives it), void steps exactly 0."""
    c = gr.trajectory(oracle, "auto")
    env = _case_env(c)
    V, VL = gr.gaussian_values(c["K"], c["n"])
    w = gr.Weights(step=-0.01, win=1.0, timeout=-0.5, invalid=-0.1, dist=0.05, progress=0.25)
    got, want = _returns(torch_cuda, env, c, K, 0.97, 0.9, w, V, VL), _want(c, K, 0.97, 0.9, w, V, VL)
    live = want["mask"] != 0
    np.testing.assert_array_equal(got["mask"], live)
    for key in ("reward", "adv", "ret"):
        err = np.abs(got[key].astype(np.float64) - want[key])
        print(f"K={K} {key}: worst error / bound {float((err[live] / want['bound'][live]).max()):.3f}")
        assert (err <= want["bound"]).all(), key
        assert (got[key][~live] == 0).all(), key
    env.close()


# ---------------------------------------------------------------------------------------------- 3. returns: against the rollout itself
@pytest.mark.parametrize("mode", (STRICT, AUTORESET))
def test_the_distance_reward_sums_to_the_rollouts_own_reward_sum(torch_cuda, oracle, mode):
    """w_dist = 1 alone, gamma = lambda = 1, no values, on the GPU's own rollout: the rewards of the played steps plus m() of the
    void steps' cells are the rollout's reward_sum, exactly - which holds the copied Manhattan reward to ts_rollout.hip's.  The
    form "ret[0] plus the void steps' m is reward_sum" is asserted in strict mode only: ret[0] stops at the first episode end, and
    only there does a board's one episode end once and the board then stand; in auto-reset mode episodes restart inside the
    log, so the rewards are summed over all steps instead."""
    torch = torch_cuda
    c = gr.trajectory(oracle, "strict" if mode == STRICT else "auto")
    env = _case_env(c)
    table = env.build_table()
    out = env.rollout(c["K"], "table", table=table, epsilon=c["eps"], seed=c["seed"], log=("start", "pos", "flags"))
    np.testing.assert_array_equal(out.flags_log.cpu().numpy(), c["log"]["flags_log"])
    from tiler_slider_amd import RewardWeights
    got = env.trajectory_returns(out, 1.0, 1.0, reward=RewardWeights(win=0.0, dist=1.0))
    void_m = np.where(c["log"]["flags_log"] & gr.VOID, c["m_after"], 0).sum(axis=0)
    assert (void_m < 0).any()
    reward_sum = out.reward_sum.cpu().numpy()
    np.testing.assert_array_equal(got.reward.cpu().numpy().astype(np.int64).sum(axis=0) + void_m, reward_sum)
    if mode == STRICT:
        np.testing.assert_array_equal(got.ret[0].cpu().numpy().astype(np.int64) + void_m, reward_sum)
        assert torch.equal(got.ret, got.adv)
    env.close()


# ---------------------------------------------------------------------------------------------- 4. returns: the inputs' forms
def test_values_in_place_from_a_logits_tensor_and_the_api_refusals(torch_cuda, oracle):
    """Column 0 (and column 2) of a [K, N, 4] tensor read in place with stride 4 gives the bits of a contiguous copy; values that
    require grad are detached; other layouts, dtypes, shapes and a rollout without the logs it needs raise."""
    torch = torch_cuda
    from tiler_slider_amd import RewardWeights, Rollout
    c = gr.trajectory(oracle, "auto")
    env = _case_env(c)
    K, n, dev = c["K"], c["n"], env.device
    log = _log(torch, env, c["first"], c["log"]["pos_log"], c["log"]["flags_log"])
    z = torch.randn((K, n, 4), device=dev, generator=torch.Generator(device=dev).manual_seed(1)).requires_grad_(True)
    w = RewardWeights(step=-0.01, win=1.0, dist=0.05, progress=0.25)
    for col in (0, 2):
        view = z[..., col]
        assert tuple(view.stride()) == (4 * n, 4)
        a = env.trajectory_returns(log, 0.97, 0.9, view, reward=w)
        b = env.trajectory_returns(log, 0.97, 0.9, view.detach().contiguous(), reward=w)
        for x, y in zip(a, b):
            assert torch.equal(x, y) and not x.requires_grad
    V, _ = gr.gaussian_values(K, n)
    with pytest.raises(ValueError):
        env.trajectory_returns(log, values=z[:, :, :2].sum(-1).t().contiguous().t())      # [K, N] with strides (1, K)
    with pytest.raises(ValueError):
        env.trajectory_returns(log, values=z.detach().double()[..., 0])
    with pytest.raises(ValueError):
        env.trajectory_returns(log, values=z.detach()[:-1, :, 0])
    with pytest.raises(ValueError):
        env.trajectory_returns(log, last_value=torch.zeros(n + 1, device=dev))
    with pytest.raises(ValueError):
        env.trajectory_returns(log, gamma=1.5)
    with pytest.raises(TypeError):
        env.trajectory_returns(log, reward=(0, 1, 0, 0, 0, 0))
    with pytest.raises(TypeError):
        env.trajectory_returns(None)
    flags_only = Rollout(K, flags_log=log.flags_log)
    assert torch.equal(env.trajectory_returns(flags_only).reward, ((log.flags_log & gr.FLAG_SUCCESS) != 0).float())   # the default: 1 for a win
    with pytest.raises(ValueError):
        env.trajectory_returns(flags_only, reward=RewardWeights(dist=1.0))            # needs pos_log
    with pytest.raises(ValueError):
        env.trajectory_returns(Rollout(K, flags_log=log.flags_log, pos_log=log.pos_log), reward=RewardWeights(progress=1.0))   # needs start_pos
    with pytest.raises(ValueError):
        env.trajectory_returns(Rollout(K, pos_log=log.pos_log, start_pos=log.start_pos))   # needs flags_log
    with pytest.raises(ValueError):
        env.trajectory_labels(Rollout(K, pos_log=log.pos_log), env.build_table())          # needs start_pos
    env.close()


SHAPES = (("4x4 / 2 single colour", 4, 2, 2, False, 16), ("5x5 / 3 multi colour", 5, 3, 3, True, 25), ("8x8 / 8 multi colour", 8, 8, 8, True, 64),
          ("8x8 / 8 single colour", 8, 8, 8, False, 64), ("3x3, more targets than tiles", 3, 2, 3, True, 9), ("3x3, fewer targets than tiles", 3, 3, 1, False, 9),
          ("3x3 multi colour, fewer targets", 3, 3, 2, True, 9), ("no tiles", 4, 0, 2, False, 16), ("no targets", 4, 2, 0, False, 16), ("1x1", 1, 1, 1, True, 1),
          ("cell ids beyond the board", 5, 3, 3, False, 256), ("7x7 / 5 single colour, eight targets", 7, 5, 8, False, 49))


@pytest.mark.parametrize("what,S,T,Tt,mc,ids", SHAPES, ids=[s[0] for s in SHAPES])
def test_returns_on_every_kind_of_shape(torch_cuda, oracle, what, S, T, Tt, mc, ids):
    """Random cells (tiles share cells; `ids` bounds the cell ids - 256 reaches beyond the board and is clamped), targets that repeat,
    random flag bytes (every combination of bits), integer weights and values, gamma = 1, K = 5 and 257 boards: bit for bit."""
    torch = torch_cuda
    n, K = 257, 5
    rng = np.random.default_rng(S * 100 + T * 10 + Tt)
    first, pos_log = rng.integers(0, ids, (T, n)).astype(np.uint8), rng.integers(0, ids, (K, T, n)).astype(np.uint8)
    tgt = rng.integers(0, min(ids, S * S), (Tt, n)).astype(np.uint8)
    if Tt > 1:
        tgt[1, ::3] = tgt[0, ::3]
    flags = rng.integers(0, 256, (K, n)).astype(np.uint8)
    flags[:, ::2] &= 0x0f          # half of the boards play every step
    mb, ma = gr.m_logs(S, mc, first, pos_log, tgt)
    V, VL = gr.integer_values(K, n)
    want = gr.returns64(flags, mb, ma, V, VL, 1.0, 1.0, gr.INT_WEIGHTS, exact=True)
    assert T == 0 or Tt == 0 or S == 1 or (ma < 0).any()
    blk = np.zeros((oracle.blk_words(S), n), np.uint32)
    env = _env(S, mc, blk, np.zeros((T, n), np.uint8), tgt)
    dev = env.device
    got = env.trajectory_returns(_log(torch, env, first, pos_log, flags), 1.0, 1.0, torch.from_numpy(V).to(dev), torch.from_numpy(VL).to(dev),
                                 _weights(gr.INT_WEIGHTS))
    _assert_exact({k: t.cpu().numpy() for k, t in zip(("reward", "adv", "ret", "mask"), got)}, want, what)
    env.close()


# ---------------------------------------------------------------------------------------------- 5. labels
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", ("auto", "mc5", "s8"))
def test_labels_equal_the_yardstick_byte_for_byte(torch_cuda, oracle, name, K):
    """4x4 / 2, 5x5 / 3 multi colour and 8x8 / 2 (a two-word obstacle board): the table's answer on c[k], step by step; with rows=,
    some of them outside the table (-1, 0, 255 and never read)."""
    torch = torch_cuda
    from tiler_slider_amd import DistanceTable
    c = gr.trajectory(oracle, name)
    K = min(K, c["K"])
    S, n = c["S"], c["n"]
    env = _case_env(c)
    dist = torch.from_numpy(c["table"]).to(env.device)
    table = DistanceTable(dist, S, c["T"], c["T"], c["mc"], tref.MAX_DEPTH)
    log = _log(torch, env, c["first"], c["log"]["pos_log"][:K])
    want = gr.labels(oracle, S, c["blk"], c["first"], c["log"]["pos_log"][:K], c["table"])
    got = env.trajectory_labels(log, table)
    assert [t.dtype for t in got] == [torch.int16, torch.uint8, torch.uint8]
    for g, w_, what in zip(got, want, ("moves", "best", "action")):
        np.testing.assert_array_equal(g.cpu().numpy(), w_, err_msg=f"{name}: {what}")
    assert K < 5 or ((want[2] != 255).any() and (want[2] == 255).any() and (want[0] > 1).any())
    # rows: a permutation of a smaller table's rows, every seventh board outside it (negative, or past its end)
    half = n // 2
    rows = (np.arange(n) * 5 % half).astype(np.int32)
    rows[::7] = np.where(np.arange(0, n, 7) % 2 == 0, -1 - np.arange(0, n, 7), half + np.arange(0, n, 7))
    small = DistanceTable(dist[:half].contiguous(), S, c["T"], c["T"], c["mc"], tref.MAX_DEPTH)
    want = gr.labels(oracle, S, c["blk"], c["first"], c["log"]["pos_log"][:K], c["table"][:half], rows)
    lenient = _env(S, c["mc"], c["blk"], c["init"], c["tgt"], c["max_steps"], c["mode"], strict=False)
    got = lenient.trajectory_labels(log, small, torch.from_numpy(rows))
    for g, w_, what in zip(got, want, ("moves", "best", "action")):
        np.testing.assert_array_equal(g.cpu().numpy(), w_, err_msg=f"{name} rows: {what}")
    assert (want[0][:, ::7] == -1).all() and (want[2][:, ::7] == 255).all()
    env.close()
    lenient.close()


@pytest.mark.parametrize("mode", (STRICT, AUTORESET))
def test_labels_are_the_lookups_of_a_twin_stepped_through_the_logged_actions(torch_cuda, oracle, mode):
    """The GPU's own table-policy rollout with start, cells and actions logged; a twin environment on the same levels plays the
    logged actions one step() at a time and answers lookup_bits / expert_actions_from before each: row k of the labels.  After the
    last step the twin stands where the rollout left the environment."""
    torch = torch_cuda
    c = gr.trajectory(oracle, "strict" if mode == STRICT else "auto")
    K = 12
    env, twin = _case_env(c), _env(c["S"], c["mc"], c["blk"], c["init"], c["tgt"], c["max_steps"], c["mode"], strict=False)
    table = env.build_table()
    out = env.rollout(K, "table", table=table, epsilon=c["eps"], seed=c["seed"], log=("start", "pos", "act"))
    moves, best, action = env.trajectory_labels(out, table)
    for k in range(K):
        m, b = twin.lookup_bits(table)
        assert torch.equal(moves[k], m) and torch.equal(best[k], b) and torch.equal(action[k], twin.expert_actions_from(table)), k
        twin.step(out.act_log[k])
    assert torch.equal(twin.positions, env.positions) and torch.equal(twin.done, env.done)
    assert bool((action != 255).any())
    env.close()
    twin.close()


def test_rollout_logs_its_start(torch_cuda, oracle):
    """rollout(log="start"): the cells before the call, whether or not the environment advances; nothing else changes."""
    torch = torch_cuda
    c = gr.trajectory(oracle, "auto")
    env = _case_env(c)
    env.rollout(3, "random", seed=9)                     # somewhere inside the episodes
    for advance in (False, True):
        before = env.positions.clone()
        plain = env.rollout(4, "random", seed=10, log=("pos",), advance=False)
        out = env.rollout(4, "random", seed=10, log=("start", "pos"), advance=advance)
        assert out.start_pos is not None and out.start_pos.data_ptr() != env.positions.data_ptr()
        assert torch.equal(out.start_pos, before) and torch.equal(out.pos_log, plain.pos_log) and torch.equal(out.wins, plain.wins)
        assert plain.start_pos is None
        assert torch.equal(env.positions, out.pos_log[3] if advance else before)
    assert env.rollout(2, "random", log="start", stats=False).start_pos is not None
    with pytest.raises(ValueError):
        env.rollout(2, "random", log=("logits",))
    env.close()


# ---------------------------------------------------------------------------------------------- 6. the raw C-ABI into guarded memory
@pytest.mark.parametrize("name", ("auto", "mc5", "s8"))
def test_raw_calls_into_guarded_memory(torch_cuda, oracle, name):
    """Every buffer of a call between 256 guard bytes, the outputs prefilled with the complement of the expected bytes; outputs
    not asked for keep their fill; labels: pos_log holds K - 1 rows only (its last row is never read), steps = 1 with pos_log =
    NULL; returns: with the distance weights at 0 neither cells nor level are given (NULL), and with w_progress = 0 no `first`."""
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _targets_cabi as gc
    c = gr.trajectory(oracle, name)
    S, n, T, K = c["S"], c["n"], c["T"], min(5, c["K"])
    env = _case_env(c)
    dev = env.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = gc.lib()
    V, VL = gr.integer_values(c["K"], n)
    V4 = np.zeros((K, n, 4), np.float32)
    V4[..., 0] = V[:K]
    V4[..., 1:] = 1e30
    comp = lambda a: np.ascontiguousarray(~np.ascontiguousarray(a).view(np.uint8)).view(a.dtype).reshape(a.shape)

    def run_returns(steps, w, asked, with_cells, stride):
        f, pos = c["log"]["flags_log"][:steps], c["log"]["pos_log"][:steps]
        want = gr.returns64(f, c["m_before"][:steps], c["m_after"][:steps], V[:steps], VL, 1.0, 1.0, w, exact=True)
        outs = {"reward": want["reward"].astype(np.float32), "adv": want["adv"].astype(np.float32), "ret": want["ret"].astype(np.float32),
                "mask": want["mask"].astype(np.uint8)}
        bufs = {"flags": f, "values": V4[:steps] if stride == 4 else V[:steps], "last": VL, "tgt": c["tgt"], "first": c["first"], "pos_log": pos}
        g = {k: _guarded(torch, dev, v) for k, v in bufs.items()}
        g.update({k: _guarded(torch, dev, comp(v)) for k, v in outs.items()})
        at = lambda k: g[k].data_ptr() + GUARD
        st = _cabi.State(None, None, at("tgt"), None, None, None, None) if with_cells else None
        tin = gc.ReturnsIn(at("first") if w.progress else None, at("pos_log") if with_cells else None, at("flags"), at("values"), at("last"),
                           steps, stride, 1.0, 1.0, *w)
        tout = gc.ReturnsOut(*(at(k) if k in asked else None for k in ("reward", "adv", "ret", "mask")))
        assert L.ts_traj_returns(C.byref(env._dims), C.byref(st) if st else None, C.byref(tin), C.byref(tout), stream) == 0
        for k, v in outs.items():
            np.testing.assert_array_equal(_bits(_payload(g[k], v.dtype, v.shape)), _bits(v if k in asked else comp(v)), err_msg=f"{name} {steps}: {k}")
        for k, v in bufs.items():      # the inputs: guards intact, bytes as they were
            np.testing.assert_array_equal(_payload(g[k], np.uint8, (np.ascontiguousarray(v).nbytes,)), np.ascontiguousarray(v).reshape(-1).view(np.uint8))

    flat = gr.Weights(step=-1, win=5, timeout=-3, invalid=-2, dist=0, progress=0)
    for steps in (K, 2, 1):
        run_returns(steps, gr.INT_WEIGHTS, ("reward", "adv", "ret", "mask"), True, 4)
        run_returns(steps, gr.INT_WEIGHTS._replace(progress=0), ("adv",), True, 1)
        run_returns(steps, flat, ("ret", "mask"), False, 1)

    def run_labels(steps, asked, rows):
        pos = c["log"]["pos_log"][:steps - 1]
        want = gr.labels(oracle, S, c["blk"], c["first"], c["log"]["pos_log"][:steps], c["table"], rows)
        outs = dict(zip(("moves", "best", "action"), want))
        bufs = {"blk": c["blk"], "first": c["first"], "pos_log": pos, "table": c["table"]}
        if rows is not None:
            bufs["rows"] = rows
        g = {k: _guarded(torch, dev, v) for k, v in bufs.items()}
        g.update({k: _guarded(torch, dev, comp(v)) for k, v in outs.items()})
        at = lambda k: g[k].data_ptr() + GUARD
        st = _cabi.State(None, None, None, at("blk"), None, None, None)
        tin = gc.LabelsIn(at("first"), at("pos_log") if steps > 1 else None, at("table"), at("rows") if rows is not None else None, n, steps, 0)
        tout = gc.LabelsOut(*(at(k) if k in asked else None for k in ("moves", "best", "action")))
        assert L.ts_traj_labels(C.byref(env._dims), C.byref(st), C.byref(tin), C.byref(tout), stream) == 0
        for k, v in outs.items():
            np.testing.assert_array_equal(_payload(g[k], v.dtype, v.shape), v if k in asked else comp(v), err_msg=f"{name} {steps}: {k}")
        for k, v in bufs.items():
            np.testing.assert_array_equal(_payload(g[k], np.uint8, (np.ascontiguousarray(v).nbytes,)), np.ascontiguousarray(v).reshape(-1).view(np.uint8))

    rows = (np.arange(n)[::-1] - 3).astype(np.int32)      # the last three boards' rows are negative
    for steps in (K, 2, 1):
        run_labels(steps, ("moves", "best", "action"), None)
        run_labels(steps, ("action",), rows)
        run_labels(steps, ("moves",), None)
    env.close()


# ---------------------------------------------------------------------------------------------- 7. every compiled kernel at occupancy
OCC_WAVES, OCC_STEPS = 4096, 2


@pytest.mark.parametrize("name", sorted(gr.OCCUPANCY_CASES))
def test_every_compiled_targets_kernel_at_occupancy(torch_cuda, oracle, name):
    """Every kernel of the targets library on 262,144 boards (4,096 waves), two steps, on 128 distinct (level, cells, flags, values)
    in turn, exactly: the answer of the batch is the answer of the 128, tiled."""
    torch = torch_cuda
    from tiler_slider_amd import DistanceTable, _targets_cabi as gc
    S, T, Ko = gr.OCCUPANCY_CASES[name]
    distinct, n, K = 128, OCC_WAVES * 64, OCC_STEPS
    mc = S % 2 == 0
    Cc = S * S
    rng = np.random.default_rng(S)
    blk, init, tgt = gr.occupancy_levels(oracle, S, T, Ko, distinct, 0x0CC + S)
    level = (np.arange(n) % distinct).astype(np.int64)
    tile = lambda a: np.ascontiguousarray(a[..., level])
    env = _env(S, mc, tile(blk), tile(init), tile(tgt))
    dev = env.device
    if "returns" in name:
        first, pos_log = rng.integers(0, Cc, (T, distinct)).astype(np.uint8), rng.integers(0, Cc, (K, T, distinct)).astype(np.uint8)
        flags = rng.integers(0, 128, (K, distinct)).astype(np.uint8)
        flags[:, ::2] &= 0x0f
        V, VL = gr.integer_values(K, distinct)
        mb, ma = gr.m_logs(S, mc, first, pos_log, tgt)
        want = gr.returns64(flags, mb, ma, V, VL, 1.0, 1.0, gr.INT_WEIGHTS, exact=True)
        d = gc.describe_traj_returns(env._dims, K)
        assert d["name"] == name and d["samples"] == K * n and d["blocks"] * (d["threads_per_block"] // 64) >= OCC_WAVES
        got = env.trajectory_returns(_log(torch, env, tile(first), tile(pos_log), tile(flags)), 1.0, 1.0, torch.from_numpy(tile(V)).to(dev),
                                     torch.from_numpy(tile(VL)).to(dev), _weights(gr.INT_WEIGHTS))
        _assert_exact({k: t.cpu().numpy() for k, t in zip(("reward", "adv", "ret", "mask"), got)},
                      {k: v[:, level] for k, v in want.items()}, name)
    else:
        table = tref.table(oracle, S, mc, blk, tgt, T)
        # cells the oracle can be asked about: the levels' own start, and one random step on
        b = oracle.OracleBatch(S, mc, 100, blk, init, tgt)
        b.reset()
        first = b.pos.copy()
        b.step(rng.integers(0, 4, distinct).astype(np.uint8), obs=False)
        pos_log = np.stack([b.pos.copy(), b.pos.copy()])
        want = gr.labels(oracle, S, blk, first, pos_log, table)
        d = gc.describe_traj_labels(env._dims, K)
        assert d["name"] == name and d["samples"] == K * n and d["blocks"] * (d["threads_per_block"] // 64) >= OCC_WAVES
        small = DistanceTable(torch.from_numpy(table).to(dev), S, T, T, mc, tref.MAX_DEPTH)
        got = env.trajectory_labels(_log(torch, env, tile(first), tile(pos_log)), small, torch.from_numpy(level.astype(np.int32)))
        for g, w_, what in zip(got, want, ("moves", "best", "action")):
            np.testing.assert_array_equal(g.cpu().numpy(), w_[:, level], err_msg=f"{name}: {what}")
    env.close()


# ---------------------------------------------------------------------------------------------- 8. streams
def test_both_calls_on_a_stream_of_their_own_behind_a_policy_rollout(torch_cuda, oracle):
    """2**16 boards, one extra stream, no host synchronisation until the end: a rollout_policy of 24 steps and, enqueued behind it
    on the same side stream while it still runs, both target calls on its logs.  A launch that ignored its `stream` argument
    would run on the idle default stream at once and read logs the rollout has not written yet (they are zero-filled: every
    step would be a played step with no win).  Checked against the same calls made after a synchronisation."""
    torch = torch_cuda
    from tiler_slider_amd import PolicyNet
    S, T, n, K = 4, 2, 1 << 16, 24
    blk, init, tgt = oracle.generate(S, T, T, 2, n, seed=21)
    env = _env(S, False, blk, init, tgt, 6)
    table = env.build_table()
    net = PolicyNet(3 * S * S, 32, env.device, generator=torch.Generator(device=env.device).manual_seed(3))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=env.device)
    assert side.cuda_stream != torch.cuda.current_stream(env.device).cuda_stream
    with torch.cuda.stream(side):
        out = env.rollout_policy(K, net.policy(), select="sample", seed=2, log=("start", "pos", "flags"))
        ret = env.trajectory_returns(out, 0.5, 1.0)
        lab = env.trajectory_labels(out, table)
    torch.cuda.synchronize()
    again, lab2 = env.trajectory_returns(out, 0.5, 1.0), env.trajectory_labels(out, table)
    for a, b in zip(tuple(ret) + tuple(lab), tuple(again) + tuple(lab2)):
        assert torch.equal(a, b)
    assert not bool(ret.mask.all()) and bool((ret.reward != 0).any()) and bool((lab[2] != 255).any())
    env.close()


# ---------------------------------------------------------------------------------------------- 9. one learning check
def test_thirty_dagger_iterations_lower_the_loss(torch_cuda):
    """DAgger on 256 solvable 4x4 levels, H = 32, Adam at 1e-2, 30 iterations: the learner's own rollout_policy of 32 steps ->
    trajectory_labels -> cross-entropy on the steps where the expert has a move, through trajectory_logits.  Asserted: the last
    loss is below the first; the curve is printed."""
    torch = torch_cuda
    from tiler_slider_amd import PolicyNet, TilerSliderEnvFactory
    dev = torch.device("cuda", 0)
    seeds = TilerSliderEnvFactory.solvable_seeds(256, size=4, num_tiles=2, num_obstacles=2, device=dev)
    env = TilerSliderEnvFactory.create_vec_env_from_seeds(seeds, size=4, num_tiles=2, num_obstacles=2, device=dev, max_steps=16, auto_reset=True,
                                                          obs_dtype=None)
    env.reset()
    table = env.build_table()
    net = PolicyNet(env.onehot_channels * 16, 32, dev, generator=torch.Generator(device=dev).manual_seed(0))
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    losses = []
    for it in range(30):
        out = env.rollout_policy(32, net.policy(), select="sample", seed=it, log=("start", "pos"))
        _, _, action = env.trajectory_labels(out, table)
        has = action != 255
        logp = torch.log_softmax(env.trajectory_logits(net, out), dim=2)
        loss = -(logp.gather(2, action.clamp(max=3).long().unsqueeze(2)).squeeze(2) * has).sum() / has.sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("DAgger losses:", [round(x, 3) for x in losses])
    assert losses[-1] < losses[0]
    env.close()
