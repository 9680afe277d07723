"""The V-trace targets on the GPU (lib/libtiler_slider_vtrace.so, VecTilerSliderEnv.trajectory_vtrace) against the CPU yardstick
tests/vtrace_reference.py - the definition of include/tiler_slider_vtrace.h in float64 with its a-priori bound -, against
trajectory_returns() through the header's identities, and on the logs of real mixed rollouts.  Every comparison with the
yardstick first asserts the floors on its inputs."""
import ctypes as C

import numpy as np
import pytest

import targets_reference as gr
import vtrace_reference as vr
from table_harness import GUARD, guarded as _guarded, payload as _payload

pytestmark = pytest.mark.gpu

STRICT, AUTORESET = 0, 1
GREEDY, SAMPLE = 0, 1
SELECT = {GREEDY: "greedy", SAMPLE: "sample"}
INF = float("inf")
KEYS = ("reward", "adv", "ret", "mask", "weight", "log_mu")


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


def _case_env(c, boards=None):
    cut = (lambda a: np.ascontiguousarray(a[..., :boards])) if boards else (lambda a: a)
    return _env(c["S"], c["mc"], cut(c["blk"]), cut(c["init"]), cut(c["tgt"]), c["max_steps"], c["mode"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _chunk(env):
    from tiler_slider_amd import _vtrace_cabi as vc
    return vc.describe_traj_vtrace(env._dims, 1)["chunk_steps"]


def _rollout(torch, env, c, i, K, expert=True):
    """A Rollout that holds the first K steps of case c's log and of the inputs i, on the environment's device."""
    from tiler_slider_amd import Rollout
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.device)
    return Rollout(K, start_pos=put(c["first"]), pos_log=put(c["log"]["pos_log"][:K]), flags_log=put(i["flags_log"][:K]), act_log=put(i["act_log"][:K]),
                   logits_log=put(i["mu_logits"][:K]), expert_log=put(i["expert_log"][:K]) if expert else None)


def _call(torch, env, roll, i, K, eps=0.0, beta=0.0, select=SAMPLE, pi=True, values=True, last=True, w=vr.FLAT, **kw):
    from tiler_slider_amd import RewardWeights
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.device)
    got = env.trajectory_vtrace(roll, put(i["pi_logits"][:K]) if pi else None, put(i["values"][:K]) if values else None,
                                put(i["last_value"]) if last else None, kw.pop("gamma", vr.GAMMA), kw.pop("lam", vr.LAM), kw.pop("rho_bar", 1.0),
                                kw.pop("c_bar", 1.0), SELECT[select], eps, beta, RewardWeights(*w))
    assert not kw and got.mask.dtype == torch.bool and all(t.dtype == torch.float32 and tuple(t.shape) == tuple(got.mask.shape) for t in (got[:3] + got[4:]))
    return {k: t.cpu().numpy() for k, t in zip(KEYS, got)}


def _want(i, K, eps=0.0, beta=0.0, select=SAMPLE, pi=True, w=vr.FLAT, **kw):
    return vr.vtrace64(i["flags_log"][:K], i["act_log"][:K], i["m_before"][:K], i["m_after"][:K], i["mu_logits"][:K], i["pi_logits"][:K] if pi else None,
                       i["expert_log"][:K], i["values"][:K], i["last_value"], w=w, select=select, explore_threshold=vr.threshold_of(eps),
                       beta_threshold=vr.threshold_of(beta), **kw)


def _within(got, want, what):
    share = vr.worst(got, want)
    print(f"{what}: worst share of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in share.items() if k != "mask"))
    assert max(share.values()) <= 1.0, (what, share)
    return share


# ---------------------------------------------------------------------------------------------- 1. on-policy: exact
@pytest.mark.parametrize("name", ("auto", "strict", "given"))
def test_on_policy_integer_targets_are_trajectory_returns_bit_for_bit(torch_cuda, oracle, name):
    """Integer values and reward weights, gamma = lambda = 1/2, episodes of at most 6 steps: targets_reference asserts that every
    intermediate of the recursion is a float32, so no order of evaluation can show.  pi_logits NULL, both thresholds 0, SAMPLE, on
    Gaussian logits: weight == 1 exactly on every live sample, ret is trajectory_returns()' ret bit for bit and - both at
    lambda = 1 - adv its adv.  With the bars at 1, above 1 and infinite."""
    torch = torch_cuda
    from tiler_slider_amd import RewardWeights
    c = gr.trajectory(oracle, name)
    env = _case_env(c)
    i = dict(vr.inputs(c))
    i["values"], i["last_value"] = gr.integer_values(c["K"], c["n"])
    dev = env.device
    for K in (1, _chunk(env) + 1, 24):
        roll = _rollout(torch, env, c, i, K, expert=False)
        for lam in (0.5, 1.0):
            gr.returns64(i["flags_log"][:K], i["m_before"][:K], i["m_after"][:K], i["values"][:K], i["last_value"], 0.5, lam, gr.INT_WEIGHTS, exact=True)
            tr = env.trajectory_returns(roll, 0.5, lam, torch.from_numpy(i["values"][:K]).to(dev), torch.from_numpy(i["last_value"]).to(dev),
                                        RewardWeights(*gr.INT_WEIGHTS))
            for bar in (1.0, 3.0, INF):
                got = _call(torch, env, roll, i, K, pi=False, w=gr.INT_WEIGHTS, gamma=0.5, lam=lam, rho_bar=bar, c_bar=bar)
                live = got["mask"]
                np.testing.assert_array_equal(live, tr.mask.cpu().numpy())
                np.testing.assert_array_equal(got["weight"], live.astype(np.float32), err_msg=f"{name} K={K}: weight")
                np.testing.assert_array_equal(_bits(got["ret"]), _bits(tr.ret.cpu().numpy()), err_msg=f"{name} K={K} lam={lam}: ret")
                np.testing.assert_array_equal(_bits(got["reward"]), _bits(tr.reward.cpu().numpy()), err_msg=f"{name} K={K}: reward")
                if lam == 1.0:
                    np.testing.assert_array_equal(_bits(got["adv"]), _bits(tr.adv.cpu().numpy()), err_msg=f"{name} K={K}: adv")
                assert np.isfinite(got["log_mu"]).all() and (got["log_mu"][live] < 0).all() and (got["log_mu"][~live] == 0).all()
        assert K < 5 or (0 < live.mean() < 1 and np.abs(got["adv"]).max() > 0)
    env.close()


# ---------------------------------------------------------------------------------------------- 2. the sixteen combinations: the bound
@pytest.mark.parametrize("select", vr.SELECTS, ids=("greedy", "sample"))
@pytest.mark.parametrize("eps,beta", vr.PARAMS)
@pytest.mark.parametrize("name", vr.CASES)
def test_gaussian_targets_lie_within_the_bound(torch_cuda, oracle, name, eps, beta, select):
    """rho_bar = c_bar = 1, gamma = 0.97, lambda = 0.9, Gaussian logits, values and last_value: every output of every sample within
    the yardstick's bound, void steps and infinite weights exactly, for K = 1, around the chunk, 24 and - "long" - 200."""
    torch = torch_cuda
    c = gr.trajectory(oracle, name)
    env = _case_env(c)
    i = vr.inputs(c)
    full = _want(i, c["K"], eps, beta, select)
    print(name, eps, beta, select, vr.check_floors(vr.shares(full, i["flags_log"], i["act_log"], i["expert_log"]), select, vr.threshold_of(eps)))
    chunk = _chunk(env)
    for K in sorted({1, chunk - 1, chunk, chunk + 1, 24, c["K"]}):
        got = _call(torch, env, _rollout(torch, env, c, i, K), i, K, eps, beta, select)
        _within(got, full if K == c["K"] else _want(i, K, eps, beta, select), f"{name} eps={eps} beta={beta} {SELECT[select]} K={K}")
    env.close()


# ---------------------------------------------------------------------------------------------- 3. the reward reads the cells
@pytest.mark.parametrize("select", vr.SELECTS, ids=("greedy", "sample"))
@pytest.mark.parametrize("name", vr.CELL_CASES)
def test_all_six_reward_weights_on_the_cell_cases(torch_cuda, oracle, name, select):
    torch = torch_cuda
    from tiler_slider_amd import _vtrace_cabi as vc
    c = gr.trajectory(oracle, name)
    env = _case_env(c)
    i = vr.inputs(c)
    assert all(x != 0 for x in vr.WEIGHTS) and (i["m_after"] != i["m_before"]).any()
    assert vc.describe_traj_vtrace(env._dims, c["K"], vc.OUT_ALL | vc.IN_CELLS)["name"] == f"k_traj_vtrace<{c['S']}>"
    roll = _rollout(torch, env, c, i, c["K"])
    for w in (vr.WEIGHTS, vr.WEIGHTS._replace(progress=0.0), vr.WEIGHTS._replace(dist=0.0)):
        _within(_call(torch, env, roll, i, c["K"], 0.125, 0.5, select, w=w), _want(i, c["K"], 0.125, 0.5, select, w=w), f"{name} {SELECT[select]} {w}")
    env.close()


# ---------------------------------------------------------------------------------------------- 4. the bars
def test_infinite_bars_and_a_zero_bar(torch_cuda, oracle):
    """rho_bar = c_bar = +infinity: no clipping, within the bound, on the three parameter sets whose mu is positive everywhere
    (under GREEDY with eps = 0 an infinite weight meets an infinite bar and nothing finite is left: the header's mu == 0 rule).
    rho_bar = 0: ret == V and adv == 0 exactly, on all four."""
    torch = torch_cuda
    c = gr.trajectory(oracle, "auto")
    env = _case_env(c)
    i = vr.inputs(c)
    K = c["K"]
    roll = _rollout(torch, env, c, i, K)
    for eps, beta in vr.PARAMS:
        for select in vr.SELECTS:
            if not (select == GREEDY and eps == 0):
                want = _want(i, K, eps, beta, select, rho_bar=INF, c_bar=INF)
                assert (want["weight"][want["live"]] > 4).mean() > 0.01                 # weights a bar of 1 would have cut, by far
                _within(_call(torch, env, roll, i, K, eps, beta, select, rho_bar=INF, c_bar=INF), want, f"infinite bars eps={eps} {SELECT[select]}")
            got = _call(torch, env, roll, i, K, eps, beta, select, rho_bar=0.0)
            live = got["mask"]
            np.testing.assert_array_equal(got["ret"], np.where(live, i["values"][:K], np.float32(0)))
            assert (got["adv"] == 0).all() and (got["reward"][live] != 0).any() and (got["weight"][live] != 1).any()
    env.close()


# ---------------------------------------------------------------------------------------------- 5. pairs that agree bit for bit
def test_null_pointers_and_what_stands_for_them_agree_bit_for_bit(torch_cuda, oracle):
    """pi_logits NULL and the logged tensor passed again; expert_log NULL, all 255, and any bytes at beta = 0."""
    torch = torch_cuda
    from tiler_slider_amd import Rollout
    c = gr.trajectory(oracle, "auto")
    env = _case_env(c)
    i = vr.inputs(c)
    K = c["K"]
    roll, bare = _rollout(torch, env, c, i, K), _rollout(torch, env, c, i, K, expert=False)
    same = lambda a, b, what: [np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{what}: {k}") for k in KEYS]
    again = dict(i, pi_logits=i["mu_logits"])
    for select in vr.SELECTS:
        a = _call(torch, env, roll, i, K, 0.125, 0.5, select, pi=False)
        same(a, _call(torch, env, roll, again, K, 0.125, 0.5, select, pi=True), "pi_logits NULL / the logged logits")
        assert (a["weight"][a["mask"]] != 1).any()
        none = Rollout(K, flags_log=roll.flags_log, act_log=roll.act_log, logits_log=roll.logits_log, expert_log=torch.full_like(roll.expert_log, 255))
        at0 = _call(torch, env, bare, i, K, 0.125, 0.0, select)
        same(at0, _call(torch, env, none, i, K, 0.125, 0.0, select), "expert_log NULL / all 255, beta = 0")
        same(at0, _call(torch, env, roll, i, K, 0.125, 0.0, select), "expert_log NULL / any bytes, beta = 0")
        same(at0, _call(torch, env, none, i, K, 0.125, 0.5, select), "expert_log NULL, beta = 0 / all 255, beta = 1/2")
        assert any((_call(torch, env, roll, i, K, 0.125, 0.5, select)[k] != at0[k]).any() for k in ("weight", "ret"))
    with pytest.raises(ValueError, match="expert"):
        _call(torch, env, bare, i, K, 0.125, 0.5, SAMPLE)
    env.close()


# ---------------------------------------------------------------------------------------------- 6. mu == 0
def test_a_behaviour_probability_of_zero_gives_the_bars(torch_cuda, oracle):
    """GREEDY with eps = 0: an action that is neither the argmax nor the expert's has mu == 0.  There weight is +infinity and log_mu
    -infinity exactly, everywhere else both are finite, and rho and c are the bars: with rho_bar = 2.5 and c_bar = 1.5 every output
    is inside the bound, whose weights on those samples are the bars themselves."""
    torch = torch_cuda
    c = gr.trajectory(oracle, "auto")
    env = _case_env(c)
    i = vr.inputs(c)
    K = c["K"]
    want = _want(i, K, 0.0, 0.5, GREEDY, rho_bar=2.5, c_bar=1.5)
    live, zero = want["live"], want["live"] & (want["mu"] == 0)
    assert vr.check_floors(vr.shares(want, i["flags_log"], i["act_log"], i["expert_log"]), GREEDY, 0)["mu_zero"] >= 0.30
    got = _call(torch, env, _rollout(torch, env, c, i, K), i, K, 0.0, 0.5, GREEDY, rho_bar=2.5, c_bar=1.5)
    assert (got["weight"][zero] == INF).all() and (got["log_mu"][zero] == -INF).all()
    assert np.isfinite(got["weight"][~zero]).all() and np.isfinite(got["log_mu"][~zero]).all()
    assert np.isfinite(got["ret"]).all() and np.isfinite(got["adv"]).all()
    _within(got, want, "mu == 0, bars 2.5 and 1.5")
    env.close()


# ---------------------------------------------------------------------------------------------- 7. values in place, the refusals
def test_values_in_place_from_a_logits_tensor_and_the_api_refusals(torch_cuda, oracle):
    torch = torch_cuda
    from tiler_slider_amd import Rollout
    c = gr.trajectory(oracle, "auto")
    env = _case_env(c)
    i = vr.inputs(c)
    K, n, dev = c["K"], c["n"], env.device
    roll = _rollout(torch, env, c, i, K)
    V4 = torch.full((K, n, 4), 1e30, dtype=torch.float32, device=dev)
    V4[..., 0] = torch.from_numpy(i["values"]).to(dev)
    pi, VL = torch.from_numpy(i["pi_logits"]).to(dev), torch.from_numpy(i["last_value"]).to(dev)
    a = env.trajectory_vtrace(roll, pi, V4[..., 0], VL, vr.GAMMA, vr.LAM, epsilon=0.125, beta=0.5)
    b = env.trajectory_vtrace(roll, pi, V4[..., 0].contiguous(), VL, vr.GAMMA, vr.LAM, epsilon=0.125, beta=0.5)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert all(torch.equal(x, y) for x, y in zip(a.returns, (a.reward, a.adv, a.ret, a.mask)))
    pi.requires_grad_(True)
    assert not env.trajectory_vtrace(roll, pi, epsilon=0.125, beta=0.5).adv.requires_grad      # detached
    for gone, asked in (("flags_log", "flags"), ("act_log", "act"), ("logits_log", "logits")):
        kw = {k: getattr(roll, k) for k in ("flags_log", "act_log", "logits_log", "expert_log") if k != gone}
        with pytest.raises(ValueError, match=asked):
            env.trajectory_vtrace(Rollout(K, **kw))
    from tiler_slider_amd import RewardWeights
    no_cells = Rollout(K, flags_log=roll.flags_log, act_log=roll.act_log, logits_log=roll.logits_log)
    with pytest.raises(ValueError, match="pos"):
        env.trajectory_vtrace(no_cells, reward=RewardWeights(dist=1.0))
    with pytest.raises(ValueError, match="start"):
        env.trajectory_vtrace(Rollout(K, flags_log=roll.flags_log, act_log=roll.act_log, logits_log=roll.logits_log, pos_log=roll.pos_log),
                              reward=RewardWeights(progress=1.0))
    with pytest.raises(ValueError, match="expert"):
        env.trajectory_vtrace(no_cells, beta=0.5)
    with pytest.raises(ValueError, match="logits"):
        env.trajectory_vtrace(roll, pi.detach()[:, :, :3])
    with pytest.raises(ValueError, match="values"):
        env.trajectory_vtrace(roll, values=V4[..., 0][:, ::2])
    env.close()


# ---------------------------------------------------------------------------------------------- 8. raw calls into guarded memory
@pytest.mark.parametrize("name", ("auto", "mc5"))
def test_raw_calls_into_guarded_memory(torch_cuda, oracle, name):
    """165 boards (two full waves and 37 lanes of a third), every buffer of a call between 256 guard bytes, the outputs prefilled
    with the complement of the expected bytes: all six outputs together and each alone give the wrapper's bytes, outputs not
    asked for keep their fill, every input is as it was.  "mc5" reads the cells (k_traj_vtrace<5>), "auto" does not - neither
    cells nor level are then given (NULL)."""
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _vtrace_cabi as vc
    c = gr.trajectory(oracle, name)
    n, K = 165, min(c["K"], 6)
    cut = lambda a: np.ascontiguousarray(a[..., :n]) if a.ndim and a.shape[-1] == c["n"] else np.ascontiguousarray(np.asarray(a)[:, :n, :])
    cells = name == "mc5"
    w = vr.WEIGHTS if cells else vr.FLAT
    i = {k: cut(v[:K]) if k != "last_value" else cut(v) for k, v in vr.inputs(c).items()}
    small = dict(c, n=n, first=cut(c["first"]), log=dict(pos_log=cut(c["log"]["pos_log"][:K])))
    env = _case_env(c, n)
    dev = env.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    want = _want(i, K, 0.125, 0.5, SAMPLE, w=w)
    ref = _call(torch, env, _rollout(torch, env, small, i, K), i, K, 0.125, 0.5, SAMPLE, w=w)
    _within(ref, want, f"{name} x165")
    ref["mask"] = ref["mask"].astype(np.uint8)
    comp = lambda a: np.ascontiguousarray(~np.ascontiguousarray(a).view(np.uint8)).view(a.dtype).reshape(a.shape)
    bufs = {"flags": i["flags_log"], "act": i["act_log"], "expert": i["expert_log"], "mu": i["mu_logits"], "pi": i["pi_logits"], "values": i["values"],
            "last": i["last_value"], "tgt": cut(c["tgt"]), "first": small["first"], "pos_log": small["log"]["pos_log"]}
    for asked in (vc.OUT_FIELDS,) + tuple((f,) for f in vc.OUT_FIELDS):
        g = {k: _guarded(torch, dev, v) for k, v in bufs.items()}
        g.update({k: _guarded(torch, dev, comp(ref[k])) for k in vc.OUT_FIELDS})
        at = lambda k: g[k].data_ptr() + GUARD
        st = _cabi.State(None, None, at("tgt"), None, None, None, None) if cells else None
        tin = vc.VtraceIn(at("first") if cells else None, at("pos_log") if cells else None, at("flags"), at("values"), at("last"), K, 1, vr.GAMMA, vr.LAM,
                          *w, at("act"), at("expert"), at("mu"), at("pi"), SAMPLE, 0, vr.threshold_of(0.125), vr.threshold_of(0.5), 1.0, 1.0)
        tout = vc.VtraceOut(*(at(k) if k in asked else None for k in vc.OUT_FIELDS))
        assert vc.lib().ts_traj_vtrace(C.byref(env._dims), C.byref(st) if st else None, C.byref(tin), C.byref(tout), stream) == 0
        for k in vc.OUT_FIELDS:
            np.testing.assert_array_equal(_bits(_payload(g[k], ref[k].dtype, ref[k].shape)), _bits(ref[k] if k in asked else comp(ref[k])),
                                          err_msg=f"{name} {asked}: {k}")
        for k, v in bufs.items():      # the inputs: guards intact, bytes as they were
            np.testing.assert_array_equal(_payload(g[k], np.uint8, (np.ascontiguousarray(v).nbytes,)), np.ascontiguousarray(v).reshape(-1).view(np.uint8))
    env.close()


# ---------------------------------------------------------------------------------------------- 9. every compiled kernel at occupancy
OCC_WAVES, OCC_STEPS = 4096, 5


@pytest.mark.parametrize("name", sorted(vr.OCCUPANCY_CASES))
def test_every_compiled_vtrace_kernel_at_occupancy(torch_cuda, oracle, name):
    """Every kernel of the library on 262,144 boards (4,096 waves), five steps, on 128 distinct (level, cells, flags, actions,
    logits, values) in turn: the 128 lie within the yardstick's bound, and the answer of the batch is their answer, tiled, bit for
    bit."""
    torch = torch_cuda
    from tiler_slider_amd import Rollout, RewardWeights, _vtrace_cabi as vc
    S, T, Ko = vr.OCCUPANCY_CASES[name]
    cells = not name.endswith("<0>")
    distinct, n, K = 128, OCC_WAVES * 64, OCC_STEPS
    mc = S % 2 == 0
    rng = np.random.default_rng(40 + S + cells)
    blk, init, tgt = gr.occupancy_levels(oracle, S, T, Ko, distinct, 0x0CC + S)
    level = np.arange(n) % distinct
    first, pos_log = rng.integers(0, S * S, (T, distinct)).astype(np.uint8), rng.integers(0, S * S, (K, T, distinct)).astype(np.uint8)
    flags = rng.integers(0, 128, (K, distinct)).astype(np.uint8)
    flags[:, ::2] &= 0x0f
    mb, ma = gr.m_logs(S, mc, first, pos_log, tgt)
    act = rng.integers(0, 4, (K, distinct)).astype(np.uint8)
    u = rng.random((K, distinct))
    V, VL = gr.gaussian_values(K, distinct)
    i = dict(flags_log=flags, act_log=act, m_before=mb, m_after=ma, mu_logits=(2 * rng.standard_normal((K, distinct, 4))).astype(np.float32),
             expert_log=np.where(u < 0.4, 255, np.where(u < 0.7, act, rng.integers(0, 4, (K, distinct)))).astype(np.uint8), values=V, last_value=VL)
    i["pi_logits"] = (i["mu_logits"] + rng.standard_normal((K, distinct, 4))).astype(np.float32)
    w = vr.WEIGHTS if cells else vr.FLAT
    want = _want(i, K, 0.125, 0.5, SAMPLE, w=w)
    assert 0.2 < want["live"].mean() < 0.8

    def run(idx):
        tile = lambda a: np.ascontiguousarray(a[..., idx]) if a.shape[-1] == distinct else np.ascontiguousarray(a[:, idx, :])
        env = _env(S, mc, tile(blk), tile(init), tile(tgt))
        put = lambda a: torch.from_numpy(tile(a)).to(env.device)
        d = vc.describe_traj_vtrace(env._dims, K, vc.OUT_ALL | (vc.IN_CELLS if cells else 0))
        assert d["name"] == name and d["samples"] == K * len(idx)
        roll = Rollout(K, start_pos=put(first), pos_log=put(pos_log), flags_log=put(flags), act_log=put(act), logits_log=put(i["mu_logits"]),
                       expert_log=put(i["expert_log"]))
        got = env.trajectory_vtrace(roll, put(i["pi_logits"]), put(V), put(VL), vr.GAMMA, vr.LAM, 1.0, 1.0, "sample", 0.125, 0.5, RewardWeights(*w))
        got = {k: t.cpu().numpy() for k, t in zip(KEYS, got)}
        env.close()
        return got, d

    small, _ = run(np.arange(distinct))
    _within(small, want, name)
    big, d = run(level)
    assert d["blocks"] * (d["threads_per_block"] // 64) >= OCC_WAVES
    for k in KEYS:
        np.testing.assert_array_equal(_bits(big[k]), _bits(small[k][:, level]), err_msg=f"{name}: {k}")


# ---------------------------------------------------------------------------------------------- 10. streams; real mixed rollouts
def _mixed(torch, oracle, n, seed, hidden=32):
    from tiler_slider_amd import PolicyNet
    S, T = 4, 2
    blk, init, tgt = oracle.generate(S, T, T, 2, n, seed=seed)
    env = _env(S, False, blk, init, tgt, 6)
    table = env.build_table()
    net = PolicyNet(3 * S * S, hidden, env.device, generator=torch.Generator(device=env.device).manual_seed(3))
    return env, table, net, tgt


def test_a_call_on_a_stream_of_its_own_behind_a_mixed_rollout(torch_cuda, oracle):
    """2**16 boards, one extra stream, no host synchronisation until the end: a mixed rollout of 24 steps and, enqueued behind it on
    the same side stream while it still runs, the V-trace call on its logs.  A launch that ignored its `stream` argument would run
    on the idle default stream at once and read logs the rollout has not written yet.  Checked against the same call made after a
    synchronisation."""
    torch = torch_cuda
    env, table, net, _ = _mixed(torch, oracle, 1 << 16, 21)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=env.device)
    assert side.cuda_stream != torch.cuda.current_stream(env.device).cuda_stream
    kw = dict(gamma=0.5, epsilon=0.125, beta=0.5)
    with torch.cuda.stream(side):
        out = env.rollout_policy(24, net.policy(), select="sample", epsilon=0.125, seed=2, log=("flags", "act", "logits", "expert"), expert=table, beta=0.5)
        vt = env.trajectory_vtrace(out, **kw)
    torch.cuda.synchronize()
    again = env.trajectory_vtrace(out, **kw)
    for a, b in zip(vt, again):
        assert torch.equal(a, b)
    assert not bool(vt.mask.all()) and bool((vt.reward != 0).any()) and bool((vt.weight[vt.mask] != 1).any())
    env.close()


@pytest.mark.parametrize("select,epsilon", (("greedy", 0.125), ("sample", 0.125), ("sample", 0.0)))
def test_the_logs_of_a_real_mixed_rollout(torch_cuda, oracle, select, epsilon):
    """rollout_policy(expert=table, beta=0.5, epsilon=, log=(...)) on 517 4x4 boards of two tiles, K = 24: trajectory_vtrace on the
    device's own logs lies within the yardstick's bound, with the logged logits as the target policy and with drifted ones; mu > 0
    on every live sample - the rollout's parameters explain every action it played -; and where who_log says the expert played,
    the action is the expert's."""
    torch = torch_cuda
    n, K = 517, 24
    env, table, net, tgt = _mixed(torch, oracle, n, 23)
    out = env.rollout_policy(K, net.policy(), select=select, epsilon=epsilon, seed=5, log=("start", "pos", "flags", "act", "logits", "expert", "who"),
                             expert=table, beta=0.5)
    host = lambda t: t.cpu().numpy()
    act, expert, who = host(out.act_log), host(out.expert_log), host(out.who_log)
    assert (who == 1).mean() > 0.05 and (act[who == 1] == expert[who == 1]).all()
    mb, ma = gr.m_logs(4, False, host(out.start_pos), host(out.pos_log), tgt)
    rng = np.random.default_rng(9)
    V, VL = gr.gaussian_values(K, n)
    i = dict(flags_log=host(out.flags_log), act_log=act, m_before=mb, m_after=ma, mu_logits=host(out.logits_log), expert_log=expert, values=V, last_value=VL)
    i["pi_logits"] = (i["mu_logits"] + 0.5 * rng.standard_normal((K, n, 4))).astype(np.float32)
    sel = GREEDY if select == "greedy" else SAMPLE
    for pi in (False, True):
        want = _want(i, K, epsilon, 0.5, sel, pi=pi, w=vr.WEIGHTS)
        live = want["live"]
        assert 0.3 < live.mean() < 1 and (want["mu"][live] > 0).all()
        got = _call(torch, env, out, i, K, epsilon, 0.5, sel, pi=pi, w=vr.WEIGHTS)
        assert np.isfinite(got["weight"]).all() and np.isfinite(got["log_mu"]).all()
        _within(got, want, f"mixed rollout {select} eps={epsilon} pi={'drifted' if pi else 'logged'}")
    env.close()
