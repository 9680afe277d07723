"""The lookahead on the GPU (lib/libtiler_slider_lookahead.so, VecTilerSliderEnv.lookahead / td_targets) against the CPU yardstick
tests/lookahead_reference.py - the definition of include/tiler_slider_lookahead.h on NumPy over the oracle -, against the distance
tables, against twin environments stepped by hand and against the training library's logits on the successor boards.

THE INPUTS are lookahead_reference.near_win_levels: levels of generate_mt19937 whose targets are where the tiles stand after
1 + n % 4 seeded moves, so wins lie inside the horizon.  Every case asserts on the yardstick's own numbers, before it looks at the
GPU, that they do (lookahead_reference.conditions): a win inside the horizon on at least 25 % of the samples, every action the
best on at least 5 %, an invalid root move on at least 1 %, and up to 4x4 a board won on entry.  The degenerate shapes - 1x1 and
zero tiles, where every board is won or none can be - are exempt from what they cannot have and say so."""
import ctypes as C

import numpy as np
import pytest

import ac_reference as ar
import lookahead_reference as lr
import policy_reference as pref
from table_harness import guarded as _guarded, payload as _payload

pytestmark = pytest.mark.gpu

ZERO, VALUE, QMAX = lr.LEAF_ZERO, lr.LEAF_VALUE, lr.LEAF_QMAX
LEAF_NAMES = {ZERO: "zero", VALUE: "value", QMAX: "qmax"}
W_EXACT = (-1.0, 8.0, -2.0)   # w_step, w_win, w_invalid
BIG = 1 << 20


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _env(S, mc, blk, init, tgt, **kw):
    from tiler_slider_amd import VecTilerSliderEnv
    kw.setdefault("obs_dtype", None)
    env = VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=mc, max_steps=BIG, **kw)
    env.reset()
    return env


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _nets(torch, env, mlp, head):
    """(ActorCriticNet, PolicyNet) holding `mlp` (torch.nn.Linear's layout, as the yardsticks keep it) and `head`."""
    from tiler_slider_amd import ActorCriticNet, PolicyNet
    H, D = mlp[0].shape
    acn, pn = ActorCriticNet(D, H, env.device), PolicyNet(D, H, env.device)
    with torch.no_grad():
        for p, a in zip((acn.w1, acn.b1, acn.w2, acn.b2, acn.wv, acn.bv), ar.kernel_layout(mlp, head)):
            p.copy_(torch.from_numpy(a))
        for p, a in zip((pn.w1, pn.b1, pn.w2, pn.b2), ar.kernel_layout(mlp, head)[:4]):
            p.copy_(torch.from_numpy(a))
    return acn, pn


def _net_of(nets, leaf):
    return {VALUE: nets[0], QMAX: nets[1], ZERO: None}[leaf]


def _reward(w):
    from tiler_slider_amd import RewardWeights
    return RewardWeights(step=w[0], win=w[1], invalid=w[2])


def _host(got):
    return {k: getattr(got, k).cpu().numpy() for k in ("q", "value", "best", "win_in")}


def _assert_conditions(ref, S, ctx):
    c = lr.conditions(ref)
    print(ctx, {k: np.round(v, 3).tolist() for k, v in c.items()})
    assert c["win"] >= 0.25 and min(c["best"]) >= 0.05 and c["invalid"] >= 0.01, (ctx, c)
    if S <= 4:
        assert c["won0"] > 0, (ctx, c)


def _assert_exact(got, ref, ctx):
    """All four outputs bit for bit (the yardstick's float64 values are exactly representable), and the won boards' constants."""
    np.testing.assert_array_equal(_bits(got["q"]), _bits(ref["q"]), err_msg=str(ctx))
    np.testing.assert_array_equal(_bits(got["value"]), _bits(ref["value"]), err_msg=str(ctx))
    np.testing.assert_array_equal(got["best"], ref["best"], err_msg=str(ctx))
    np.testing.assert_array_equal(got["win_in"], ref["win_in"], err_msg=str(ctx))
    won = ref["won0"]
    assert not got["q"][won].any() and (got["best"][won] == 255).all() and not got["win_in"][won].any()


def _guard_exactness(ref, ctx):
    q = ref["q"]
    assert np.array_equal(q * 16, np.round(q * 16)) and np.abs(q).max() < 2 ** 20, ctx   # multiples of 1 / 16 far below 2**20


# (S, T, obstacles, multi colour, targets or None for T, the conditions hold): 257 boards each, a ragged last wave
EXACT_SHAPES = {"4x4/2": (4, 2, 2, False, None, True), "5x5/3 multi": (5, 3, 3, True, None, True), "8x8/2": (8, 2, 10, False, None, True),
                "3x3/4": (3, 4, 1, False, None, True), "1x1": (1, 1, 0, False, None, False), "4x4/2 three targets": (4, 2, 2, False, 3, True),
                "4x4 no tiles": (4, 0, 2, False, 0, False), "4x4 no tiles, targets": (4, 0, 2, True, 2, False)}


# ---------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("shape", sorted(EXACT_SHAPES))
def test_integer_networks_back_up_bit_for_bit(torch_cuda, oracle, shape):
    """Integer weights in [-4, 4] (the head in [-2, 2]), 16 hidden units, gamma in {1, 1 / 2}, w_step = -1, w_win = 8,
    w_invalid = -2: every value is a multiple of 1 / 16 far below 2**20, so float32 in any order is the float64 yardstick: q, value,
    best and win_in bit for bit, three leaf kinds, depths 1 .. 4, 257 boards as they stand."""
    torch = torch_cuda
    S, T, K, mc, Tt, cond = EXACT_SHAPES[shape]
    n, H = 257, 16
    Tt_ = T if Tt is None else Tt
    blk, init, tgt = lr.near_win_levels(oracle, S, T, K, n, mc, Tt)
    mlp, head = lr.int_network(np.random.default_rng(7 * S + T), lr.features(S, T, Tt_, mc), H)
    plies = lr.expand(oracle, S, mc, blk, tgt, init, 4)
    env = _env(S, mc, blk, init, tgt)
    nets = _nets(torch, env, mlp, head)
    for depth in (1, 2, 3, 4):
        for leaf in (ZERO, VALUE, QMAX):
            for gamma in (1.0, 0.5):
                ctx = (shape, depth, LEAF_NAMES[leaf], gamma)
                ref = lr.search(oracle, S, mc, blk, tgt, init, depth, leaf, gamma, W_EXACT, mlp, head, plies=plies)
                _guard_exactness(ref, ctx)
                if cond and gamma == 0.5:
                    _assert_conditions(ref, S, ctx)
                elif not cond:   # 1x1 with its tile on its target, no tiles and no targets: all won; no tiles but targets: none
                    assert ref["won0"].all() or (not ref["won0"].any() and not ref["win_in"].any()), ctx
                got = env.lookahead(_net_of(nets, leaf), depth=depth, gamma=gamma, reward=_reward(W_EXACT))
                assert got.q.grad_fn is None and got.q.dtype == torch.float32 and got.best.dtype == torch.uint8 and got.win_in.dtype == torch.uint8
                assert tuple(got.q.shape) == (n, 4) and tuple(got.value.shape) == tuple(got.best.shape) == tuple(got.win_in.shape) == (n,)
                _assert_exact(_host(got), ref, ctx)
    # an ActorCriticNet may ask for the largest logit; a PolicyNet has no value head; the defaults are the table's
    ref = lr.search(oracle, S, mc, blk, tgt, init, 2, QMAX, 0.5, W_EXACT, mlp, head, plies=plies)
    _assert_exact(_host(env.lookahead(nets[0], depth=2, leaf="qmax", gamma=0.5, reward=_reward(W_EXACT))), ref, (shape, "ac qmax"))
    _assert_exact(_host(env.lookahead(nets[1].policy(), depth=2, gamma=0.5, reward=_reward(W_EXACT))), ref, (shape, "MlpPolicy"))
    with pytest.raises(ValueError, match="value head"):
        env.lookahead(nets[1], leaf="value")
    with pytest.raises(ValueError, match="needs a network"):
        env.lookahead(None, leaf="qmax")
    from tiler_slider_amd import RewardWeights
    for field in ("timeout", "dist", "progress"):
        with pytest.raises(ValueError, match=field):
            env.lookahead(None, reward=RewardWeights(**{field: 0.5}))
    for bad in ({"depth": 0}, {"depth": 5}, {"gamma": 1.5}, {"leaf": "best"}):
        with pytest.raises(ValueError):
            env.lookahead(nets[0], **bad)
    with pytest.raises(TypeError):
        env.lookahead(mlp)


# ---------------------------------------------------------------------------------------------- 2. bounded
# (S, T, obstacles, multi colour, H, boards, depths): Gaussian weights; 8x8 / 8 multi colour at 29 units gathers its weights from L2
BOUNDED = {"4x4/2 H=1": (4, 2, 2, False, 1, 257, (1, 2, 3, 4)), "5x5/3 multi H=7": (5, 3, 3, True, 7, 257, (1, 2, 3, 4)),
           "3x3/4 H=16": (3, 4, 1, False, 16, 257, (1, 2, 3, 4)), "8x8/2 H=64": (8, 2, 10, False, 64, 500, (1, 2, 3)),
           "8x8/8 multi H=29": (8, 8, 6, True, 29, 500, (1, 2, 3))}
W_REAL = (-0.3, 1.7, -0.6)


@pytest.mark.parametrize("case", sorted(BOUNDED))
def test_gaussian_networks_stay_inside_the_bound(torch_cuda, oracle, case):
    """Gaussian weights, gamma = 0.97, real reward weights: every q within the yardstick's bound of the float64 value; `best` the
    lowest index among the STORED q equal to their maximum and `value` that q, bit for bit, no exclusions; win_in exact."""
    torch = torch_cuda
    from tiler_slider_amd import _lookahead_cabi as lc
    S, T, K, mc, H, n, depths = BOUNDED[case]
    blk, init, tgt = lr.near_win_levels(oracle, S, T, K, n, mc)
    rng = np.random.default_rng(1000 + H)
    mlp, head = pref.random_mlp(rng, lr.features(S, T, T, mc), H), ar.random_head(rng, H)
    plies = lr.expand(oracle, S, mc, blk, tgt, init, max(depths))
    env = _env(S, mc, blk, init, tgt)
    assert lc.describe_lookahead(env._dims, H, 1, 2, VALUE)["weights_in_lds"] == (0 if case == "8x8/8 multi H=29" else 1)
    nets = _nets(torch, env, mlp, head)
    for depth in depths:
        for leaf in (VALUE, QMAX, ZERO):
            ctx = (case, depth, LEAF_NAMES[leaf])
            ref = lr.search(oracle, S, mc, blk, tgt, init, depth, leaf, 0.97, W_REAL, mlp, head, plies=plies)
            _assert_conditions(ref, S, ctx)
            got = _host(env.lookahead(_net_of(nets, leaf), depth=depth, gamma=0.97, reward=_reward(W_REAL)))
            err = np.abs(got["q"].astype(np.float64) - ref["q"])
            alive = ~ref["won0"]
            print(ctx, f"worst error / bound {float((err[alive] / ref['qbound'][alive]).max()):.3f}, median bound {float(np.median(ref['qbound'][alive])):.2e}")
            assert (err <= ref["qbound"]).all(), ctx
            stored_best = np.argmax(got["q"] == got["q"].max(axis=1, keepdims=True), axis=1)
            np.testing.assert_array_equal(got["best"], np.where(ref["won0"], 255, stored_best), err_msg=str(ctx))
            np.testing.assert_array_equal(_bits(got["value"]), _bits(got["q"][np.arange(n), stored_best]), err_msg=str(ctx))
            np.testing.assert_array_equal(got["value"], got["q"].max(axis=1), err_msg=str(ctx))
            np.testing.assert_array_equal(got["win_in"], ref["win_in"], err_msg=str(ctx))
            assert not got["q"][ref["won0"]].any()


# ---------------------------------------------------------------------------------------------- 3. the distance tables
@pytest.mark.parametrize("S,T,K", ((4, 2, 2), (3, 4, 1)))
def test_plain_reward_search_is_the_distance_table_inside_the_horizon(torch_cuda, oracle, S, T, K):
    """LEAF_ZERO, gamma = 1, w_step = -1 and nothing else: value = -min(dist, depth), win_in = dist where dist <= depth and 0
    beyond, and where dist < depth the search's move is the table's expert's (both the lowest move that starts a shortest solution;
    at dist = depth every move scores -depth) - dist from build_table() / lookup() on the same boards, which share nothing with
    the search but the slide."""
    torch = torch_cuda
    from tiler_slider_amd import RewardWeights
    n = 1000
    for mc in (False, True):
        blk, init, tgt = lr.near_win_levels(oracle, S, T, K, n, mc)
        env = _env(S, mc, blk, init, tgt)
        table = env.build_table()
        moves = env.lookup(table)[0].cpu().numpy().astype(np.int64)
        expert = env.expert_actions_from(table).cpu().numpy()
        dist = np.where(moves >= 0, moves, 1 << 20)
        assert (dist == 0).any() and ((dist >= 1) & (dist <= 4)).mean() > 0.5
        for depth in (1, 2, 3, 4):
            got = _host(env.lookahead(None, depth=depth, gamma=1.0, reward=RewardWeights(step=-1.0, win=0.0)))
            np.testing.assert_array_equal(got["value"], np.where(dist == 0, 0, -np.minimum(dist, depth)).astype(np.float32))
            np.testing.assert_array_equal(got["win_in"], np.where(dist <= depth, dist, 0))
            assert ((dist >= 1) & (dist <= depth)).mean() >= 0.25
            near = (dist >= 1) & (dist < depth)
            assert depth == 1 or near.mean() >= 0.25
            np.testing.assert_array_equal(got["best"][near], expert[near])
            assert (got["best"][dist == 0] == 255).all()


# ---------------------------------------------------------------------------------------------- 4. the trajectory form
def test_a_logged_rollout_is_searched_row_by_row_and_depth_one_is_dqns_target(torch_cuda, oracle):
    """1,000 boards, an integer PolicyNet playing 8 greedy steps, half of them explored, with its start and cells logged: row k of lookahead(rollout=) is
    lookahead() of a twin environment standing on c[k], for every output; and DQN's identity, exactly: at depth 1
    q[k, n, a] = r + gamma max trajectory_logits(net) on the successor - the twin stepped with the constant action a - and r alone
    where the successor is won.  td_targets() is that q."""
    torch = torch_cuda
    S, T, K, mc, n, H, steps = 4, 2, 2, False, 1000, 16, 8
    blk, init, tgt = lr.near_win_levels(oracle, S, T, K, n, mc)
    mlp, head = lr.int_network(np.random.default_rng(4), lr.features(S, T, T, mc), H)
    env = _env(S, mc, blk, init, tgt, auto_reset=True)
    acn, pn = _nets(torch, env, mlp, head)
    out = env.rollout_policy(steps, pn.policy(), select="greedy", epsilon=0.5, seed=5, log=("start", "pos"))
    reward = _reward(W_EXACT)
    full = {(d, leaf): env.lookahead(net, depth=d, rollout=out, gamma=0.5, reward=reward)
            for d, net, leaf in ((1, pn, QMAX), (2, acn, VALUE), (3, None, ZERO))}
    for got in full.values():
        assert tuple(got.q.shape) == (steps, n, 4) and tuple(got.best.shape) == (steps, n) and got.q.is_contiguous()
    cells = torch.cat([out.start_pos[None], out.pos_log[:steps - 1]], dim=0)
    ref = lr.trajectory(oracle, S, mc, blk, tgt, out.start_pos.cpu().numpy(), out.pos_log.cpu().numpy(), 2, VALUE, 0.5, W_EXACT, mlp, head)
    _assert_conditions(ref, S, "trajectory")
    _assert_exact({k: v.reshape((steps * n,) + v.shape[2:]) for k, v in _host(full[(2, VALUE)]).items()},
                  {k: v.reshape((steps * n,) + v.shape[2:]) for k, v in ref.items()}, "trajectory")
    assert len({bytes(cells[k].cpu().numpy()) for k in range(steps)}) == steps       # the rows are different boards
    twin = _env(S, mc, blk, init, tgt)
    td = env.td_targets(pn, out, gamma=0.5, reward=reward)
    assert torch.equal(td, full[(1, QMAX)].q)
    seen_won = seen_invalid = 0
    for k in range(steps):
        twin._pos.copy_(cells[k])
        for (d, leaf), got in full.items():
            row = twin.lookahead({QMAX: pn, VALUE: acn, ZERO: None}[leaf], depth=d, gamma=0.5, reward=reward)
            for name in ("q", "value", "best", "win_in"):
                assert torch.equal(getattr(got, name)[k], getattr(row, name)), (k, d, name)
        won_now = twin.is_won()
        for a in range(4):
            twin._pos.copy_(cells[k])
            twin._done.zero_()
            _, _, info = twin.step(torch.full((n,), a, dtype=torch.uint8, device=env.device))
            won, same = info["is_won"].clone(), info["invalid_move"].clone()
            with torch.no_grad():
                z = twin.trajectory_logits(pn)[0]
            want = -1.0 + 8.0 * won.float() - 2.0 * same.float() + 0.5 * torch.where(won, torch.zeros_like(z[:, 0]), z.max(dim=1).values)
            want = torch.where(won_now, torch.zeros_like(want), want)
            assert torch.equal(td[k, :, a], want), (k, a)
            seen_won += int(won.sum())
            seen_invalid += int(same.sum())
    assert seen_won > 0 and seen_invalid > 0
    bad = env.rollout_policy(2, pn.policy(), log=("pos",))
    with pytest.raises(ValueError):
        env.lookahead(pn, rollout=bad)


# ---------------------------------------------------------------------------------------------- 5. the raw C-ABI
def test_raw_calls_write_what_is_asked_for_and_nothing_else(torch_cuda, oracle):
    """ts_lookahead itself into buffers between guard bytes, prefilled with the complement of the answer: all four outputs at
    once, each one alone (the others NULL: nothing else is written, the guards stand), steps = 1 with pos_log = NULL, and a
    logged trajectory of three steps whose unread last row is poisoned with cell ids past the board."""
    torch = torch_cuda
    from tiler_slider_amd import _lookahead_cabi as lc
    S, T, K, mc, n, H = 4, 2, 2, False, 257, 16
    blk, init, tgt = lr.near_win_levels(oracle, S, T, K, n, mc)
    mlp, head = lr.int_network(np.random.default_rng(9), lr.features(S, T, T, mc), H)
    env = _env(S, mc, blk, init, tgt)
    dev = env.device
    kl = [torch.from_numpy(a).to(dev) for a in ar.kernel_layout(mlp, head)]
    cmlp, chead = lc.Mlp(*(t.data_ptr() for t in kl[:4]), H, 0), lc.ValueHead(kl[4].data_ptr(), kl[5].data_ptr())
    stream = torch.cuda.current_stream(dev).cuda_stream
    b = lr._batch(oracle, S, mc, blk, tgt, init)
    rows = []
    for k in range(2):
        b.done[...] = 0
        b.step(oracle.fill_actions(n, 0xAB1, k), obs=False)
        rows.append(b.pos.copy())
    pos_log = np.stack(rows + [np.full_like(init, 200)])                                 # the last row is never read
    first_d, log_d = torch.from_numpy(init).to(dev), torch.from_numpy(pos_log).to(dev)
    shapes = {"q": (np.float32, (4,)), "value": (np.float32, ()), "best": (np.uint8, ()), "win_in": (np.uint8, ())}
    for steps, log in ((1, None), (3, log_d)):
        ref = lr.trajectory(oracle, S, mc, blk, tgt, init, pos_log[:steps], 2, VALUE, 0.5, W_EXACT, mlp, head)
        want = {"q": ref["q"].astype(np.float32), "value": ref["value"].astype(np.float32), "best": ref["best"], "win_in": ref["win_in"]}
        tin = lc.TrainIn(first_d.data_ptr(), log.data_ptr() if log is not None else None, steps, 0)
        cfg = lc.LookaheadCfg(2, VALUE, 0.5, *W_EXACT)
        for asked in (("q", "value", "best", "win_in"), ("q",), ("value",), ("best",), ("win_in",)):
            fill = {k: ~np.ascontiguousarray(want[k]).view(np.uint8) for k in want}
            bufs = {k: _guarded(torch, dev, fill[k]) for k in want}
            ptr = lambda k: bufs[k].data_ptr() + 256 if k in asked else None
            out = lc.LookaheadOut(ptr("q"), ptr("value"), ptr("best"), ptr("win_in"))
            assert bufs["q"].data_ptr() % 16 == 0
            rc = lc.lib().ts_lookahead(C.byref(env._dims), C.byref(env._state), C.byref(cmlp), C.byref(chead), C.byref(tin), C.byref(cfg),
                                       C.byref(out), stream)
            assert rc == 0, (steps, asked, rc)
            for k, (dtype, tail) in shapes.items():
                got = _payload(bufs[k], dtype, (steps, n) + tail)
                expect = want[k] if k in asked else fill[k].view(dtype).reshape((steps, n) + tail)
                np.testing.assert_array_equal(got.view(np.uint8), np.ascontiguousarray(expect).view(np.uint8), err_msg=str((steps, asked, k)))
    assert lc.lib().ts_lookahead_last_hip_error() == 0


# ---------------------------------------------------------------------------------------------- 6. every kernel at occupancy
_OCC_SHAPES = {1: (1, 0), 2: (1, 0), 3: (2, 1), 4: (2, 2), 5: (2, 3), 6: (2, 6), 7: (2, 8), 8: (2, 10)}   # size -> (tiles, obstacles)
OCCUPANCY_CASES = {f"k_lookahead<{S}, {D}>": (S, T, K, D) for S, (T, K) in _OCC_SHAPES.items() for D in (1, 2, 3, 4)}


def test_the_occupancy_cases_are_the_compiled_kernels():
    from cabi_harness import _kernel_names
    from tiler_slider_amd import _lookahead_cabi as lc
    assert sorted(OCCUPANCY_CASES) == _kernel_names(lc.LIB_PATH)


@pytest.mark.parametrize("kernel", sorted(OCCUPANCY_CASES))
def test_every_kernel_at_4096_waves(torch_cuda, oracle, kernel):
    """262,144 lanes - 4,096 waves - replicate 1,024 distinct boards (256 at depth 4, so the yardstick's 4^D leaves stay few): 64
    hidden units, integer weights, leaf "value", all four outputs exactly, and the describe call names the kernel under test."""
    torch = torch_cuda
    from tiler_slider_amd import _lookahead_cabi as lc
    S, T, K, D = OCCUPANCY_CASES[kernel]
    lanes, distinct, H = 262144, (256 if D == 4 else 1024), 64
    blk, init, tgt = lr.near_win_levels(oracle, S, T, K, distinct, False)
    mlp, head = lr.int_network(np.random.default_rng(S + 10 * D), lr.features(S, T, T, False), H)
    ref = lr.search(oracle, S, False, blk, tgt, init, D, VALUE, 0.5, W_EXACT, mlp, head)
    _guard_exactness(ref, kernel)
    if S >= 2:
        assert (ref["win_in"] > 0).mean() >= 0.25 and set(ref["best"].tolist()) >= {0, 1, 2, 3}, kernel
    reps = lanes // distinct
    env = _env(S, False, np.tile(blk, (1, reps)), np.tile(init, (1, reps)), np.tile(tgt, (1, reps)))
    d = lc.describe_lookahead(env._dims, H, 1, D, VALUE)
    assert d["name"] == kernel and d["blocks"] * d["threads_per_block"] == lanes and d["leaves"] == lanes * 4 ** D
    net = _nets(torch, env, mlp, head)[0]
    got = _host(env.lookahead(net, depth=D, gamma=0.5, reward=_reward(W_EXACT)))
    tiled = {k: np.tile(v, (reps,) + (1,) * (v.ndim - 1)) for k, v in ref.items() if k in ("q", "value", "best", "win_in", "won0")}
    _assert_exact(got, tiled, kernel)


# ---------------------------------------------------------------------------------------------- 7. stream ordering
def test_a_call_on_a_stream_of_its_own_runs_behind_the_step_before_it(torch_cuda, oracle):
    """On a side stream: a step() and the lookahead behind it, 262,144 boards, then the same on the default stream after a
    synchronisation: the search saw the stepped cells, not the ones before."""
    torch = torch_cuda
    S, T, K, mc, distinct, H = 4, 2, 2, False, 1024, 16
    blk, init, tgt = lr.near_win_levels(oracle, S, T, K, distinct, mc)
    reps = 256
    mlp, head = lr.int_network(np.random.default_rng(3), lr.features(S, T, T, mc), H)
    env = _env(S, mc, np.tile(blk, (1, reps)), np.tile(init, (1, reps)), np.tile(tgt, (1, reps)), auto_reset=True)
    net = _nets(torch, env, mlp, head)[0]
    n = env.num_envs
    act = torch.from_numpy(np.tile(oracle.fill_actions(distinct, 0x57, 0), reps)).to(env.device)
    before = _host(env.lookahead(net, depth=2, gamma=0.5, reward=_reward(W_EXACT)))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=env.device)
    with torch.cuda.stream(side):
        env.step(act)
        got = env.lookahead(net, depth=2, gamma=0.5, reward=_reward(W_EXACT))
    side.synchronize()
    got = _host(got)
    b = lr._batch(oracle, S, mc, blk, tgt, init)
    b.step(act[:distinct].cpu().numpy(), obs=False)
    ref = lr.search(oracle, S, mc, blk, tgt, b.pos, 2, VALUE, 0.5, W_EXACT, mlp, head)
    tiled = {k: np.tile(v, (reps,) + (1,) * (v.ndim - 1)) for k, v in ref.items() if k in ("q", "value", "best", "win_in", "won0")}
    _assert_exact(got, tiled, "side stream")
    assert (got["q"] != before["q"]).any(axis=1).mean() > 0.25 and got["q"].shape == (n, 4)
