"""The fused rollouts on the GPU (lib/libtiler_slider_rollout.so, VecTilerSliderEnv.rollout) against the CPU yardstick
tests/rollout_reference.py - the loop of include/tiler_slider_rollout.h on NumPy and the oracle - and against the shipped
entry points ts_fill_actions / ts_table_lookup / ts_step driven one step at a time."""
import ctypes as C

import numpy as np
import pytest

import rollout_reference as rref
from table_harness import GUARD, guarded as _guarded, payload as _payload

pytestmark = pytest.mark.gpu

ALL_LOGS = ("act", "flags", "pos")
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


def _state(env):
    return {k: getattr(env, "_" + k).cpu().numpy().copy() for k in ("pos", "step_count", "done", "flags")}


def _check(got, env, want, ctx, outputs=rref.OUTPUTS, state=True):
    """Every output of a Rollout, and the environment's state after an advancing call, against the yardstick's dict."""
    for name in outputs:
        t = getattr(got, name)
        assert t is not None, (ctx, name)
        np.testing.assert_array_equal(t.cpu().numpy(), want[name], err_msg=f"{ctx}: {name}")
    if state:
        for name in ("pos", "step_count", "done"):
            np.testing.assert_array_equal(getattr(env, "_" + name).cpu().numpy(), want[name], err_msg=f"{ctx}: {name} after the call")
        np.testing.assert_array_equal(env._flags.cpu().numpy(), want["flags"], err_msg=f"{ctx}: the environment's flag byte")


# ---------------------------------------------------------------------------------------------- every output against the yardstick
# (policy, S, T, obstacles, multi colour, n, max_steps, K, epsilon) on the reference's seeded levels (generate_mt19937, seeds 0 .. n-1)
CASES = ((rref.RANDOM, 4, 2, 2, False, 3000, 6, 40, None),
         (rref.TABLE, 4, 2, 2, True, 3000, 12, 60, 0.25),
         (rref.TABLE, 5, 2, 3, False, 2000, 8, 40, 0.1),
         (rref.TABLE, 5, 3, 3, True, 300, 20, 50, 0.25),
         (rref.TABLE, 8, 2, 10, True, 500, 15, 40, 0.5))
RUNS = [(i, AUTORESET) for i in range(len(CASES))] + [(0, STRICT), (1, STRICT)]
SEED = 0x0110CA5E


def yardstick_case(oracle, case, mode):
    """Levels, table and the yardstick's answer of one case, with the assertions that keep the case from passing on idle boards -
    all on the YARDSTICK's numbers: some board wins, some board times out, (auto-reset mode: strict mode cannot reset) some board
    auto-resets, and each of the three action sources of the table policy supplies at least 1 % of the board-steps."""
    import table_reference as tref
    policy, S, T, K, mc, n, max_steps, steps, eps = CASES[case]
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    table = tref.table(oracle, S, mc, blk, tgt, T) if policy == rref.TABLE else None
    want = rref.rollout(oracle, S, mc, max_steps, blk, init, tgt, steps, policy, mode, table=table,
                        threshold=rref.threshold_of(eps or 0.0), seed=SEED + case, step_index=case * 1000, board_offset=case * 77)
    share = want["source"] / float(n * steps)
    print(f"case {case} mode {mode}: boards winning {want['won'].mean():.3f}, timing out {want['timed_out'].mean():.3f}, resetting "
          f"{want['reset'].mean():.3f}; board-steps by expert / exploration / fallback {share.round(3).tolist()}")
    assert want["won"].any() and want["timed_out"].any()
    if mode == AUTORESET:
        assert want["reset"].any()
    else:
        assert ((want["flags_log"] & rref.FLAG_STEPPED_DONE) != 0).any()
    if policy == rref.TABLE:
        assert (share >= 0.01).all(), share
    return (blk, init, tgt), table, want


@pytest.mark.parametrize("case,mode", RUNS)
def test_every_output_against_the_yardstick(torch_cuda, oracle, case, mode):
    policy, S, T, K, mc, n, max_steps, steps, eps = CASES[case]
    (blk, init, tgt), table, want = yardstick_case(oracle, case, mode)
    env = _env(S, mc, blk, init, tgt, max_steps, mode)
    kw = dict(seed=SEED + case, step_index=case * 1000, board_offset=case * 77)
    if policy == rref.TABLE:
        built = env.build_table()
        np.testing.assert_array_equal(built.dist.cpu().numpy(), table)
        kw.update(table=built, epsilon=eps)
    got = env.rollout(steps, "table" if policy == rref.TABLE else "random", log=ALL_LOGS, **kw)
    _check(got, env, want, (case, mode))
    assert got.steps == steps and env._started


# ---------------------------------------------------------------------------------------------- against the shipped entry points
@pytest.mark.parametrize("policy,mode", (("random", AUTORESET), ("table", AUTORESET), ("table", STRICT)))
def test_a_twin_driven_step_by_step_ends_byte_equal(torch_cuda, oracle, policy, mode):
    """ts_fill_actions + expert_actions_from + step(), K times, on a twin environment: state, last flags and the staged actions
    are the fused call's, byte for byte.  Some tiles and targets carry cell ids beyond the board (kept by boards that never move)."""
    torch = torch_cuda
    from tiler_slider_amd import _cabi
    S, T, K, mc, n, max_steps, steps, eps = 4, 2, 2, True, 3001, 9, 30, 0.25
    seed, step_index, offset = 0x7171, 5, 11
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    safe = ((blk[0] >> 15) & 1) == 0                                  # cell 15 is free: an id beyond the board clamps onto it
    safe &= (init != 15).all(axis=0)
    init[0, safe & (np.arange(n) % 7 == 0)] = 200
    tgt[1, np.arange(n) % 5 == 0] = 255
    fused, twin = _env(S, mc, blk, init, tgt, max_steps, mode), _env(S, mc, blk, init, tgt, max_steps, mode)
    table = fused.build_table() if policy == "table" else None
    for env in (fused, twin):
        _put(env, "_pos", init)   # reset() stored clamped cells: the ids beyond the board go back in
        if mode == STRICT:        # boards that are done from the start never move: their cells stay as they are
            env._done[::3] = 1
    got = fused.rollout(steps, policy, table=table, epsilon=eps if table is not None else 0.0, seed=seed, step_index=step_index,
                        board_offset=offset, log=("act",))
    act = torch.empty(n, dtype=torch.uint8, device=twin.device)
    stream = torch.cuda.current_stream(twin.device).cuda_stream
    sources = np.zeros(3, np.int64)
    for k in range(steps):
        assert _cabi.lib().ts_fill_actions(n, seed, offset, step_index + k, act.data_ptr(), stream) == 0
        a = act
        if table is not None:
            e = twin.expert_actions_from(table)
            r = rref.draws(n, seed, step_index + k, offset)
            explore = torch.from_numpy((r & np.uint64(0xffffffff)) < np.uint64(rref.threshold_of(eps))).to(twin.device)
            a = torch.where(explore | (e == 255), act, e)
            sources += (int((~explore & (e != 255)).sum()), int(explore.sum()), int((~explore & (e == 255)).sum()))
        assert torch.equal(got.act_log[k], a), (policy, mode, k)
        twin.step(a)
    if table is not None:
        assert (sources >= 0.01 * n * steps).all(), sources
    a, b = _state(fused), _state(twin)
    for name in a:
        np.testing.assert_array_equal(a[name], b[name], err_msg=f"{policy} mode {mode}: {name}")
    assert (a["pos"] >= 16).any() == (mode == STRICT)   # auto-reset brings every board back to clamped cells sooner or later
    np.testing.assert_array_equal(got.flags.cpu().numpy(), b["flags"])


# ---------------------------------------------------------------------------------------------- GIVEN
def _levels(oracle, S, T, Tt, K, n, seed=0x6171):
    """n random levels of any shape: the reference's seeded levels where obstacles, tiles and targets fit side by side, else tiles
    and obstacles drawn apart from the targets (which may then lie under tiles)."""
    if T == Tt and 2 * T + K <= S * S:
        return oracle.generate_mt19937(S, T, T, K, np.arange(2000, 2000 + n, dtype=np.uint32))
    blk, init, _ = oracle.generate(S, T, 0, K, n, seed=seed)
    _, _, tgt = oracle.generate(S, 0, Tt, 0, n, seed=seed + 1)
    return blk, init, tgt


def _given_actions(rng, steps, n):
    a = rng.integers(0, 4, (steps, n)).astype(np.uint8)
    bad = rng.random((steps, n)) < 0.06
    a[bad] = rng.integers(4, 256, int(bad.sum())).astype(np.uint8)
    return a


# (S, T, Tt, obstacles, what): the sizes the seeded cases leave out, eight tiles on 8x8 (the register cap), unequal counts,
# repeated targets, no tiles, cell ids beyond the board
GIVEN_SHAPES = ((1, 1, 1, 0, ""), (2, 2, 2, 1, ""), (3, 2, 2, 1, ""), (6, 2, 2, 6, ""), (7, 2, 2, 8, ""), (8, 8, 8, 6, ""), (4, 3, 2, 2, ""),
                (5, 2, 4, 3, ""), (4, 2, 8, 2, ""), (4, 3, 3, 2, "repeated targets"), (4, 0, 0, 3, ""), (5, 0, 2, 3, ""), (3, 1, 0, 1, ""),
                (4, 2, 2, 2, "beyond"), (8, 3, 3, 10, "beyond"))


@pytest.mark.parametrize("S,T,Tt,K,what", GIVEN_SHAPES)
def test_given_actions_on_every_kind_of_board(torch_cuda, oracle, S, T, Tt, K, what):
    """257 boards (a ragged last wave), 24 steps of GIVEN actions with bytes above 3 mixed in, both colour modes and both step
    modes, every output."""
    torch = torch_cuda
    n, steps, max_steps = 257, 24, 5
    rng = np.random.default_rng(S * 1000 + T * 10 + Tt)
    Cc = S * S
    for mc in (False, True):
        blk, init, tgt = _levels(oracle, S, T, Tt, K, n)
        if what == "repeated targets":
            tgt[2] = tgt[0]
        raw_init, raw_tgt = init.copy(), tgt.copy()
        if what == "beyond":   # ids S*S .. 255: the kernels clamp them to S*S - 1; the oracle is handed the clamped level
            last = Cc - 1
            safe = ((blk[last >> 5] >> (last & 31)) & 1) == 0
            safe &= (init != last).all(axis=0)
            some = safe & (rng.random(n) < 0.4)
            assert some.sum() >= 20
            raw_init[0, some] = rng.integers(Cc, 256, int(some.sum()))
            raw_tgt[Tt - 1, rng.random(n) < 0.3] = 255
            init, tgt = np.minimum(raw_init, last).astype(np.uint8), np.minimum(raw_tgt, last).astype(np.uint8)
        actions = _given_actions(rng, steps, n)
        done0 = np.zeros(n, np.uint8)
        if what == "beyond":   # boards that keep their bytes for a step (a bad action) or, in strict mode, for good (done on entry)
            first = np.flatnonzero(some)
            actions[0, first[:10]] = 255
            done0[first[10:16]] = 1
        for mode in (AUTORESET, STRICT):
            ctx = (S, T, Tt, what, mc, mode)
            want = rref.rollout(oracle, S, mc, max_steps, blk, init, tgt, steps, rref.GIVEN, mode, actions=actions, done=done0)
            assert ((want["flags_log"] & rref.FLAG_BAD_ACTION) != 0).sum() >= (50 if mode == AUTORESET else 10), ctx   # strict: a done board is flagged STEPPED_DONE whatever its action
            if T:
                assert (want["timed_out"].any() if S > 1 else want["won"].all()) and (want["reset"].any() if mode == AUTORESET else (want["flags_log"] & rref.FLAG_STEPPED_DONE).any()), ctx
            env = _env(S, mc, blk, raw_init, raw_tgt, max_steps, mode)
            _put(env, "_pos", raw_init)   # reset() stored clamped cells: the ids beyond the board go back in
            _put(env, "_done", done0)
            got = env.rollout(steps, "given", actions=torch.from_numpy(actions).to(env.device), log=ALL_LOGS)
            np.testing.assert_array_equal(got.act_log.cpu().numpy(), actions)
            if what == "beyond":   # a board that has not moved yet keeps its bytes; everything that moved is clamped
                pos_log, pos = got.pos_log.cpu().numpy(), env._pos.cpu().numpy()
                moved = np.cumsum((want["flags_log"] & (rref.FLAG_BAD_ACTION | rref.FLAG_STEPPED_DONE)) == 0, axis=0) > 0
                np.testing.assert_array_equal(pos_log, np.where(moved[:, None, :], want["pos_log"], raw_init[None]), err_msg=str(ctx))
                np.testing.assert_array_equal(pos, np.where(moved[-1][None], want["pos"], raw_init), err_msg=str(ctx))
                beyond = (raw_init >= Cc).any(axis=0)
                assert (~moved[0] & beyond).sum() >= 10 and (~moved[-1] & beyond).sum() == (6 if mode == STRICT else 0), ctx
                _check(got, env, want, ctx, outputs=[o for o in rref.OUTPUTS if o != "pos_log"], state=False)
                np.testing.assert_array_equal(env._step_count.cpu().numpy(), want["step_count"])
                np.testing.assert_array_equal(env._done.cpu().numpy(), want["done"])
            else:
                _check(got, env, want, ctx)
            env.close()


# ---------------------------------------------------------------------------------------------- advance=False
def test_a_playout_leaves_the_environment_untouched(torch_cuda, oracle):
    torch = torch_cuda
    S, T, K, mc, n, max_steps, steps = 5, 2, 3, False, 1500, 7, 25
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    env = _env(S, mc, blk, init, tgt, max_steps, AUTORESET, obs_dtype="float32")
    twin = _env(S, mc, blk, init, tgt, max_steps, AUTORESET, obs_dtype="float32")
    table = env.build_table()
    for e in (env, twin):   # somewhere in the middle of their episodes
        e.rollout(5, "random", seed=3)
    names = ("_pos", "_step_count", "_done", "_flags", "_obs", "_init", "_tgt", "_blk")
    before = {k: getattr(env, k).clone() for k in names}
    assert torch.equal(before["_obs"], env.encode(torch.empty_like(env._obs)))     # the advancing call kept the observation truthful
    for policy, kw in (("random", {}), ("table", dict(table=table, epsilon=0.2))):
        got = env.rollout(steps, policy, seed=9, advance=False, log=ALL_LOGS, **kw)
        for k in names:
            assert torch.equal(getattr(env, k), before[k]), (policy, k)
        saved = {k: getattr(twin, k).clone() for k in ("_pos", "_step_count", "_done", "_flags")}
        adv = twin.rollout(steps, policy, seed=9, log=ALL_LOGS, **kw)
        for name in rref.OUTPUTS:
            assert torch.equal(getattr(got, name), getattr(adv, name)), (policy, name)
        assert not torch.equal(twin._pos, saved["_pos"])
        assert torch.equal(twin._obs, twin.encode(torch.empty_like(twin._obs)))
        assert torch.equal(twin._flags, adv.flags)
        for k, v in saved.items():   # the twin goes back to where the playout started
            getattr(twin, k).copy_(v)
    # statistics alone, and nothing at all
    only = env.rollout(steps, "random", seed=9, advance=False, stats=("wins", "reward_sum"))
    assert only.finished is None and only.flags is None and only.act_log is None and only.wins is not None
    none = env.rollout(steps, "random", seed=9, advance=False, stats=False)
    assert all(getattr(none, f) is None for f in rref.OUTPUTS)
    for k in names:
        assert torch.equal(getattr(env, k), before[k]), k


# ---------------------------------------------------------------------------------------------- rows=
def test_rows_let_a_table_of_levels_serve_many_boards_and_rows_outside_it_play_the_random_draw(torch_cuda, oracle):
    torch = torch_cuda
    import table_reference as tref
    S, T, K, mc, L, max_steps, steps = 4, 2, 2, False, 50, 10, 30
    n = 64 * L
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(L, dtype=np.uint32))
    tab = tref.table(oracle, S, mc, blk, tgt, T)
    level = (np.arange(n) % L).astype(np.int32)
    tile = lambda a: np.ascontiguousarray(a[:, level])
    rows = level.copy()
    out = np.arange(n) % 9 == 0
    rows[out] = np.resize(np.array([-1, L, L + 1, 2**31 - 1, -2**31], np.int64), int(out.sum())).astype(np.int32)
    small = _env(S, mc, blk, init, tgt)
    table = small.build_table()
    env = _env(S, mc, tile(blk), tile(init), tile(tgt), max_steps, AUTORESET)
    want = rref.rollout(oracle, S, mc, max_steps, tile(blk), tile(init), tile(tgt), steps, rref.TABLE, AUTORESET, table=tab, rows=rows,
                        threshold=0, seed=44)
    no_table = rref.rollout(oracle, S, mc, max_steps, tile(blk), tile(init), tile(tgt), steps, rref.RANDOM, AUTORESET, seed=44)
    np.testing.assert_array_equal(want["act_log"][:, out], no_table["act_log"][:, out])     # rows outside the table: the random draw
    assert (want["act_log"][:, ~out] != no_table["act_log"][:, ~out]).mean() > 0.05 and want["source"][0] >= 0.01 * n * steps
    got = env.rollout(steps, "table", table=table, rows=torch.from_numpy(rows), seed=44, log=ALL_LOGS)
    _check(got, env, want, "rows")
    # int64 rows that would wrap into the table as int32: outside it all the same.  A playout from where the boards stand now.
    wide = env.rollout(steps, "table", table=table, rows=torch.from_numpy(rows.astype(np.int64) + np.where(out, 2**40, 0)), seed=45,
                       advance=False, log=("act",))
    again = rref.rollout(oracle, S, mc, max_steps, tile(blk), tile(init), tile(tgt), steps, rref.TABLE, AUTORESET, table=tab, rows=rows,
                         threshold=0, seed=45, pos=want["pos"], step_count=want["step_count"], done=want["done"])
    np.testing.assert_array_equal(wide.act_log.cpu().numpy(), again["act_log"])
    # host checks
    with pytest.raises(ValueError):
        env.rollout(3, "table", table=table)                                   # 50 rows for 3,200 boards: rows= is needed
    with pytest.raises(TypeError):
        env.rollout(3, "table", table=table.dist, rows=rows)
    with pytest.raises(TypeError):
        env.rollout(3, "given", actions=torch.zeros((3, n), dtype=torch.int64, device=env.device))
    with pytest.raises(TypeError):
        env.rollout(3, "given", actions=torch.zeros((2, n), dtype=torch.uint8, device=env.device))
    with pytest.raises(ValueError):
        env.rollout(3, "expert")
    with pytest.raises(ValueError):
        env.rollout(70000)
    with pytest.raises(ValueError):
        env.rollout(3, "table", table=table, rows=rows, epsilon=1.5)
    big = _env(9, False, *oracle.generate(9, 2, 2, 3, 4, seed=1))
    with pytest.raises(ValueError, match="8x8"):
        big.rollout(3)
    many = _env(8, False, *oracle.generate(8, 3, 3, 3, 4, seed=1))
    with pytest.raises(ValueError, match="65536"):
        many.rollout(3, "table", table=table)
    assert many.rollout(3).wins is not None


# ---------------------------------------------------------------------------------------------- the raw C-ABI into guarded memory
def _raw_call(torch, env, cfg, bufs, ask):
    from tiler_slider_amd import _cabi, _rollout_cabi as rc
    st = _cabi.State(*(bufs[k].data_ptr() + GUARD for k in ("pos", "init", "tgt", "blk", "step_count", "done")), None)
    out = rc.RolloutOut(*(bufs[f].data_ptr() + GUARD if f in ask else None for f in rc.OUT_FIELDS))
    return rc.lib().ts_rollout(C.byref(env._dims), C.byref(st), C.byref(cfg), C.byref(out), torch.cuda.current_stream(env.device).cuda_stream)


@pytest.mark.parametrize("policy", (rref.GIVEN, rref.RANDOM, rref.TABLE))
def test_raw_calls_into_guarded_memory(torch_cuda, oracle, policy):
    """Every buffer of a call between 256 guard bytes, outputs prefilled with the complement of the expected bytes: no guard byte
    changes, outputs not asked for keep their fill, write_state = 0 touches no state byte, steps = 0 writes nothing."""
    torch = torch_cuda
    import table_reference as tref
    from tiler_slider_amd import _rollout_cabi as rc
    S, T, K, mc, n, max_steps, steps = 5, 2, 3, True, 257, 6, 17
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    tab = tref.table(oracle, S, mc, blk, tgt, T)
    rng = np.random.default_rng(policy)
    actions = _given_actions(rng, steps, n)
    env = _env(S, mc, blk, init, tgt, max_steps, AUTORESET)
    start = rref.rollout(oracle, S, mc, max_steps, blk, init, tgt, 4, rref.RANDOM, AUTORESET, seed=1)     # somewhere mid-episode
    kw = dict(pos=start["pos"], step_count=start["step_count"], done=start["done"])
    want = rref.rollout(oracle, S, mc, max_steps, blk, init, tgt, steps, policy, AUTORESET, actions=actions, table=tab,
                        threshold=rref.threshold_of(0.3), seed=21, step_index=3, **kw)
    dev = env.device
    act_buf, tab_buf = _guarded(torch, dev, actions), _guarded(torch, dev, tab)

    def fresh():
        bufs = {"pos": start["pos"], "init": init, "tgt": tgt, "blk": blk, "step_count": start["step_count"], "done": start["done"]}
        bufs.update({f: ~want[f] for f in rref.OUTPUTS})
        return {k: _guarded(torch, dev, v) for k, v in bufs.items()}

    def cfg(steps=steps, write_state=1):
        return rc.RolloutCfg(steps, AUTORESET, policy, write_state, act_buf.data_ptr() + GUARD, 21, 3, 0, rref.threshold_of(0.3),
                             tab_buf.data_ptr() + GUARD, n, None)

    def read(bufs, name, like):
        return _payload(bufs[name], like.dtype, like.shape)

    # everything asked for
    bufs = fresh()
    assert _raw_call(torch, env, cfg(), bufs, rref.OUTPUTS) == 0
    for f in rref.OUTPUTS + ("pos", "step_count", "done"):
        np.testing.assert_array_equal(read(bufs, f, want[f]), want[f], err_msg=f)
    for f, v in (("init", init), ("tgt", tgt), ("blk", blk)):
        np.testing.assert_array_equal(read(bufs, f, v), v, err_msg=f)
    _payload(act_buf, np.uint8, actions.shape), _payload(tab_buf, np.uint8, tab.shape)
    # a subset, no state written: the rest keeps its fill, the state its bytes
    for ask in (("wins", "pos_log"), ("flags",), ("reward_sum", "act_log", "first_win")):
        bufs = fresh()
        assert _raw_call(torch, env, cfg(write_state=0), bufs, ask) == 0
        for f in rref.OUTPUTS:
            np.testing.assert_array_equal(read(bufs, f, want[f]), want[f] if f in ask else ~want[f], err_msg=f"{ask}: {f}")
        for f in ("pos", "step_count", "done"):
            np.testing.assert_array_equal(read(bufs, f, start[f]), start[f], err_msg=f"{ask}: {f}")
    # no output, the state alone
    bufs = fresh()
    assert _raw_call(torch, env, cfg(), bufs, ()) == 0
    for f in rref.OUTPUTS:
        np.testing.assert_array_equal(read(bufs, f, want[f]), ~want[f], err_msg=f)
    for f in ("pos", "step_count", "done"):
        np.testing.assert_array_equal(read(bufs, f, want[f]), want[f], err_msg=f)
    # steps = 0: nothing at all
    bufs = fresh()
    assert _raw_call(torch, env, cfg(steps=0), bufs, rref.OUTPUTS) == 0
    for f in rref.OUTPUTS:
        np.testing.assert_array_equal(read(bufs, f, want[f]), ~want[f], err_msg=f)
    for f in ("pos", "step_count", "done"):
        np.testing.assert_array_equal(read(bufs, f, start[f]), start[f], err_msg=f)


# ---------------------------------------------------------------------------------------------- every compiled kernel at occupancy
OCC_WAVES, OCC_STEPS, OCC_MAX_STEPS = 4096, 6, 3


def _occupancy_levels(oracle, S, T, K, mc, n):
    if S == 1:   # one cell: the tile sits on its target (won), or there is no target to sit on (single colour: never won)
        return np.zeros((1, n), np.uint32), np.zeros((1, n), np.uint8), np.zeros((1 if mc else 0, n), np.uint8)
    return _levels(oracle, S, T, T, K, n, seed=0x50F7)


@pytest.mark.parametrize("name", sorted(rref.OCCUPANCY_CASES))
def test_every_compiled_rollout_kernel_at_occupancy(torch_cuda, oracle, name):
    """Every kernel of the rollout library at 4,096 waves and a ragged last one - one wave per SIMD and more on every CU - on 128
    distinct levels in turn: every board's outputs and state are the yardstick's.  (RANDOM and TABLE draw per board index, so the
    yardstick plays all 262,141 boards.)"""
    torch = torch_cuda
    import table_reference as tref
    from tiler_slider_amd import _rollout_cabi as rc
    S, T, K, policy = rref.OCCUPANCY_CASES[name]
    distinct, n = 128, OCC_WAVES * 64 - 3
    level = (np.arange(n) % distinct).astype(np.int32)
    mc = S % 2 == 0
    blk, init, tgt = _occupancy_levels(oracle, S, T, K, mc, distinct)
    tile = lambda a: np.ascontiguousarray(a[:, level])
    env = _env(S, mc, tile(blk), tile(init), tile(tgt), OCC_MAX_STEPS, AUTORESET)
    cfg = rc.RolloutCfg(OCC_STEPS, AUTORESET, policy, 1, None, 0, 0, 0, 0, None, 0, None)
    d = rc.describe_rollout(env._dims, cfg, 0x1ff)
    assert d["name"] == name and d["blocks"] * (d["threads_per_block"] // 64) >= OCC_WAVES
    kw, ykw = {}, {}
    if policy == rref.GIVEN:
        actions = _given_actions(np.random.default_rng(S), OCC_STEPS, n)
        kw, ykw = dict(actions=torch.from_numpy(actions).to(env.device)), dict(actions=actions)
    elif policy == rref.TABLE:
        small = _env(S, mc, blk, init, tgt)
        tab = tref.table(oracle, S, mc, blk, tgt, T)
        rows = torch.from_numpy(level).to(env.device)
        kw, ykw = dict(table=small.build_table(), rows=rows, epsilon=0.25), dict(table=tab, rows=level, threshold=rref.threshold_of(0.25))
    want = rref.rollout(oracle, S, mc, OCC_MAX_STEPS, tile(blk), tile(init), tile(tgt), OCC_STEPS, policy, AUTORESET, seed=S, **ykw)
    assert want["timed_out"].any() and want["reset"].any()
    got = env.rollout(OCC_STEPS, ("given", "random", "table")[policy], seed=S, log=ALL_LOGS, **kw)
    _check(got, env, want, name)
    env.close()


# ---------------------------------------------------------------------------------------------- one run at scale
def test_a_quarter_of_a_million_boards_for_32_steps(torch_cuda, oracle):
    S, T, K, mc, n, max_steps, steps = 4, 2, 2, False, 262144, 20, 32
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    want = rref.rollout(oracle, S, mc, max_steps, blk, init, tgt, steps, rref.RANDOM, AUTORESET, seed=0x5CA1E)
    assert want["won"].mean() > 0.01 and want["timed_out"].any() and want["reset"].any()
    env = _env(S, mc, blk, init, tgt, max_steps, AUTORESET)
    got = env.rollout(steps, "random", seed=0x5CA1E, log=ALL_LOGS)
    _check(got, env, want, "scale")


# ---------------------------------------------------------------------------------------------- streams
def test_a_rollout_on_a_stream_of_its_own_ordered_after_a_step(torch_cuda, oracle):
    """2**18 boards, one extra stream, no host synchronisation until the end: the rollout is enqueued while the step still runs.
    A launch that ignored its `stream` argument would play from cells the step has not written yet."""
    torch = torch_cuda
    S, T, K, mc, n, max_steps, steps = 4, 2, 2, False, 1 << 18, 30, 12
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    act = oracle.fill_actions(n, seed=0x57EA, step_index=0)
    twin = oracle.OracleBatch(S, mc, max_steps, blk, init, tgt)
    twin.reset()
    twin.step(act, mode=AUTORESET, obs=False)
    want = rref.rollout(oracle, S, mc, max_steps, blk, init, tgt, steps, rref.RANDOM, AUTORESET, seed=8, pos=twin.pos,
                        step_count=twin.step_count, done=twin.done)
    from_start = rref.rollout(oracle, S, mc, max_steps, blk, init, tgt, steps, rref.RANDOM, AUTORESET, seed=8)
    assert (want["pos"] != from_start["pos"]).any(axis=0).sum() >= 1000      # the step matters
    env = _env(S, mc, blk, init, tgt, max_steps, AUTORESET)
    actions = torch.from_numpy(act).to(env.device)
    side = torch.cuda.Stream(device=env.device)
    assert side.cuda_stream != torch.cuda.current_stream(env.device).cuda_stream
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        env.step(actions)
        got = env.rollout(steps, "random", seed=8, log=ALL_LOGS)
    side.synchronize()
    _check(got, env, want, "stream")
