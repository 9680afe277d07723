"""ts_reach_solve on the GPU against the CPU yardstick (tests/reach_reference.py: breadth-first search over the oracle with sorted
keys) and, on shapes both take, against ts_solve itself.  Exact equality everywhere: moves, best and states are sizes of sets, the
same bits however the lanes race.  The raw C-ABI calls write into buffers between guard bytes, prefilled with the complement of the
yardstick's answer, and search in a workspace between guard bytes that is never zeroed."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAPACITY = 4096
# size, tiles, obstacles, multi colour, seeds 0 .. n-1: shapes ts_solve refuses, and what an exhaustive search of them reaches
BEYOND = ((5, 4, 3, True, 400), (5, 4, 3, False, 400), (8, 3, 10, False, 400), (7, 3, 8, False, 300))
# size, tiles, obstacles, multi colour, walk length, boards: levels whose targets are where a random walk left the tiles
WALKED = ((5, 4, 3, True, 12, 128), (5, 4, 3, False, 12, 128), (8, 3, 10, True, 12, 64), (7, 3, 8, True, 12, 64), (8, 4, 10, True, 10, 32),
          (8, 8, 12, True, 10, 16))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _oracle():
    from oracle import binding
    return binding


@functools.lru_cache(maxsize=None)
def _seeded(S, T, K, n):
    return _oracle().generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))


def _drawn(S, T, K, mc, n):
    """The first n levels of the occupancy case of size S (tests/reach_cases.py) where (T, K) is its shape, else the seeded ones."""
    import reach_cases as cases
    if (T, K) != cases.SHAPES[S][:2]:
        return _seeded(S, T, K, n)
    return tuple(np.ascontiguousarray(a[:, :n]) for a in cases.levels(_oracle(), S, mc))


@functools.lru_cache(maxsize=None)
def _walked(S, T, K, L, n):
    """(blk, init, tgt): the level of seed i with its targets moved to where L moves of ts_fill_actions' stream leave the tiles.
    In multi colour the same moves win it; fewer may."""
    orc = _oracle()
    blk, init, _ = _seeded(S, T, K, n)
    b = orc.OracleBatch(S, True, 2**30, blk, init, init)
    b.reset()
    for k in range(L):
        b.step(orc.fill_actions(n, seed=0x3A1C, step_index=k), obs=False)
    return blk, init, b.pos.copy()


@functools.lru_cache(maxsize=None)
def _yard_seeded(S, T, K, mc, n, max_depth=64, capacity=CAPACITY):
    import reach_reference as reach
    blk, init, tgt = _seeded(S, T, K, n)
    return reach.solve(_oracle(), S, mc, blk, tgt, init, max_depth, capacity)


@functools.lru_cache(maxsize=None)
def _yard_walked(S, T, K, mc, L, n, max_depth=64, capacity=CAPACITY):
    import reach_reference as reach
    blk, init, tgt = _walked(S, T, K, L, n)
    return reach.solve(_oracle(), S, mc, blk, tgt, init, max_depth, capacity)


def _env(S, mc, blk, init, tgt, pos=None, **kw):
    import torch
    from tiler_slider_amd import VecTilerSliderEnv
    env = VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=mc, obs_dtype=None, **kw)
    env.reset()
    if pos is not None:
        env._pos.copy_(torch.from_numpy(np.ascontiguousarray(pos)).to(env._pos.device))
    return env


def _raw(env, max_depth=64, capacity=CAPACITY, want=None, ask=(True, True), in_flight=None, stream=None):
    """ts_reach_solve through the C-ABI.  Outputs: buffers the test owns, each between guard bytes, prefilled with the bytewise
    complement of the yardstick's answer `want` = (moves, best, states) where the caller has it - an entry the kernel skips then
    differs by construction - else with 77.  `ask` = (best, states): an output not asked for is passed as NULL and its buffer must
    keep its fill.  Workspace: `in_flight` slices (default: as many as the library would use of 1 GiB) between guard bytes,
    prefilled with 0xA5 - the kernel clears what it uses and writes nothing outside it.  Returns (moves, best, states)."""
    import torch
    from table_harness import GUARD, guarded, payload
    from tiler_slider_amd import _reach_cabi as rc
    n = env.num_envs
    dts = (np.int16, np.uint8, np.int32)
    fills = [np.full(n, 77, dt) if want is None else ~np.asarray(want[i]).astype(dt) for i, dt in enumerate(dts)]
    bufs = [guarded(torch, env.device, f) for f in fills]
    per_board = rc.workspace_bytes(env._dims, capacity, 1)
    if in_flight is None:
        in_flight = rc.describe_reach(env._dims, max_depth, capacity)["boards_in_flight"]
    ws = torch.full((2 * GUARD + in_flight * per_board,), 0xA5, dtype=torch.uint8, device=env.device)
    assert (ws.data_ptr() + GUARD) % 8 == 0
    cfg = rc.ReachCfg(int(max_depth), int(capacity), ws.data_ptr() + GUARD, in_flight * per_board)
    d = rc.describe_reach(env._dims, max_depth, capacity, in_flight * per_board)
    assert d["blocks"] == d["boards_in_flight"] == min(n, in_flight, 1024) and d["name"] == f"k_reach<{env.size}>"
    ptr = lambda i: bufs[i].data_ptr() + GUARD
    out = rc.ReachOut(ptr(0), ptr(1) if ask[0] else None, ptr(2) if ask[1] else None)
    s = torch.cuda.current_stream(env.device) if stream is None else stream
    code = rc.lib().ts_reach_solve(C.byref(env._dims), C.byref(env._state), C.byref(cfg), C.byref(out), s.cuda_stream)
    assert code == 0, code
    s.synchronize()
    edge = ws.cpu().numpy()
    assert (edge[:GUARD] == 0xA5).all() and (edge[len(edge) - GUARD:] == 0xA5).all(), "a guard byte of the workspace was overwritten"
    got = [payload(b, dt, (n,)) for b, dt in zip(bufs, dts)]
    for i, asked in ((1, ask[0]), (2, ask[1])):
        if not asked:
            np.testing.assert_array_equal(got[i], fills[i], err_msg="an output that was not asked for was written")
            got[i] = None
    return tuple(got)


def _same(got, want, ctx):
    for name, g, w in zip(("moves", "best", "states"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{name}: {ctx}")


# ---------------------------------------------------------------------------------------------------- against ts_solve itself
@pytest.mark.parametrize("S,T,K,mc,n", ((4, 2, 2, False, 300), (3, 4, 1, False, 300), (4, 4, 2, True, 64), (4, 2, 2, True, 300),
                                         (3, 5, 1, False, 64), (3, 5, 1, True, 64)))
def test_equals_ts_solve_where_both_apply(torch_cuda, S, T, K, mc, n):
    """capacity = the index space: never FULL, so moves and best are ts_solve's, bit for bit, at full depth and cut short.  3x3 with
    five tiles is the one shape ts_solve takes whose keys split into two halves, by a division that is no shift."""
    from tiler_slider_amd import SOLVE_FULL
    blk, init, tgt = _drawn(S, T, K, mc, n)
    env = _env(S, mc, blk, init, tgt)
    for depth in (64, 5, 0):
        moves, bits = env.solve_bits(depth)
        got = _raw(env, depth, (S * S) ** T)
        _same(got[:2], (moves.cpu().numpy(), bits.cpu().numpy()), (S, T, mc, depth))
        assert (got[2] <= (S * S) ** T).all() and (got[0] != SOLVE_FULL).all()


def test_equals_ts_solve_on_the_smallest_boards(torch_cuda, oracle):
    """1x1 - the tile sits on its target, or there is none to sit on - and boards without tiles: one state each."""
    from tiler_slider_amd import SOLVE_NONE
    one = (np.zeros((1, 2), np.uint32), np.zeros((1, 2), np.uint8))
    for mc in (False, True):
        for tgt in (np.zeros((1, 2), np.uint8), np.zeros((0, 2), np.uint8)):
            env = _env(1, mc, one[0], one[1], tgt)
            moves, bits = env.solve_bits()
            got = _raw(env, 64, 1)
            _same(got[:2], (moves.cpu().numpy(), bits.cpu().numpy()), (1, mc, tgt.shape))
            assert got[2].tolist() == [0 if m == 0 else 1 for m in got[0]] and set(got[0].tolist()) <= {0, SOLVE_NONE}
    # no tiles: won where there is no target either, else never - one state, expanded once
    for S, level, lit in ((3, ([(1, 1)], [], []), 0), (3, ([(1, 1)], [], [(0, 0)]), SOLVE_NONE), (8, ([], [], []), 0),
                          (8, ([(7, 7)], [], [(3, 3), (3, 3)]), SOLVE_NONE)):
        blk, init, tgt = oracle.pack_levels(S, [level])
        for mc in (False, True):
            env = _env(S, mc, blk, init, tgt)
            moves, bits = env.solve_bits()
            got = _raw(env, 64, 1)
            _same(got[:2], (moves.cpu().numpy(), bits.cpu().numpy()), (S, mc, "no tiles"))
            assert got[0].tolist() == [lit] and got[2].tolist() == [0 if lit == 0 else 1]


# ---------------------------------------------------------------------------------------------------- beyond ts_solve
@pytest.mark.parametrize("S,T,K,mc,n", BEYOND)
def test_random_levels_beyond_the_index_space_of_ts_solve(torch_cuda, S, T, K, mc, n):
    """Almost all of these boards cannot be won: the whole reachable set is expanded, thousands of states a board."""
    import reach_reference as reach
    from tiler_slider_amd import VecTilerSliderEnv, _search_cabi
    want = _yard_seeded(S, T, K, mc, n)
    # properties of the YARDSTICK's answer: some boards can be won, none runs out of its budget
    assert (want[0] >= 1).sum() >= 2 and (want[0] == reach.SOLVE_FULL).sum() == 0 and (want[0] == reach.SOLVE_NONE).sum() >= n // 2
    env = VecTilerSliderEnv.from_seeds(np.arange(n), size=S, num_tiles=T, num_obstacles=K, multi_color=mc, obs_dtype=None)
    assert _search_cabi.solve_states(env._dims) == 0
    np.testing.assert_array_equal(env._init.cpu().numpy(), _seeded(S, T, K, n)[1])
    print(f"{S}x{S} T={T} K={K} mc={mc}: solvable {(want[0] >= 1).sum()} of {n}, deepest {want[0].max()}, most states {want[2].max()}, mean {want[2].mean():.0f}")
    _same(_raw(env, 64, CAPACITY, want), want, (S, T, K, mc))


@pytest.mark.parametrize("S,T,K,mc,L,n", WALKED)
def test_solvable_boards_with_long_keys(torch_cuda, S, T, K, mc, L, n):
    """Targets where a random walk left the tiles: every multi-colour board can be won, the optima are spread, and at 8x8 with 8
    tiles the keys run up to 2^48."""
    want = _yard_walked(S, T, K, mc, L, n)
    assert len(set(want[0][want[0] >= 1].tolist())) >= 3 and (not mc or (want[0] >= 0).all())
    every = [_yard_walked(*case) for case in WALKED]
    assert any(bin(b).count("1") >= 2 for w in every for b in w[1].tolist())   # two first moves of shortest solutions, somewhere
    blk, init, tgt = _walked(S, T, K, L, n)
    print(f"{S}x{S} T={T} K={K} mc={mc} walk {L}: optima {sorted(set(want[0].tolist()))}, most states {want[2].max()}")
    _same(_raw(_env(S, mc, blk, init, tgt), 64, CAPACITY, want), want, (S, T, K, mc, L))


@pytest.mark.parametrize("depth", (0, 3, 7))
def test_max_depth_on_the_walked_levels(torch_cuda, depth):
    """A shallower search: exactly the boards within reach keep their optimum and their best moves, the others that can be won
    report SOLVE_DEPTH."""
    import reach_reference as reach
    cut = 0
    for case in WALKED[:2] + WALKED[-1:]:
        S, T, K, mc, L, n = case
        full, want = _yard_walked(*case), _yard_walked(*case, max_depth=depth)
        can = full[0] >= 0
        np.testing.assert_array_equal(want[0][can], np.where(full[0][can] <= depth, full[0][can], reach.SOLVE_DEPTH))
        np.testing.assert_array_equal(want[1][can], np.where(full[0][can] <= depth, full[1][can], 0))
        cut += int((want[0] == reach.SOLVE_DEPTH).sum())
        blk, init, tgt = _walked(S, T, K, L, n)
        _same(_raw(_env(S, mc, blk, init, tgt), depth, CAPACITY, want), want, (case, depth))
    assert cut >= 3


def test_full_at_4x4_with_six_tiles(torch_cuda):
    """16.7 M placements, tens of thousands of them reached: at capacity 1,024 most boards run out of their budget."""
    import reach_reference as reach
    S, T, K, mc, n = 4, 6, 2, False, 32
    want = _yard_seeded(S, T, K, mc, n, 64, 1024)
    full = want[0] == reach.SOLVE_FULL
    assert full.sum() >= n // 2 and (~full).sum() >= 1 and (want[2][full] <= 1024).all()
    blk, init, tgt = _seeded(S, T, K, n)
    _same(_raw(_env(S, mc, blk, init, tgt), 64, 1024, want), want, "4x4 / 6 tiles at capacity 1024")


def test_the_edge_of_the_budget(torch_cuda):
    """Three boards of 5x5 / 4 tiles that cannot be won, R states reachable: capacity R ends in NONE with R states expanded,
    capacity R - 1 in FULL; capacities 1, 2 and 3 are tables of 2, 4 and 8 slots, where every probe sequence wraps around."""
    import reach_reference as reach
    S, T, K, mc, n = BEYOND[0]
    moves, _, states = _yard_seeded(S, T, K, mc, n)
    none = np.flatnonzero((moves == reach.SOLVE_NONE) & (states > 8))
    picks = none[np.argsort(states[none], kind="stable")[[0, len(none) // 2, -1]]]   # the smallest, the median and the largest reachable set
    blk, init, tgt = _seeded(S, T, K, n)
    for i in picks:
        R = int(states[i])
        one = lambda a: np.ascontiguousarray(a[:, i:i + 1])
        env = _env(S, mc, one(blk), one(init), one(tgt))
        for cap in (R, R - 1, 1, 2, 3):
            want = reach.solve(_oracle(), S, mc, one(blk), one(tgt), one(init), 64, cap)
            assert want[0].tolist() == [reach.SOLVE_NONE if cap == R else reach.SOLVE_FULL] and (cap != R or want[2].tolist() == [R])
            _same(_raw(env, 64, cap, want), want, (int(i), R, cap))


def test_slices_are_reused_when_the_workspace_is_smaller_than_the_batch(torch_cuda):
    """257 boards through a workspace for 3 boards, and for 1: each block clears its slice between boards, and the answers are
    those of the call that has a slice for every board."""
    S, T, K, mc, n = BEYOND[0]
    blk, init, tgt = (np.ascontiguousarray(a[:, :257]) for a in _seeded(S, T, K, n))
    want = tuple(a[:257] for a in _yard_seeded(S, T, K, mc, n))
    env = _env(S, mc, blk, init, tgt)
    for in_flight in (257, 3, 1):
        _same(_raw(env, 64, CAPACITY, want, in_flight=in_flight), want, f"{in_flight} boards in flight")


# ---------------------------------------------------------------------------------------------------- other cases
def test_targets_that_repeat_or_differ_in_number_and_cells_beyond_the_board(torch_cuda, oracle):
    """T != Tt (multi colour: never won; single colour: the sets of cells are compared), repeated targets, and cell ids >= S * S
    in tiles and targets, which read as S * S - 1: the oracle is handed the clamped level."""
    import reach_reference as reach
    S, T, K, n = 5, 4, 3, 48
    blk, init, tgt4 = _walked(S, T, K, 12, 128)
    blk, init, tgt4 = (np.ascontiguousarray(a[:, :n]) for a in (blk, init, tgt4))
    for mc in (False, True):
        # one target more (a repeat of the first), one fewer, and all four equal to the first
        for tgt in (np.concatenate([tgt4, tgt4[:1]]), tgt4[:3], np.repeat(tgt4[:1], 4, axis=0)):
            tgt = np.ascontiguousarray(tgt)
            want = reach.solve(oracle, S, mc, blk, tgt, init, 64, CAPACITY)
            _same(_raw(_env(S, mc, blk, init, tgt), 64, CAPACITY, want), want, (mc, tgt.shape))
        # ids beyond the board: every third board's last tile and every fourth board's last target
        free = ((blk[0] >> 24) & 1) == 0                       # cell 24 holds no obstacle ...
        raw_init, raw_tgt = init.copy(), tgt4.copy()
        on24 = (init[:3] == 24).any(axis=0)                    # ... and no other tile: two tiles on one cell is another test's matter
        edit = free & ~on24 & (np.arange(n) % 3 == 0)
        raw_init[3, edit] = 200
        raw_tgt[3, np.arange(n) % 4 == 0] = 255
        assert edit.sum() >= 3
        clamped = (np.minimum(raw_init, 24), np.minimum(raw_tgt, 24))
        want = reach.solve(oracle, S, mc, blk, clamped[1], clamped[0], 64, CAPACITY)
        env = _env(S, mc, blk, init, tgt4, pos=raw_init)   # reset() stores clamped cells: the ids beyond the board go in behind it
        env._tgt.copy_(torch_cuda.from_numpy(raw_tgt).to(env._tgt.device))
        _same(_raw(env, 64, CAPACITY, want), want, (mc, "ids beyond the board"))
        assert (want[0] >= 1).sum() >= 3


def test_mid_episode_twice_and_state_untouched(torch_cuda, oracle):
    """After 1, 2 and 5 random steps the boards are searched from where they stand; no byte of state changes; a second run gives
    the same bits."""
    import reach_reference as reach
    torch = torch_cuda
    S, T, K, mc, n = 5, 4, 3, True, 96
    blk, init, tgt = _walked(S, T, K, 12, 128)
    blk, init, tgt = (np.ascontiguousarray(a[:, :n]) for a in (blk, init, tgt))
    twin = oracle.OracleBatch(S, mc, 3, blk, init, tgt)
    env = _env(S, mc, blk, init, tgt, max_steps=3)
    twin.reset()
    for step in range(5):
        act = oracle.fill_actions(n, seed=0x501E, step_index=step)
        env.step(torch.from_numpy(act))
        twin.step(act, obs=False)
        if step + 1 in (1, 2, 5):
            np.testing.assert_array_equal(env.positions.cpu().numpy(), twin.pos)
            before = [t.clone() for t in (env._pos, env._step_count, env._done, env._init, env._tgt, env._blk)]
            want = reach.solve(oracle, S, mc, blk, tgt, twin.pos, 64, CAPACITY)
            first = _raw(env, 64, CAPACITY, want)
            _same(first, want, ("after steps", step + 1))
            _same(_raw(env, 64, CAPACITY), first, "the second run")
            for a, b in zip(before, (env._pos, env._step_count, env._done, env._init, env._tgt, env._blk)):
                assert torch.equal(a, b)


def test_outputs_that_are_not_asked_for_keep_their_fill(torch_cuda):
    case = WALKED[0]
    S, T, K, mc, L, n = case
    want = _yard_walked(*case)
    blk, init, tgt = _walked(S, T, K, L, n)
    env = _env(S, mc, blk, init, tgt)
    for ask in ((False, False), (True, False), (False, True)):
        got = _raw(env, 64, CAPACITY, want, ask=ask)
        np.testing.assert_array_equal(got[0], want[0])
        assert (got[1] is None) == (not ask[0]) and (got[2] is None) == (not ask[1])
        for i in (1, 2):
            if got[i] is not None:
                np.testing.assert_array_equal(got[i], want[i])


def test_on_a_stream_of_its_own_behind_a_step(torch_cuda, oracle):
    """The call is asynchronous on ITS stream: launched on a side stream that waits for the step, it searches the boards the
    step left."""
    import reach_reference as reach
    torch = torch_cuda
    case = WALKED[0]
    S, T, K, mc, L, n = case
    blk, init, tgt = _walked(S, T, K, L, n)
    env = _env(S, mc, blk, init, tgt)
    twin = oracle.OracleBatch(S, mc, 100, blk, init, tgt)
    twin.reset()
    act = oracle.fill_actions(n, seed=0x57EA, step_index=0)
    twin.step(act, obs=False)
    want = reach.solve(oracle, S, mc, blk, tgt, twin.pos, 64, CAPACITY)
    side = torch.cuda.Stream(env.device)
    env.step(torch.from_numpy(act))
    side.wait_stream(torch.cuda.current_stream(env.device))
    _same(_raw(env, 64, CAPACITY, want, stream=side), want, "on a side stream")


def test_solve_reachable_and_expert(torch_cuda):
    """The method against the raw call: dtypes, shapes, best as columns of bits, expert as the lowest bit - and a board stepped by
    its expert moves is won in exactly moves steps."""
    torch = torch_cuda
    from tiler_slider_amd import SOLVE_FULL, ReachResult
    case = WALKED[0]
    S, T, K, mc, L, n = case
    want = _yard_walked(*case)
    blk, init, tgt = _walked(S, T, K, L, n)
    env = _env(S, mc, blk, init, tgt, max_steps=1000)
    res = env.solve_reachable()
    assert isinstance(res, ReachResult) and (res.moves.dtype, res.bits.dtype, res.states.dtype, res.best.dtype, res.expert.dtype) == (
        torch.int16, torch.uint8, torch.int32, torch.bool, torch.uint8)
    assert tuple(res.best.shape) == (n, 4) and tuple(res.expert.shape) == (n,)
    _same((res.moves.cpu().numpy(), res.bits.cpu().numpy(), res.states.cpu().numpy()), want, "solve_reachable()")
    np.testing.assert_array_equal(res.best.cpu().numpy(), (want[1][:, None] >> np.arange(4)) & 1 != 0)
    lowest = np.array([255 if b == 0 else (int(b) & -int(b)).bit_length() - 1 for b in want[1]], np.uint8)
    np.testing.assert_array_equal(res.expert.cpu().numpy(), lowest)
    bare = env.solve_reachable(with_best=False)
    assert bare.bits is None and bare.best is None and torch.equal(bare.moves, res.moves) and torch.equal(bare.states, res.states)
    small = env.solve_reachable(workspace_bytes=3 * 120 * 1024)   # three slices of 112 KiB: the boards queue up behind them
    assert torch.equal(small.moves, res.moves) and torch.equal(small.bits, res.bits) and torch.equal(small.states, res.states)
    tight = env.solve_reachable(capacity=2)
    assert bool(((tight.moves == SOLVE_FULL) | (tight.moves == res.moves)).all()) and bool((tight.moves == SOLVE_FULL).any())
    left = res.moves.clone()
    for step in range(int(res.moves.max())):
        now = env.solve_reachable()
        assert torch.equal(now.moves, left)
        env.step(now.expert)
        left = torch.where(left >= 1, left - 1, left)
    assert bool(env.is_won()[res.moves >= 0].all())
    for kw in ({"max_depth": -1}, {"max_depth": 40000}, {"capacity": 0}, {"capacity": (1 << 30) + 1}, {"workspace_bytes": 1000}):
        with pytest.raises(ValueError, match=next(iter(kw)).split("_")[0]):
            env.solve_reachable(**kw)


def test_shapes_beyond_the_hashed_solver_raise_and_solve_still_refuses(torch_cuda):
    from tiler_slider_amd import VecTilerSliderEnv
    for S, T in ((9, 1), (8, 9), (6, 9)):
        env = VecTilerSliderEnv.random(4, size=S, num_tiles=T, num_obstacles=2, obs_dtype=None)
        with pytest.raises(ValueError, match="8x8 with up to 8 tiles"):
            env.solve_reachable()
    env = VecTilerSliderEnv.random(4, size=5, num_tiles=4, num_obstacles=3, obs_dtype=None)
    with pytest.raises(ValueError, match="65536"):
        env.solve()
    assert env.solve_reachable().moves.shape[0] == 4


def test_solvable_seeds_beyond_the_index_space_of_ts_solve(torch_cuda):
    """The scan of the yardstick: the first three seeds whose 5x5 level of four tiles can be won in multi colour, for two batch
    sizes; with a smaller budget one of them is FULL and is not found, again whatever the batch size."""
    import reach_reference as reach
    from tiler_slider_amd import TilerSliderEnvFactory
    S, T, K, mc, n = BEYOND[0]
    moves = _yard_seeded(S, T, K, mc, n)[0]
    want = np.flatnonzero(moves >= 1)[:3].astype(np.uint32)
    assert len(want) == 3
    for batch in (100, 400):
        got = TilerSliderEnvFactory.solvable_seeds(3, S, T, K, multi_color=True, batch_size=batch)
        assert got.dtype == np.uint32
        np.testing.assert_array_equal(got, want)
    deep = np.flatnonzero(moves >= 4)[:1].astype(np.uint32)
    np.testing.assert_array_equal(TilerSliderEnvFactory.solvable_seeds(1, S, T, K, multi_color=True, min_moves=4, batch_size=64), deep)
    # at capacity 256 the third of them - 981 states expanded before its win - is FULL, and FULL is not found
    tight = _yard_seeded(S, T, K, mc, n, 32767, 256)[0]
    assert tight[want[2]] == reach.SOLVE_FULL and (tight[want[:2]] >= 1).all() and (tight >= 1).sum() == 2
    for batch in (150, 400):
        np.testing.assert_array_equal(TilerSliderEnvFactory.solvable_seeds(2, S, T, K, multi_color=True, batch_size=batch, capacity=256), want[:2])
