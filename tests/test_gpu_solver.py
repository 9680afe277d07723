"""ts_solve on the GPU against the CPU yardstick (tests/solver_reference.py: breadth-first search over the oracle), exact equality
everywhere: optimal move counts, SOLVE_NONE / SOLVE_DEPTH, and the mask of first moves of all shortest solutions."""
import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

# size, tiles, obstacles, multi colour, seeds 0 .. n-1: the rows of DESIGN.md section 11 (how many random levels can be solved)
ROWS = ((4, 2, 2, False, 2000), (4, 2, 2, True, 2000), (5, 2, 3, False, 1000), (5, 3, 3, True, 500), (6, 3, 6, False, 300),
        (8, 2, 10, True, 300), (3, 4, 1, False, 300), (4, 4, 2, True, 200))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _env(S, mc, blk, init, tgt, pos=None, **kw):
    import torch
    from tiler_slider_amd import VecTilerSliderEnv
    env = VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=mc, obs_dtype=None, **kw)
    env.reset()
    if pos is not None:
        env._pos.copy_(torch.from_numpy(np.ascontiguousarray(pos)).to(env._pos.device))
    return env


def _solve_raw(env, max_depth, want=None):
    """ts_solve through the C-ABI into buffers the test owns, each between guard bytes: prefilled with the bytewise complement of
    the yardstick's answer `want` = (moves, best) where the caller has it - an entry the kernel skips then differs by construction
    -, else with 77 (no answer of the library: moves 19789, best 77).  env.solve_bits() writes into torch.empty, which hands
    back the block of the previous, equal call."""
    import ctypes as C
    import torch
    from table_harness import GUARD, guarded as _guarded, payload as _payload
    from tiler_slider_amd import _search_cabi as sc
    n = env.num_envs
    fill = lambda i, dt: np.full(n, 77, dt) if want is None else ~np.asarray(want[i]).astype(dt)
    mbuf, bbuf = _guarded(torch, env.device, fill(0, np.int16)), _guarded(torch, env.device, fill(1, np.uint8))
    rc = sc.lib().ts_solve(C.byref(env._dims), C.byref(env._state), int(max_depth), mbuf.data_ptr() + GUARD, bbuf.data_ptr() + GUARD,
                           torch.cuda.current_stream(env.device).cuda_stream)
    assert rc == 0, rc
    return _payload(mbuf, np.int16, (n,)), _payload(bbuf, np.uint8, (n,))


def _gpu(S, mc, blk, init, tgt, pos=None, max_depth=64, want=None):
    """(moves int16 [N], best uint8 [N]) of ts_solve, and solve()'s bool [N, 4] checked against the bits on the way.  `want`: the
    yardstick's answer where the caller has it beforehand (_solve_raw)."""
    env = _env(S, mc, blk, init, tgt, pos)
    raw = _solve_raw(env, max_depth, want)
    if want is not None:
        _same(raw, want, "into the complement of the yardstick's answer")
    moves, bits = env.solve_bits(max_depth)
    _same(raw, (moves.cpu().numpy(), bits.cpu().numpy()), "the raw call and solve_bits()")
    moves2, best4 = env.solve(max_depth)
    moves, bits = moves.cpu().numpy(), bits.cpu().numpy()
    assert moves.dtype == np.int16 and bits.dtype == np.uint8 and str(best4.dtype) == 'torch.bool' and tuple(best4.shape) == (len(moves), 4)
    np.testing.assert_array_equal(moves2.cpu().numpy(), moves)
    np.testing.assert_array_equal(best4.cpu().numpy(), (bits[:, None] >> np.arange(4)) & 1 != 0)
    only_moves, none = env.solve(max_depth, with_best=False)   # best = NULL in the C-ABI
    assert none is None
    np.testing.assert_array_equal(only_moves.cpu().numpy(), moves)
    return moves, bits


def _same(got, want, ctx):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"moves {ctx}")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"best {ctx}")


def test_screenshot_levels(torch_cuda, oracle):
    """The 400 levels the game ships: moves == the optimum recorded in the fixture, best == the yardstick's; and with a
    shallower max_depth exactly the boards beyond it report SOLVE_DEPTH."""
    import solver_reference as ref
    from tiler_slider_amd.levels import pack_levels
    total = 0
    for (S, T, mc), (ids, blk, init, tgt, want) in ref.fixture_groups(GOLDEN_DIR, pack_levels).items():
        yard = ref.solve(oracle, S, mc, blk, tgt, init)
        moves, best = _gpu(S, mc, blk, init, tgt, want=yard)
        np.testing.assert_array_equal(moves, want, err_msg=str((S, T, mc)))
        _same((moves, best), yard, (S, T, mc))
        assert 1 <= moves.min() and moves.max() <= 15
        for depth in (0, 3, 7):
            m, b = _gpu(S, mc, blk, init, tgt, max_depth=depth, want=(np.where(want <= depth, want, ref.SOLVE_DEPTH), np.where(want <= depth, yard[1], 0)))
            np.testing.assert_array_equal(m, np.where(want <= depth, want, ref.SOLVE_DEPTH))
            np.testing.assert_array_equal(b, np.where(want <= depth, best, 0))
        total += len(ids)
    assert total == 400


@pytest.mark.parametrize("S,T,K,mc,n", ROWS)
def test_random_levels_from_seeds(torch_cuda, oracle, S, T, K, mc, n):
    import solver_reference as ref
    from tiler_slider_amd import VecTilerSliderEnv
    seeds = np.arange(n, dtype=np.uint32)
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, seeds)
    want = ref.solve(oracle, S, mc, blk, tgt, init)
    # no row tests one outcome only - a property of the YARDSTICK's answer
    assert (want[0] >= 1).sum() >= 3 and (want[0] == ref.SOLVE_NONE).sum() >= 3, ((want[0] >= 1).sum(), (want[0] == ref.SOLVE_NONE).sum())
    env = VecTilerSliderEnv.from_seeds(seeds, size=S, num_tiles=T, num_obstacles=K, multi_color=mc, obs_dtype=None)
    np.testing.assert_array_equal(env._init.cpu().numpy(), init)
    _same(_solve_raw(env, 64, want), want, (S, T, K, mc, "into the complement of the yardstick's answer"))
    moves, bits = env.solve_bits()
    print(f"{S}x{S} T={T} K={K} mc={mc}: solvable {(want[0] >= 1).sum()} of {n}, deepest {want[0].max()}")
    _same((moves.cpu().numpy(), bits.cpu().numpy()), want, (S, T, K, mc))


def _pack(oracle, S, levels):
    return oracle.pack_levels(S, levels)


def test_hand_made_boards(torch_cuda, oracle):
    import solver_reference as ref
    NONE, DEPTH = ref.SOLVE_NONE, ref.SOLVE_DEPTH
    U, D, L, R = 1, 2, 4, 8
    # (S, multi colour, [(blocked, tiles, targets)], literal moves, literal best)
    cases = [
        # already won; one move; a tile walled into its corner (its target elsewhere); the reachable set exhausted
        (4, True, [([], [(0, 0), (3, 3)], [(0, 0), (3, 3)]), ([(2, 1)], [(0, 1), (0, 2)], [(1, 1), (3, 2)]),
                   ([(0, 1), (1, 0)], [(0, 0), (2, 2)], [(3, 0), (2, 2)]), ([], [(0, 0), (0, 1)], [(1, 1), (2, 2)])], [0, 1, NONE, NONE], [0, D, 0, 0]),
        # the same boards in single colour: the SETS of cells are compared
        (4, False, [([], [(0, 0), (3, 3)], [(3, 3), (0, 0)]), ([(2, 1)], [(0, 1), (0, 2)], [(3, 2), (1, 1)]),
                    ([(0, 1), (1, 0)], [(0, 0), (2, 2)], [(3, 0), (2, 2)]), ([], [(0, 0), (0, 1)], [(1, 1), (2, 2)])], [0, 1, NONE, NONE], [0, D, 0, 0]),
        # one tile on 8x8 without obstacles: a corner takes two moves in either order, an edge cell of its row one, an inner cell is never reached
        (8, False, [([], [(3, 3)], [(0, 0)]), ([], [(3, 3)], [(3, 0)]), ([], [(3, 3)], [(4, 4)]), ([], [(3, 3)], [(7, 7)]), ([], [(3, 3)], [(0, 5)])],
         [2, 1, NONE, 2, NONE], [U | L, L, 0, D | R, 0]),
        (8, True, [([], [(3, 3)], [(0, 0)]), ([], [(3, 3)], [(3, 0)]), ([], [(3, 3)], [(4, 4)]), ([], [(3, 3)], [(7, 7)]), ([], [(3, 3)], [(0, 5)])],
         [2, 1, NONE, 2, NONE], [U | L, L, 0, D | R, 0]),
        # repeated targets with n_tiles != n_targets: one tile, the same target twice - single colour compares sets (solvable),
        # multi colour needs n_tiles == n_targets (never won)
        (5, False, [([], [(2, 2)], [(2, 0), (2, 0)]), ([], [(2, 0)], [(2, 0), (2, 0)])], [1, 0], [L, 0]),
        (5, True, [([], [(2, 2)], [(2, 0), (2, 0)]), ([], [(2, 0)], [(2, 0), (2, 0)])], [NONE, NONE], [0, 0]),
        # repeated targets with n_tiles == n_targets: two distinct tiles never cover one cell, in either colour mode
        (4, False, [([], [(0, 0), (1, 1)], [(3, 3), (3, 3)])], [NONE], [0]),
        (4, True, [([], [(0, 0), (1, 1)], [(3, 3), (3, 3)])], [NONE], [0]),
        # more tiles than targets, single colour: never; no targets at all and no tiles: won as it stands
        (4, False, [([], [(0, 0), (1, 1)], [(3, 3)])], [NONE], [0]),
        (3, False, [([(1, 1)], [], [])], [0], [0]),
        (3, True, [([(1, 1)], [], [])], [0], [0]),
        (3, False, [([(1, 1)], [], [(0, 0)])], [NONE], [0]),
    ]
    for S, mc, levels, lit_moves, lit_best in cases:
        blk, init, tgt = _pack(oracle, S, levels)
        want = ref.solve(oracle, S, mc, blk, tgt, init)
        assert want[0].tolist() == lit_moves and want[1].tolist() == lit_best, (S, mc, want)   # the yardstick against the literals
        _same(_gpu(S, mc, blk, init, tgt, want=want), want, (S, mc, levels))
        # max_depth = d - 1 stops short of a board of optimum d, max_depth = d finds it; a board whose reachable set is exhausted at
        # a depth <= max_depth reports SOLVE_NONE, before that SOLVE_DEPTH
        for depth in (0, 1, 2):
            shallow = ref.solve(oracle, S, mc, blk, tgt, init, max_depth=depth)
            got = _gpu(S, mc, blk, init, tgt, max_depth=depth, want=shallow)
            _same(got, shallow, (S, mc, depth))
            for n, d in enumerate(lit_moves):
                if d >= 0:
                    assert got[0][n] == (d if d <= depth else DEPTH)
            if depth == 0:
                assert all(g == DEPTH for g, d in zip(got[0], lit_moves) if d != 0)
    # the walled-in tile: nothing is reachable, so depth 1 already exhausts the set
    blk, init, tgt = _pack(oracle, 4, [([(0, 1), (1, 0), (3, 2), (2, 3)], [(0, 0), (3, 3)], [(3, 3), (1, 1)])])
    lit = lambda m: (np.array([m], np.int16), np.array([0], np.uint8))   # best is 0 wherever moves < 1
    assert _gpu(4, True, blk, init, tgt, max_depth=1, want=lit(NONE))[0].tolist() == [NONE]
    assert _gpu(4, True, blk, init, tgt, max_depth=0, want=lit(DEPTH))[0].tolist() == [DEPTH]
    assert _gpu(4, True, blk, init, tgt, max_depth=32767, want=lit(NONE))[0].tolist() == [NONE]


def test_mid_episode_and_state_untouched(torch_cuda, oracle):
    """After 1, 2 and 5 random steps (max_steps = 3: some boards won, some timed out, all of them still searched from where they
    stand): solve() == the yardstick from the oracle's current cells, and not a byte of state changes."""
    import solver_reference as ref
    torch = torch_cuda
    for S, T, K, mc, n in ((4, 2, 2, False, 1500), (5, 3, 3, True, 300)):
        blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
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
                moves, bits = env.solve_bits()
                for a, b in zip(before, (env._pos, env._step_count, env._done, env._init, env._tgt, env._blk)):
                    assert torch.equal(a, b)
                _same((moves.cpu().numpy(), bits.cpu().numpy()), ref.solve(oracle, S, mc, blk, tgt, twin.pos), (S, T, mc, step + 1))
        assert twin.done.any() and (twin.step_count >= 3).any()


def test_following_the_expert(torch_cuda, oracle):
    """Stepping with expert_actions() wins every solvable board in exactly moves[n] steps, the optimum falling by one per step;
    unsolvable boards stay unsolvable whatever is played."""
    torch = torch_cuda
    from tiler_slider_amd import SOLVE_NONE, VecTilerSliderEnv
    for S, T, K, mc, n in ((4, 2, 2, False, 2000), (4, 2, 2, True, 2000), (5, 3, 3, True, 500)):
        env = VecTilerSliderEnv.from_seeds(np.arange(n), size=S, num_tiles=T, num_obstacles=K, multi_color=mc, obs_dtype=None, max_steps=1000)
        env.reset()
        moves0, _ = env.solve()
        solvable = moves0 >= 1
        assert int(solvable.sum()) >= 3
        won_at = torch.full((n,), -1, dtype=torch.int32, device=moves0.device)
        left = moves0.clone()
        for step in range(1, int(moves0.max()) + 1):
            act = env.expert_actions()
            assert torch.equal(act != 255, left >= 1)
            _, _, info = env.step(act)
            assert torch.equal(info["bad_action"] | info["stepped_done"], left < 1)   # untouched: nothing to play, or already won
            now, _ = env.solve()
            assert torch.equal(now[left >= 1], left[left >= 1] - 1)
            assert torch.equal(now[left < 1], left[left < 1])
            won_at[(left == 1) & info["is_won"]] = step
            left = now
        assert torch.equal(won_at[solvable], moves0[solvable].to(torch.int32)) and bool((won_at[~solvable] == -1).all())
        assert bool(env.is_won()[solvable].all())
        # boards without a solution: ten random steps, still none
        stuck = VecTilerSliderEnv.from_seeds(np.arange(n), size=S, num_tiles=T, num_obstacles=K, multi_color=mc, obs_dtype=None, max_steps=1000)
        stuck.reset()
        none0 = moves0 == SOLVE_NONE
        assert int(none0.sum()) >= 3
        for step in range(10):
            stuck.step(torch.from_numpy(oracle.fill_actions(n, seed=0xE9, step_index=step)))
            assert bool((stuck.solve()[0][none0] == SOLVE_NONE).all())


def _form_cases():
    # kernel name -> (S, T, obstacles): a shape that launches it under the library's policy
    cases = {f"k_solve_wave<{S}>": (S, T, K) for S, T, K in ((2, 1, 1), (3, 2, 1), (4, 2, 2), (5, 2, 3), (6, 2, 6), (7, 2, 8), (8, 2, 10))}
    cases.update({f"k_solve_block<{S}>": (S, T, K) for S, T, K in ((3, 5, 0), (4, 4, 2), (5, 3, 3), (6, 3, 6))})
    cases["k_solve_wave<1>"] = (1, 1, 0)
    return cases


@pytest.mark.parametrize("name", sorted(_form_cases()))
def test_every_compiled_form_at_occupancy(torch_cuda, oracle, name):
    """Every kernel of the search library (tests/test_solver_cpu.py pins this list to the code object), a few hundred levels tiled
    to at least 4,096 waves - two waves per SIMD and more, as tests/test_kernel_instantiations.py runs the step kernels: every
    copy of a level gets the yardstick's answer for it."""
    import solver_reference as ref
    from tiler_slider_amd import _cabi, _search_cabi
    S, T, K = _form_cases()[name]
    distinct = 256
    for mc in (False, True):
        if S == 1:   # one cell: the tile sits on its target (won), or there is no target to sit on (single colour: never won)
            blk, init = np.zeros((1, distinct), np.uint32), np.zeros((1, distinct), np.uint8)
            tgt = np.zeros((1 if mc else 0, distinct), np.uint8)
        elif 2 * T + K > S * S:   # 3x3 with five tiles: the targets are drawn on their own and may lie under tiles
            blk, init, _ = oracle.generate(S, T, 0, 1, distinct, seed=0x50F7)
            _, _, tgt = oracle.generate(S, 0, T, 0, distinct, seed=0x50F8)
        else:
            blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(1000, 1000 + distinct, dtype=np.uint32))
        want = ref.solve(oracle, S, mc, blk, tgt, init)
        print(f"{name} mc={mc}: {(want[0] >= 1).sum()} solvable, {(want[0] == ref.SOLVE_NONE).sum()} without a solution, deepest {want[0].max()}")
        d = _search_cabi.describe_solve(_cabi.Dims(distinct, S, T, tgt.shape[0], int(mc), 100, 0))
        assert d["name"] == name
        waves_per_block = d["threads_per_block"] // 64
        copies = -(-4096 * d["boards_per_block"] // (waves_per_block * distinct)) + 1
        n = copies * distinct - 3   # a ragged last block
        tile = lambda a: np.ascontiguousarray(np.tile(a, (1, copies))[:, :n])
        env = _env(S, mc, tile(blk), tile(init), tile(tgt))
        assert _search_cabi.describe_solve(env._dims)["blocks"] * waves_per_block >= 4096
        tiled = (np.tile(want[0], copies)[:n], np.tile(want[1], copies)[:n])
        _same(_solve_raw(env, 64, tiled), tiled, (name, mc, "into the complement of the yardstick's answer"))
        moves, bits = env.solve_bits()
        _same((moves.cpu().numpy(), bits.cpu().numpy()), tiled, (name, mc))


def test_both_forms_agree_where_both_exist(torch_cuda, oracle):
    """ts_search_tuning moves the boundary: cfg1's shape through the block form, a 4x4 board of four tiles through the wave form
    (one board per wave, 56 KiB of LDS), two bitmap words per lane - the answers do not change."""
    import solver_reference as ref
    from tiler_slider_amd import _search_cabi as sc
    L = sc.lib()
    try:
        for (S, T, K, mc, n), states, wpl in (((4, 2, 2, False, 700), 0, 1), ((4, 4, 2, True, 200), 65536, 1), ((5, 2, 3, False, 700), 8192, 2),
                                              ((8, 2, 10, True, 300), 8192, 4), ((3, 4, 1, False, 300), 0, 1)):
            blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
            want = ref.solve(oracle, S, mc, blk, tgt, init)
            L.ts_search_tuning(sc.TUNE_WAVE_MAX_STATES, states)
            L.ts_search_tuning(sc.TUNE_WORDS_PER_LANE, wpl)
            _same(_gpu(S, mc, blk, init, tgt, want=want), want, (S, T, states, wpl))
    finally:
        L.ts_search_tuning(sc.TUNE_WAVE_MAX_STATES, 8192)
        L.ts_search_tuning(sc.TUNE_WORDS_PER_LANE, 1)


def test_solvable_seeds(torch_cuda, oracle):
    import solver_reference as ref
    from tiler_slider_amd import TilerSliderEnvFactory, VecTilerSliderEnv

    def yardstick(count, S, T, K, scan, lo=1, hi=None):
        blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(scan, dtype=np.uint32))
        m = ref.optimum(oracle, S, False, blk, tgt, init, max_depth=32767)
        ok = np.flatnonzero((m >= lo) & ((m <= hi) if hi is not None else True))
        assert len(ok) >= count
        return ok[:count].astype(np.uint32), m

    want, m = yardstick(50, 4, 2, 2, 300)
    assert want[-1] == 245
    for batch in (64, 1000, None):
        kw = {} if batch is None else {"batch_size": batch}
        got = TilerSliderEnvFactory.solvable_seeds(50, size=4, num_tiles=2, num_obstacles=2, **kw)
        assert got.dtype == np.uint32
        np.testing.assert_array_equal(got, want)
    want5, m5 = yardstick(20, 5, 2, 3, 600, lo=4)
    assert want5[-1] == 523
    for batch in (100, 7):
        np.testing.assert_array_equal(TilerSliderEnvFactory.solvable_seeds(20, 5, 2, 3, min_moves=4, batch_size=batch), want5)
    # a window of optima, a later start, and the result feeding from_seeds unchanged
    win, _ = yardstick(10, 4, 2, 2, 600, lo=3, hi=5)
    np.testing.assert_array_equal(TilerSliderEnvFactory.solvable_seeds(10, 4, 2, 2, min_moves=3, max_moves=5, batch_size=50), win)
    later = TilerSliderEnvFactory.solvable_seeds(5, 4, 2, 2, start_seed=100, batch_size=33)
    np.testing.assert_array_equal(later, np.flatnonzero(m >= 1)[np.flatnonzero(m >= 1) >= 100][:5])
    env = TilerSliderEnvFactory.create_vec_env_from_seeds(want, size=4, num_tiles=2, num_obstacles=2)
    assert bool((env.solve()[0] >= 1).all())
    assert len(TilerSliderEnvFactory.solvable_seeds(0)) == 0


def test_unsupported_shapes_raise(torch_cuda, oracle):
    from tiler_slider_amd import VecTilerSliderEnv
    for S, T in ((5, 4), (9, 1)):
        env = VecTilerSliderEnv.random(16, size=S, num_tiles=T, num_obstacles=2, obs_dtype=None)
        with pytest.raises(ValueError, match="65536"):
            env.solve()
    env = VecTilerSliderEnv.random(16, size=4, num_tiles=2, num_obstacles=2, obs_dtype=None)
    with pytest.raises(ValueError, match="max_depth"):
        env.solve(max_depth=-1)
    with pytest.raises(ValueError, match="max_depth"):
        env.solve(max_depth=40000)
