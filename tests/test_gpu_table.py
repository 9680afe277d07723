"""ts_table_build and ts_table_lookup on the GPU, exact equality everywhere: whole tables byte for byte against the CPU yardstick
(tests/table_reference.py: backward relaxation over the oracle's successors), lookups against the merged solver (ts_solve)."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

# size, tiles, obstacles, multi colour, seeds 0 .. n-1: the shapes of test_gpu_solver.ROWS; the seed counts of the large index
# spaces are cut so that the yardstick (an int32 and a few index arrays per placement) stays small
ROWS = ((4, 2, 2, False, 2000), (4, 2, 2, True, 2000), (5, 2, 3, False, 1000), (5, 3, 3, True, 200), (6, 3, 6, False, 60),
        (8, 2, 10, True, 300), (3, 4, 1, False, 300), (4, 4, 2, True, 40))
SOLVE_MAX_DEPTH = 32767


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _env(S, mc, blk, init, tgt, **kw):
    from tiler_slider_amd import VecTilerSliderEnv
    env = VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=mc, obs_dtype=None, **kw)
    env.reset()
    return env


class _forms:
    """The launch forms a shape can be built in: the library's own, each of the two forced where both are compiled (boards 2x2 ..
    8x8), and the wave form with 32 placements per lane (several boards per wave).  Restores the knobs."""

    def __init__(self, S):
        from tiler_slider_amd import _table_cabi as tc
        self.tc, self.L, self.S = tc, tc.lib(), S

    def __enter__(self):
        tc, L = self.tc, self.L
        self.saved = tuple(L.ts_table_tuning(k, -1) for k in (tc.TUNE_WAVE_MAX_STATES, tc.TUNE_STATES_PER_LANE, tc.TUNE_BLOCK_BELOW_BOARDS))
        return self

    def __iter__(self):
        tc, L = self.tc, self.L
        yield "library policy"
        L.ts_table_tuning(tc.TUNE_BLOCK_BELOW_BOARDS, 0)
        L.ts_table_tuning(tc.TUNE_WAVE_MAX_STATES, 65536)
        yield "wave form"
        L.ts_table_tuning(tc.TUNE_STATES_PER_LANE, 32)
        yield "wave form, 32 placements per lane"
        L.ts_table_tuning(tc.TUNE_STATES_PER_LANE, self.saved[1])
        if self.S >= 2:
            L.ts_table_tuning(tc.TUNE_WAVE_MAX_STATES, 0)
            yield "block form"

    def __exit__(self, *exc):
        for k, v in zip((self.tc.TUNE_WAVE_MAX_STATES, self.tc.TUNE_STATES_PER_LANE, self.tc.TUNE_BLOCK_BELOW_BOARDS), self.saved):
            self.L.ts_table_tuning(k, v)


def _check_tables(env, S, dist, ctx):
    """Every form, max_depth = 252 (the default), 0, 3 and 7: the whole table equals the yardstick's."""
    import table_reference as tref
    from tiler_slider_amd import _table_cabi as tc
    full = tref.cut(dist)
    seen = set()
    with _forms(S) as forms:
        for form in forms:
            d = tc.describe_table_build(env._dims)
            seen.add(d["name"])
            assert d["name"] == (f"k_table_block<{S}>" if form == "block form" else f"k_table_wave<{S}>") or form == "library policy"
            table = env.build_table()
            assert str(table.dist.dtype) == "torch.uint8" and tuple(table.dist.shape) == full.shape
            np.testing.assert_array_equal(table.dist.cpu().numpy(), full, err_msg=f"{ctx} {form}")
            assert table.complete.cpu().numpy().tolist() == (~(full == tref.DEEP).any(axis=1)).tolist()
            for depth in (0, 3, 7):
                want = tref.cut(dist, depth)
                # the yardstick's own answer, spelled out: entries within the depth are the full table's; the rest of a board is
                # DEEP exactly where R(depth) is not empty, NONE otherwise
                within = (full <= depth) | (full == tref.INVALID)
                deep_board = (dist == depth).any(axis=1)
                np.testing.assert_array_equal(want[within], full[within])
                np.testing.assert_array_equal(want[~within], np.broadcast_to(np.where(deep_board[:, None], tref.DEEP, tref.NONE), full.shape)[~within])
                shallow = env.build_table(max_depth=depth)
                np.testing.assert_array_equal(shallow.dist.cpu().numpy(), want, err_msg=f"{ctx} {form} depth {depth}")
                assert shallow.complete.cpu().numpy().tolist() == (~(want == tref.DEEP).any(axis=1)).tolist()
    assert f"k_table_wave<{S}>" in seen and (S < 2 or f"k_table_block<{S}>" in seen)
    return full


def test_tables_of_the_screenshot_levels(torch_cuda, oracle):
    """The 400 levels the game ships, every shape group, every launch form: byte for byte; the entry where a level starts is the
    optimum recorded in the fixture."""
    import solver_reference as ref
    import table_reference as tref
    from tiler_slider_amd.levels import pack_levels
    total = 0
    for (S, T, mc), (ids, blk, init, tgt, want) in ref.fixture_groups(GOLDEN_DIR, pack_levels).items():
        dist = tref.exact(oracle, S, mc, blk, tgt, T)
        full = _check_tables(_env(S, mc, blk, init, tgt), S, dist, (S, T, mc))
        np.testing.assert_array_equal(full[np.arange(len(ids)), tref.index_of(S, init)], want)
        print(f"{S}x{S} T={T} mc={mc}: {len(ids)} levels, deepest entry {full[full <= tref.MAX_DEPTH].max()}")
        total += len(ids)
    assert total == 400


@pytest.mark.parametrize("S,T,K,mc,n", ROWS)
def test_tables_of_random_levels_from_seeds(torch_cuda, oracle, S, T, K, mc, n):
    import table_reference as tref
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    dist = tref.exact(oracle, S, mc, blk, tgt, T)
    full = tref.cut(dist)
    # no row tests one outcome only - a property of the YARDSTICK's answer
    counts = (((full >= 1) & (full <= tref.MAX_DEPTH)).sum(), (full == tref.NONE).sum(), (full == tref.INVALID).sum(), (full == 0).sum())
    assert min(counts) >= 3, counts
    print(f"{S}x{S} T={T} K={K} mc={mc}: entries at distance >= 1 / NONE / INVALID / won {counts}, deepest {full[full <= tref.MAX_DEPTH].max()}")
    _check_tables(_env(S, mc, blk, init, tgt), S, dist, (S, T, K, mc))


@pytest.mark.parametrize("S,T,K", ((1, 1, 0), (2, 2, 1), (3, 2, 1), (6, 2, 6), (7, 2, 8), (3, 5, 0)))
def test_the_remaining_board_sizes(torch_cuda, oracle, S, T, K):
    """With the rows above, every build kernel of the library (tests/test_table_cpu.py pins the list to the code object) and the
    lookup kernel of every board size runs against its yardstick: _check_tables forces both forms of every size."""
    import table_reference as tref
    n = 24
    for mc in (False, True):
        if S == 1:   # one cell: the tile sits on its target (won), or there is no target to sit on (single colour: never won)
            blk, init = np.zeros((1, n), np.uint32), np.zeros((1, n), np.uint8)
            tgt = np.zeros((1 if mc else 0, n), np.uint8)
        elif 2 * T + K > S * S:   # 3x3 with five tiles: the targets are drawn on their own and may lie under tiles
            blk, init, _ = oracle.generate(S, T, 0, 1, n, seed=0x50F7)
            _, _, tgt = oracle.generate(S, 0, T, 0, n, seed=0x50F8)
        else:
            blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(1000, 1000 + n, dtype=np.uint32))
        env = _env(S, mc, blk, init, tgt)
        dist = tref.exact(oracle, S, mc, blk, tgt, T)
        _check_tables(env, S, dist, (S, T, mc))
        table = env.build_table()
        got, want = env.lookup_bits(table), env.solve_bits(SOLVE_MAX_DEPTH)
        assert torch_cuda.equal(got[0], want[0]) and torch_cuda.equal(got[1], want[1])


def _lookup_raw(env, table, rows, moves=True, best=True, action=True):
    """ts_table_lookup through the C-ABI with any subset of its outputs; buffers prefilled so that an untouched one shows."""
    torch = __import__("torch")
    from tiler_slider_amd import _table_cabi as tc
    n = env.num_envs
    out = [torch.full((n,), 77, dtype=dt, device=env.device) if on else None
           for dt, on in ((torch.int16, moves), (torch.uint8, best), (torch.uint8, action))]
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = tc.lib().ts_table_lookup(C.byref(env._dims), C.byref(env._state), table.dist.data_ptr(), table.dist.shape[0], ptr(rows),
                                  ptr(out[0]), ptr(out[1]), ptr(out[2]), torch.cuda.current_stream(env.device).cuda_stream)
    return rc, out


_LOWEST = np.array([255, 0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0, 2, 0, 1, 0], np.uint8)


@pytest.mark.parametrize("S,T,K,mc,n", ((4, 2, 2, False, 3000), (4, 2, 2, True, 3000), (5, 3, 3, True, 500), (6, 3, 6, False, 150), (8, 2, 10, True, 500),
                                        (3, 4, 1, False, 300), (4, 4, 2, True, 60)))
def test_lookup_against_the_merged_solver(torch_cuda, oracle, S, T, K, mc, n):
    """On the boards as reset and after each of 24 steps of seeded random actions with auto_reset (max_steps = 5: boards win, time
    out and are put back all along): lookup_bits(table) == solve_bits(TS_SOLVE_MAX_DEPTH), expert_actions_from == expert_actions,
    and each optional output may be left out alone.  The table is built once, before the first step."""
    torch = torch_cuda
    from tiler_slider_amd import VecTilerSliderEnv
    env = VecTilerSliderEnv.from_seeds(np.arange(n), size=S, num_tiles=T, num_obstacles=K, multi_color=mc, obs_dtype=None, max_steps=5, auto_reset=True)
    env.reset()
    table = env.build_table()
    assert bool(table.complete.all())
    kinds = np.zeros(2, np.int64)
    moved = 0
    for step in range(25):
        before = [t.clone() for t in (env._pos, env._step_count, env._done, env._init, env._tgt, env._blk, table.dist)]
        want = env.solve_bits(SOLVE_MAX_DEPTH)
        got = env.lookup_bits(table)
        assert got[0].dtype == torch.int16 and got[1].dtype == torch.uint8
        assert torch.equal(got[0], want[0]), (step, "moves")
        assert torch.equal(got[1], want[1]), (step, "best")
        m4, b4 = env.lookup(table)
        assert b4.dtype == torch.bool and tuple(b4.shape) == (n, 4) and torch.equal(m4, want[0])
        assert torch.equal(b4, (want[1].unsqueeze(1) >> torch.arange(4, dtype=torch.uint8, device=b4.device) & 1).to(torch.bool))
        act = env.expert_actions_from(table)
        assert act.dtype == torch.uint8 and torch.equal(act, env.expert_actions(SOLVE_MAX_DEPTH))
        np.testing.assert_array_equal(act.cpu().numpy(), _LOWEST[want[1].cpu().numpy()])
        for a, b in zip(before, (env._pos, env._step_count, env._done, env._init, env._tgt, env._blk, table.dist)):
            assert torch.equal(a, b)   # neither call writes state or table
        if step in (0, 9):
            for keep in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
                rc, out = _lookup_raw(env, table, None, *map(bool, keep))
                assert rc == 0
                for o, w in zip(out, (want[0], want[1], act)):
                    assert o is None or torch.equal(o, w), (step, keep)
        m = want[0].cpu().numpy()
        kinds += ((m >= 1).sum(), (m == -1).sum())
        moved += int((env._pos != env._init).any(dim=0).sum())
        env.step(torch.from_numpy(oracle.fill_actions(n, seed=0x7AB1E, step_index=step)))
    # solvable and unsolvable boards were both looked up, away from their start (a board that wins is put back within its step, so
    # a won board is not seen here; test_playing_the_table_wins_... looks those up)
    assert kinds.min() >= 3 and moved >= 3, (kinds, moved)


def test_playing_the_table_wins_the_screenshot_levels_in_their_recorded_optimum(torch_cuda, oracle):
    """Stepping with expert_actions_from(table): every level wins after exactly its fixture min_moves steps, `moves` falling by
    one on every step until then."""
    torch = torch_cuda
    import solver_reference as ref
    from tiler_slider_amd.levels import pack_levels
    total = 0
    for (S, T, mc), (ids, blk, init, tgt, want) in ref.fixture_groups(GOLDEN_DIR, pack_levels).items():
        env = _env(S, mc, blk, init, tgt, max_steps=1000)
        table = env.build_table()
        left, _ = env.lookup_bits(table)
        np.testing.assert_array_equal(left.cpu().numpy(), want)
        won_at = torch.full((len(ids),), -1, dtype=torch.int32, device=left.device)
        for step in range(1, int(want.max()) + 1):
            act = env.expert_actions_from(table)
            assert torch.equal(act != 255, left >= 1)
            _, _, info = env.step(act)
            assert torch.equal(info["bad_action"] | info["stepped_done"], left < 1)   # untouched: already won
            now, _ = env.lookup_bits(table)
            assert torch.equal(now[left >= 1], left[left >= 1] - 1) and bool((now[left < 1] == 0).all())
            won_at[(left == 1) & info["is_won"]] = step
            left = now
        np.testing.assert_array_equal(won_at.cpu().numpy(), want.astype(np.int32))
        assert bool(env.is_won().all())
        total += len(ids)
    assert total == 400


def test_rows_let_a_table_of_levels_serve_many_boards(torch_cuda, oracle):
    """A table of the L screenshot levels of one shape serves N = 64 L replicated boards in shuffled order, mid-episode: the same
    answers as the per-board table.  Rows outside the table give NONE / 0 / 255 and, under `strict`, raise."""
    torch = torch_cuda
    import solver_reference as ref
    from tiler_slider_amd import SOLVE_NONE
    from tiler_slider_amd.levels import pack_levels
    rng = np.random.default_rng(0x7AB1E)
    for (S, T, mc), (ids, blk, init, tgt, want) in ref.fixture_groups(GOLDEN_DIR, pack_levels).items():
        L = len(ids)
        N = 64 * L
        level = rng.permutation(np.repeat(np.arange(L), 64)).astype(np.int32)
        small = _env(S, mc, blk, init, tgt)
        big = _env(S, mc, np.ascontiguousarray(blk[:, level]), np.ascontiguousarray(init[:, level]), np.ascontiguousarray(tgt[:, level]),
                   max_steps=6, auto_reset=True)
        table, own = small.build_table(), big.build_table()
        assert len(table) == L and len(own) == N
        assert torch.equal(own.dist, table.dist[torch.from_numpy(level).to(table.dist.device).long()])
        rows = torch.from_numpy(level).to(big.device)
        for step in range(6):
            for r in (rows, level, rows.long()):   # a device tensor as it is, a numpy array, another integer type
                got, ref_ = big.lookup_bits(table, rows=r), big.lookup_bits(own)
                assert torch.equal(got[0], ref_[0]) and torch.equal(got[1], ref_[1])
            assert torch.equal(big.expert_actions_from(table, rows=rows), big.expert_actions_from(own))
            assert torch.equal(big.lookup(table, rows)[1], big.lookup(own)[1])
            if step == 0:
                np.testing.assert_array_equal(got[0].cpu().numpy(), want[level])
            big.step(torch.from_numpy(oracle.fill_actions(N, seed=0x20775, step_index=step)))
        # rows outside the table
        bad = rows.clone()
        where = torch.from_numpy(rng.choice(N, 40, replace=False)).to(big.device)
        bad[where] = torch.tensor([-1, L, 2**31 - 1, -2**31] * 10, dtype=torch.int32, device=big.device)
        inside = torch.ones(N, dtype=torch.bool, device=big.device)
        inside[where] = False
        ref_ = big.lookup_bits(own)
        ref_act = big.expert_actions_from(own)
        got, act = big.lookup_bits(table, rows=bad), big.expert_actions_from(table, rows=bad)
        assert torch.equal(got[0][inside], ref_[0][inside]) and torch.equal(got[1][inside], ref_[1][inside]) and torch.equal(act[inside], ref_act[inside])
        assert bool((got[0][~inside] == SOLVE_NONE).all()) and bool((got[1][~inside] == 0).all()) and bool((act[~inside] == 255).all())
        wide = rows.long()
        wide[where] = 2**32     # would wrap to row 0 as an int32
        got = big.lookup_bits(table, rows=wide)
        assert torch.equal(got[0][inside], ref_[0][inside]) and bool((got[0][~inside] == SOLVE_NONE).all()) and bool((got[1][~inside] == 0).all())
        strict = _env(S, mc, np.ascontiguousarray(blk[:, level]), np.ascontiguousarray(init[:, level]), np.ascontiguousarray(tgt[:, level]), strict=True)
        assert torch.equal(strict.lookup_bits(table, rows=rows)[0], torch.from_numpy(want[level]).to(big.device))
        for call in (strict.lookup_bits, strict.lookup, strict.expert_actions_from):
            with pytest.raises(ValueError, match="rows"):
                call(table, rows=bad)
        with pytest.raises(ValueError, match="rows"):     # a table of L rows for 64 L boards, and no rows
            big.lookup_bits(table)
        with pytest.raises(ValueError, match="rows"):
            big.lookup_bits(table, rows=rows[:-1])


def test_host_checks(torch_cuda, oracle):
    from tiler_slider_amd import DistanceTable, VecTilerSliderEnv
    mk = lambda **kw: VecTilerSliderEnv.random(16, obs_dtype=None, **{"size": 4, "num_tiles": 2, "num_obstacles": 2, **kw})
    env = mk()
    env.reset()
    table = env.build_table()
    assert isinstance(table, DistanceTable) and (table.size, table.n_tiles, table.n_targets, table.multi_color, table.max_depth) == (4, 2, 2, False, 252)
    assert tuple(table.dist.shape) == (16, 256) and tuple(table.complete.shape) == (16,)
    # a table of another shape: size, tile count, colour mode
    for other in (mk(size=5), mk(num_tiles=3), mk(multi_color=True)):
        other.reset()
        for call in (other.lookup, other.lookup_bits, other.expert_actions_from):
            with pytest.raises(ValueError, match="built for"):
                call(table)
    with pytest.raises(TypeError):
        env.lookup_bits(table.dist)
    # unsupported shapes, as solve()
    for S, T in ((5, 4), (9, 1)):
        big = mk(size=S, num_tiles=T)
        with pytest.raises(ValueError, match="65536"):
            big.build_table()
        with pytest.raises(ValueError, match="65536"):
            big.lookup_bits(table)
    for depth in (-1, 253, 40000):
        with pytest.raises(ValueError, match="max_depth"):
            env.build_table(max_depth=depth)
    # max_bytes: the message names the size and points to rows=
    with pytest.raises(ValueError, match=r"4096 bytes.*rows="):
        env.build_table(max_bytes=4095)
    assert tuple(env.build_table(max_bytes=4096).dist.shape) == (16, 256)
    # a table cut at depth 0 says which rows are incomplete, and its lookups report SOLVE_DEPTH there
    from tiler_slider_amd import SOLVE_DEPTH, TABLE_DEEP
    shallow = env.build_table(max_depth=0)
    assert shallow.max_depth == 0
    deep_rows = (shallow.dist == TABLE_DEEP).any(dim=1)
    assert shallow.complete.tolist() == (~deep_rows).tolist()
    moves, best = env.lookup_bits(shallow)
    full_moves, _ = env.lookup_bits(table)
    assert bool((moves[full_moves >= 1] == SOLVE_DEPTH).all()) and bool((best[moves < 0] == 0).all())
    assert bool((moves[full_moves == 0] == 0).all())
    env.close()
    with pytest.raises(RuntimeError):
        env.build_table()
