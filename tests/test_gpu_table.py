"""ts_table_build and ts_table_lookup on the GPU, exact equality everywhere: whole tables byte for byte against the CPU yardstick
(tests/table_reference.py: backward relaxation over the oracle's successors), lookups against the yardstick's own lookup over
built and over made-up rows, and against the merged solver (ts_solve) where the header says the two are equal.  Every raw call
writes into memory the test owns: prefilled with the bytewise complement of the expected answer, between guard bytes - an entry
the kernel skips cannot compare equal, and a byte it writes outside its output shows."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from table_harness import GUARD, OCCUPANCY_CASES, SUB_WAVE, SUB_WAVE_CASE, guarded as _guarded, knobs as _knobs, payload as _payload

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


def _build_raw(env, want, max_depth=252):
    """ts_table_build through the C-ABI into a buffer prefilled with the complement of the yardstick's table `want`."""
    torch = __import__("torch")
    from tiler_slider_amd import _table_cabi as tc
    buf = _guarded(torch, env.device, want ^ np.uint8(0xFF))
    rc = tc.lib().ts_table_build(C.byref(env._dims), C.byref(env._state), int(max_depth), buf.data_ptr() + GUARD,
                                 torch.cuda.current_stream(env.device).cuda_stream)
    assert rc == 0, rc
    return _payload(buf, np.uint8, want.shape)


def _kinds(moves):
    """(boards or entries with moves >= 1, = 0, = -1) of a yardstick's answer."""
    moves = np.asarray(moves)
    return int((moves >= 1).sum()), int((moves == 0).sum()), int((moves == -1).sum())


def _cells_of(S, T, idx):
    C = S * S
    return np.stack([(idx // C ** t) % C for t in range(T)]).astype(np.uint8) if T else np.zeros((0, len(idx)), np.uint8)


def _valid_placements(rng, S, T, full, level):
    """uint8 [T, N]: for board n a valid placement of level[n] (a row of the yardstick's table `full`), drawn uniformly without
    repetition; where a level has no more valid placements than boards, its boards go through all of them in turn."""
    import table_reference as tref
    idx = np.empty(len(level), np.int64)
    for l in range(full.shape[0]):
        mine, valid = np.flatnonzero(level == l), np.flatnonzero(full[l] != tref.INVALID)
        assert valid.size
        idx[mine] = valid[np.arange(mine.size) % valid.size] if valid.size <= mine.size else rng.choice(valid, mine.size, replace=False)
    return _cells_of(S, T, idx)


def _put(env, name, a):
    """Overwrite a state tensor of the environment (env._pos, env._tgt) from NumPy, as test_gpu_solver._env does."""
    torch = __import__("torch")
    t = getattr(env, name)
    assert tuple(t.shape) == a.shape and a.dtype == np.uint8
    if a.size:
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(t.device))


class _forms(_knobs):
    """The launch forms a shape can be built in: the library's own, each of the two forced where both are compiled (boards 2x2 ..
    8x8), and the wave form with 32 placements per lane (several boards per wave).  Restores the knobs."""

    def __init__(self, S):
        super().__init__({})
        self.S = S

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


def _check_tables(env, S, dist, ctx):
    """Every form, max_depth = 252 (the default), 0, 3 and 7: the whole table equals the yardstick's - built through the host
    wrapper (dtype, shape, `complete`), and through the C-ABI into the complement of the expected table between guard bytes
    (_build_raw: "every entry of the table exactly once" - an entry left unwritten differs by construction)."""
    import table_reference as tref
    from tiler_slider_amd import _table_cabi as tc
    full = tref.cut(dist)
    seen = set()
    with _forms(S) as forms:
        for form in forms:
            d = tc.describe_table_build(env._dims)
            seen.add(d["name"])
            assert d["name"] == (f"k_table_block<{S}>" if form == "block form" else f"k_table_wave<{S}>") or form == "library policy"
            np.testing.assert_array_equal(_build_raw(env, full), full, err_msg=f"{ctx} {form}, into the complement")
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
                np.testing.assert_array_equal(_build_raw(env, want, depth), want, err_msg=f"{ctx} {form} depth {depth}, into the complement")
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


def _lookup_raw(env, table, rows, moves=True, best=True, action=True, want=None):
    """ts_table_lookup through the C-ABI with any subset of its outputs, each into a guarded buffer of its own: prefilled with the
    complement of `want` = (moves, best, action) where the expected answer is known beforehand, with 77 otherwise (no answer of
    the library: moves 19789, best and action 77).  `table`: a DistanceTable or a uint8 [n_rows, states] tensor of any bytes.
    Returns rc and the outputs as tensors, None where one was left out; the guards are checked here."""
    torch = __import__("torch")
    from tiler_slider_amd import _table_cabi as tc
    n = env.num_envs
    dist = table if isinstance(table, torch.Tensor) else table.dist
    kinds = ((np.int16, torch.int16, moves), (np.uint8, torch.uint8, best), (np.uint8, torch.uint8, action))
    bufs = [None if not on else _guarded(torch, env.device, np.full(n, 77, dt) if want is None else ~np.asarray(want[i]).astype(dt))
            for i, (dt, _, on) in enumerate(kinds)]
    ptr = lambda t: None if t is None else t.data_ptr()
    out = lambda b: None if b is None else b.data_ptr() + GUARD
    rc = tc.lib().ts_table_lookup(C.byref(env._dims), C.byref(env._state), dist.data_ptr(), dist.shape[0], ptr(rows),
                                  out(bufs[0]), out(bufs[1]), out(bufs[2]), torch.cuda.current_stream(env.device).cuda_stream)
    res = []
    for b, (dt, tt, _) in zip(bufs, kinds):
        if b is None:
            res.append(None)
            continue
        _payload(b, dt, (n,))
        res.append(b[GUARD:b.numel() - GUARD].view(tt))
    return rc, res


def _lookup_checked(env, table, rows, want, ctx, alone=True):
    """All three outputs in one call, then each alone (the `best || action` branch changes what the kernel computes): == want."""
    for keep in ((1, 1, 1),) + (((1, 0, 0), (0, 1, 0), (0, 0, 1)) if alone else ()):
        rc, out = _lookup_raw(env, table, rows, *map(bool, keep), want=want)
        assert rc == 0
        for o, w, what in zip(out, want, ("moves", "best", "action")):
            if o is not None:
                np.testing.assert_array_equal(o.cpu().numpy(), w, err_msg=f"{ctx} {what} {keep}")


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


# ---------------------------------------------------------------------------------------------- every kernel at occupancy
OCC_DISTINCT, OCC_WAVES, OCC_CUT_DEPTH = 128, 4096, 2


def _occupancy_levels(oracle, S, T, K, mc, n):
    """Drawn as test_gpu_solver.test_every_compiled_form_at_occupancy draws them."""
    if S == 1:   # one cell: the tile sits on its target (won), or there is no target to sit on (single colour: never won)
        return np.zeros((1, n), np.uint32), np.zeros((1, n), np.uint8), np.zeros((1 if mc else 0, n), np.uint8)
    if 2 * T + K > S * S:   # the 2x2 case (two tiles, an obstacle: 5 > 4 cells): the targets are drawn on their own and may lie under tiles
        blk, init, _ = oracle.generate(S, T, 0, K, n, seed=0x50F7)
        _, _, tgt = oracle.generate(S, 0, T, 0, n, seed=0x50F8)
        return blk, init, tgt
    return oracle.generate_mt19937(S, T, T, K, np.arange(1000, 1000 + n, dtype=np.uint32))


def _occupancy_build(oracle, name, S, T, K, knobs):
    import table_reference as tref
    from tiler_slider_amd import _cabi
    from tiler_slider_amd import _table_cabi as tc
    kernel = name.split(",")[0]
    for mc in (False, True):
        blk, init, tgt = _occupancy_levels(oracle, S, T, K, mc, OCC_DISTINCT)
        dist = tref.exact(oracle, S, mc, blk, tgt, T)
        full, shallow = tref.cut(dist), tref.cut(dist, OCC_CUT_DEPTH)
        kinds = _kinds(tref.to_moves(full))
        print(f"{name} mc={mc}: entries with moves >= 1 / 0 / -1 {kinds}, deepest {full[full <= tref.MAX_DEPTH].max() if kinds[0] + kinds[1] else None}")
        assert S == 1 or min(kinds) >= 3, kinds
        with _knobs(knobs):
            d = tc.describe_table_build(_cabi.Dims(OCC_DISTINCT, S, T, tgt.shape[0], int(mc), 100, 0))
            assert d["name"] == kernel
            waves_per_block = d["threads_per_block"] // 64
            copies = -(-OCC_WAVES * d["boards_per_block"] // (waves_per_block * OCC_DISTINCT)) + 1
            n = copies * OCC_DISTINCT - 3   # a ragged last block
            tile = lambda a: np.ascontiguousarray(np.tile(a, (1, copies))[:, :n])
            env = _env(S, mc, tile(blk), tile(init), tile(tgt))
            d = tc.describe_table_build(env._dims)
            assert d["name"] == kernel and d["blocks"] * waves_per_block >= OCC_WAVES
            if name == SUB_WAVE:
                assert d["boards_per_block"] == 8 and n % 8 != 0
            for want, depth in ((full, 252), (shallow, OCC_CUT_DEPTH)):
                want = np.tile(want, (copies, 1))[:n]
                np.testing.assert_array_equal(_build_raw(env, want, depth), want, err_msg=f"{name} mc={mc} max_depth {depth}")
            env.close()


def _occupancy_lookup(oracle, name, S, T, K):
    torch = __import__("torch")
    import table_reference as tref
    rng = np.random.default_rng(0x0CC + S)
    for mc in (False, True):
        blk, init, tgt = _occupancy_levels(oracle, S, T, K, mc, OCC_DISTINCT)
        full = tref.table(oracle, S, mc, blk, tgt, T)
        copies = -(-OCC_WAVES * 64 // OCC_DISTINCT) + 1   # one board per lane
        n = copies * OCC_DISTINCT - 3
        assert n >= OCC_WAVES * 64 - 3
        level = (np.arange(n) % OCC_DISTINCT).astype(np.int32)
        tile = lambda a: np.ascontiguousarray(np.tile(a, (1, copies))[:, :n])
        pos = _valid_placements(rng, S, T, full, level)
        want = tref.lookup(oracle, S, tile(blk), pos, full, rows=level)   # over the YARDSTICK's rows
        kinds = _kinds(want[0])
        print(f"{name} mc={mc}: {n} boards with moves >= 1 / 0 / -1 {kinds}, deepest {want[0].max()}, with a best move {(want[1] != 0).sum()}")
        assert S == 1 or min(kinds) >= 3, kinds
        small = _env(S, mc, blk, init, tgt)
        table = small.build_table()
        np.testing.assert_array_equal(table.dist.cpu().numpy(), full)
        env = _env(S, mc, tile(blk), tile(init), tile(tgt))
        _put(env, "_pos", pos)
        assert -(-n // 64) >= OCC_WAVES
        _lookup_checked(env, table, torch.from_numpy(level).to(env.device), want, f"{name} mc={mc}")
        env.close()
        small.close()


@pytest.mark.parametrize("name", sorted(OCCUPANCY_CASES) + [SUB_WAVE])
def test_every_compiled_table_kernel_at_occupancy(torch_cuda, oracle, name):
    """Every kernel of the table library, 128 distinct levels tiled to at least 4,096 waves - two waves per SIMD and more, as
    tests/test_kernel_instantiations.py runs the step kernels and test_gpu_solver.py the solver's: every copy of a level gets the
    yardstick's row for it (max_depth 252 and 2, into the complement of the expected table), every board of a lookup the
    yardstick's answer from a placement drawn from ALL valid placements of its level (won, unreachable, never visited)."""
    if name == SUB_WAVE:
        _occupancy_build(oracle, name, *SUB_WAVE_CASE)
    elif "lookup" in name:
        _occupancy_lookup(oracle, name, *OCCUPANCY_CASES[name][:3])
    else:
        _occupancy_build(oracle, name, *OCCUPANCY_CASES[name])


# ---------------------------------------------------------------------------------------------- lookups over made-up tables
_OWN_ENTRIES = (1, 127, 128, 129, 251, 252, 253, 254, 255)


def _made_up_table(oracle, rng, S, T, blk, valid):
    """(table uint8 [L + H, states], level int32 [N], rows int32 [N], pos uint8 [T, N]): L seeded rows in which every byte
    value occurs and 120 .. 255 make up more than a third, with boards on random valid placements of the L levels; and H
    hand-placed rows, one per board: the board's own entry e is each of _OWN_ENTRIES, the entries of its four successors (from
    the oracle) are e - 1, e, e + 1 and the three codes, in six rotations over the moves."""
    L, states = valid.shape
    base = np.concatenate([np.array(_OWN_ENTRIES + (0,)), rng.integers(1, 253, L)])[:L].astype(np.int64)
    u = rng.random((L, states))
    near = (base[:, None] + rng.integers(-1, 2, (L, states))) % 256
    table = np.where(u < 0.5, near, np.where(u < 0.75, rng.integers(120, 256, (L, states)), rng.integers(0, 256, (L, states)))).astype(np.uint8)
    per = 150
    level = np.repeat(np.arange(L), per)
    idx = np.concatenate([rng.choice(np.flatnonzero(valid[l]), per) for l in range(L)])
    # the hand-placed rows
    H = len(_OWN_ENTRIES) * 6
    hl = np.arange(H) % L
    hidx = np.array([rng.choice(np.flatnonzero(valid[l])) for l in hl])
    hpos = _cells_of(S, T, hidx)
    import table_reference as tref
    hand = np.empty((H, states), np.uint8)
    succ = []
    for a in range(4):
        batch = oracle.OracleBatch(S, False, 2**30, np.ascontiguousarray(blk[:, hl]), hpos, np.zeros((0, H), np.uint8))
        batch.step(np.full(H, a, np.uint8), obs=False)
        succ.append(tref.index_of(S, batch.pos))
    for k in range(H):
        e, turn = _OWN_ENTRIES[k // 6], k % 6
        around = ((e - 1) % 256, e, (e + 1) % 256, 253, 254, 255)
        hand[k] = e
        for a in range(4):
            hand[k, succ[a][k]] = around[(turn + a) % 6]
        hand[k, hidx[k]] = e     # last: a move that slides nothing leads back to the board's own entry
    return (np.concatenate([table, hand]), np.concatenate([level, hl]).astype(np.int32),
            np.concatenate([level, L + np.arange(H)]).astype(np.int32), np.concatenate([_cells_of(S, T, idx), hpos], axis=1))


@pytest.mark.parametrize("S,K", ((4, 2), (5, 3), (6, 6), (8, 10)))
def test_lookups_over_made_up_tables(torch_cuda, oracle, S, K):
    """ts_table_lookup reads whatever bytes it is given: rows nobody built, holding every value 0 .. 255, on boards standing on
    valid placements of real levels; sizes with 32-bit (4, 5) and 64-bit (6, 8) masks; with `rows` and without."""
    torch = torch_cuda
    import table_reference as tref
    T, L = 2, 24
    rng = np.random.default_rng(0x7AB1E + S)
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(L, dtype=np.uint32))
    states = (S * S) ** T
    valid = tref.is_placement(S, np.repeat(blk, states, axis=1), np.tile(_cells_of(S, T, np.arange(states)), (1, L))).reshape(L, states)
    table, level, rows, pos = _made_up_table(oracle, rng, S, T, blk, valid)
    # properties of the INPUT, before the GPU is asked anything
    assert np.unique(table).size == 256 and (table >= 120).mean() >= 1 / 3
    own = table[rows, tref.index_of(S, pos)]
    assert set(_OWN_ENTRIES) <= set(own.tolist()) and (own >= 128).sum() >= 100
    b = np.ascontiguousarray(blk[:, level])
    want = tref.lookup(oracle, S, b, pos, table, rows=rows)
    print(f"{S}x{S}: {len(rows)} boards, own entry >= 128 on {(own >= 128).sum()}, moves >= 1 / 0 / -1 {_kinds(want[0])}, -2 on {(want[0] == -2).sum()}, "
          f"with a best move {(want[1] != 0).sum()}, largest moves {want[0].max()}")
    assert want[0].max() == 252 and (want[0] == -2).sum() >= 3 and (want[1] != 0).sum() >= 100 and min(_kinds(want[0])) >= 3
    assert ((want[1] != 0) & (own >= 129)).sum() >= 3      # a best move found by comparing bytes >= 128
    env = _env(S, bool(S % 2), b, np.ascontiguousarray(init[:, level]), np.ascontiguousarray(tgt[:, level]))
    _put(env, "_pos", pos)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.device)
    _lookup_checked(env, dev(table), dev(rows), want, f"{S}x{S} rows")
    own_rows = table[rows]                                   # a row per board: rows = NULL
    np.testing.assert_array_equal(tref.lookup(oracle, S, b, pos, own_rows)[0], want[0])
    _lookup_checked(env, dev(own_rows), None, want, f"{S}x{S} no rows")


# ---------------------------------------------------------------------------------------------- the shapes and cells the header names
def _lookups_from_valid_placements(env, oracle, S, T, blk, full, ctx):
    """The boards as they stand, on a seeded draw from the valid placements of their levels, on a won placement of every level
    that has one, and on one at a distance >= 1 (random valid ones elsewhere): == table_reference.lookup over the yardstick's
    table `full` (the GPU-built table is compared with `full` by _check_tables)."""
    import table_reference as tref
    rng = np.random.default_rng(0x5EED + S * 16 + T)
    table = env.build_table()
    level = np.arange(full.shape[0])
    seen = []
    for r, pick in enumerate((None, full != tref.INVALID, full == 0, (full >= 1) & (full <= tref.MAX_DEPTH))):
        if pick is not None:
            pos = _valid_placements(rng, S, T, full, level)
            idx = tref.index_of(S, pos)
            for l in np.flatnonzero(pick.any(axis=1)):
                idx[l] = rng.choice(np.flatnonzero(pick[l]))
            _put(env, "_pos", _cells_of(S, T, idx))
        pos = env._pos.cpu().numpy()
        want = tref.lookup(oracle, S, blk, pos, full)
        _lookup_checked(env, table, None, want, f"{ctx} draw {r}", alone=r == 1)
        seen.append(want[0])
    return np.concatenate(seen)


# S, tiles, targets, obstacles, multi colour, the first target row copied over the last, levels, can be won
MISMATCHED = ((4, 2, 3, 2, False, True, 400, True), (5, 2, 3, 3, False, True, 300, True), (6, 2, 3, 6, False, True, 100, True),
              (7, 2, 3, 8, False, True, 60, True), (8, 2, 3, 10, False, True, 40, True), (3, 3, 4, 1, False, True, 100, True),
              (2, 2, 3, 0, False, True, 24, True),
              # never won: more distinct targets than tiles, more tiles than targets; multi colour with n_tiles != n_targets, and
              # with a repeated target (two tiles never share a cell)
              (4, 2, 3, 2, False, False, 100, False), (4, 3, 1, 2, False, False, 100, False), (4, 2, 3, 2, True, False, 100, False),
              (4, 3, 3, 2, True, True, 100, False))


def _mismatched_levels(oracle, S, T, Tt, K, dup, n):
    blk, init, _ = oracle.generate(S, T, 0, K, n, seed=0x50F7)
    _, _, tgt = oracle.generate(S, 0, Tt, 0, n, seed=0x50F8)
    if dup:
        tgt[-1] = tgt[0]
    return blk, init, tgt


@pytest.mark.parametrize("S,T,Tt,K,mc,dup,n,winnable", MISMATCHED)
def test_tables_with_other_target_counts_and_repeated_targets(torch_cuda, oracle, S, T, Tt, K, mc, dup, n, winnable):
    """n_tiles != n_targets and repeated targets, as the header defines them: single colour compares the SETS of cells (three
    targets on two cells are covered by two tiles), multi colour is never won unless n_tiles == n_targets and the targets are
    distinct.  Every form and depth, then lookups."""
    import table_reference as tref
    blk, init, tgt = _mismatched_levels(oracle, S, T, Tt, K, dup, n)
    dist = tref.exact(oracle, S, mc, blk, tgt, T)
    full = tref.cut(dist)
    counts = (int(((full >= 1) & (full <= tref.MAX_DEPTH)).sum()), int((full == tref.NONE).sum()), int((full == tref.INVALID).sum()), int((full == 0).sum()))
    print(f"{S}x{S} T={T} Tt={Tt} K={K} mc={mc} dup={dup}: entries at distance >= 1 / NONE / INVALID / won {counts}, "
          f"levels with a won placement {(full == 0).any(axis=1).sum()}, deepest {full[full <= tref.MAX_DEPTH].max() if winnable else None}")
    if winnable:
        assert min(counts) >= 3, counts
    else:
        assert counts[0] == 0 and counts[3] == 0 and counts[1] >= 3 and counts[2] >= 3, counts
    env = _env(S, mc, blk, init, tgt)
    _check_tables(env, S, dist, (S, T, Tt, mc, dup))
    moves = _lookups_from_valid_placements(env, oracle, S, T, blk, full, (S, T, Tt, mc, dup))
    assert (min(_kinds(moves)) >= 3) if winnable else (moves == -1).all()


@pytest.mark.parametrize("mc,targets,entry", ((False, [], 0), (True, [], 0), (False, [(0, 0)], 255), (True, [(0, 0)], 255)))
def test_zero_tiles_is_a_table_of_one_entry(torch_cuda, oracle, mc, targets, entry):
    """No tiles: one placement.  Without targets it is won as it stands; with a target it never is.  The lookup and ts_solve
    agree with the yardstick (the header: "with a complete table moves and best are exactly ts_solve's outputs")."""
    import table_reference as tref
    blk, init, tgt = oracle.pack_levels(3, [([(1, 1)], [], targets), ([], [], targets), ([(0, 0), (2, 2)], [], targets)])
    assert init.shape == (0, 3) and tgt.shape == (len(targets), 3)
    dist = tref.exact(oracle, 3, mc, blk, tgt, 0)
    env = _env(3, mc, blk, init, tgt)
    full = _check_tables(env, 3, dist, ("no tiles", mc, targets))
    assert full.tolist() == [[entry]] * 3
    want = tref.lookup(oracle, 3, blk, init, full)
    assert want[0].tolist() == [0 if entry == 0 else -1] * 3 and want[1].tolist() == [0] * 3 and want[2].tolist() == [255] * 3
    _lookup_checked(env, env.build_table(), None, want, ("no tiles", mc, targets))
    moves, best = env.solve_bits(SOLVE_MAX_DEPTH)
    np.testing.assert_array_equal(moves.cpu().numpy(), want[0])
    np.testing.assert_array_equal(best.cpu().numpy(), want[1])


@pytest.mark.parametrize("mc", (False, True))
@pytest.mark.parametrize("S,K", ((4, 2), (8, 10)))
def test_cells_beyond_the_board_are_clamped_and_invalid_placements_answered(torch_cuda, oracle, S, K, mc):
    """"Cell ids >= S*S are clamped to S*S - 1": target ids S*S .. 255 written into the environment before the build, tile ids
    before the lookup and ts_solve - the yardstick on the clipped arrays.  A board whose clipped cells are not a placement (two
    tiles on S*S - 1, a tile on an obstacle there), and one with in-range cells that are none, reports -1, 0, 255; ts_solve is
    held to the yardstick on the placements only."""
    import table_reference as tref
    T, n, C = 2, 400, S * S
    rng = np.random.default_rng(0xC1A + S + int(mc))
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    env = _env(S, mc, blk, init, tgt)
    beyond = lambda size: rng.choice(np.array([C, C + 1, 127, 128, 200, 254, 255]), size).astype(np.uint8)
    raw_tgt = tgt.copy()
    some = np.flatnonzero(rng.random(n) < 0.4)
    raw_tgt[rng.integers(0, T, some.size), some] = beyond(some.size)
    raw_tgt[:, some[:12]] = beyond((T, 12))                       # both targets on S*S - 1
    _put(env, "_tgt", raw_tgt)
    dist = tref.exact(oracle, S, mc, blk, np.minimum(raw_tgt, C - 1), T)
    full = _check_tables(env, S, dist, (S, mc, "clamped targets"))
    changed = (tref.table(oracle, S, mc, blk, tgt, T) != full).any(axis=1)
    print(f"{S}x{S} mc={mc}: {some.size} levels with a target id beyond the board, the table of {changed.sum()} differs from the in-range level's")
    assert changed.sum() >= 3
    # tiles: valid placements, then one or both ids beyond the board, and in-range cells that are no placement
    table = env.build_table()
    raw_pos = _valid_placements(rng, S, T, full, np.arange(n))
    last_blocked = ((blk[(C - 1) >> 5] >> ((C - 1) & 31)) & 1) != 0
    one = np.flatnonzero(rng.random(n) < 0.5)
    which = rng.integers(0, T, one.size)
    states = np.arange(C ** T)
    for b, t in zip(one, which):   # where the level has one: a placement with that tile on S*S - 1 from which the board can be won
        near = np.flatnonzero(((states // C ** t) % C == C - 1) & (full[b] >= 1) & (full[b] <= tref.MAX_DEPTH))
        if near.size:
            raw_pos[:, b] = _cells_of(S, T, rng.choice(near, 1))[:, 0]
    raw_pos[which, one] = beyond(one.size)
    share = one[:20]
    raw_pos[:, share] = beyond((T, 20))                           # both tiles on S*S - 1
    twice, on_wall = one[20:30], one[30:40]
    raw_pos[:, twice] = _valid_placements(rng, S, T, full, twice)
    raw_pos[1, twice] = raw_pos[0, twice]                         # in range: two tiles on one cell
    raw_pos[:, on_wall] = _valid_placements(rng, S, T, full, on_wall)
    wall = np.array([next(c for c in range(C) if (int(blk[c >> 5, b]) >> (c & 31)) & 1) for b in on_wall])
    raw_pos[0, on_wall] = wall                                    # in range: a tile on an obstacle
    _put(env, "_pos", raw_pos)
    ok = tref.is_placement(S, blk, raw_pos)
    clipped = (raw_pos >= C).any(axis=0)
    print(f"{S}x{S} mc={mc}: {clipped.sum()} boards with a tile id beyond the board, {(clipped & ok).sum()} of them placements, "
          f"{(clipped & ~ok & last_blocked).sum()} on an obstacle at S*S - 1")
    assert not ok[share].any() and not ok[twice].any() and not ok[on_wall].any()
    assert (clipped & ok).sum() >= 3 and (clipped & ~ok & last_blocked).sum() >= 3
    want = tref.lookup(oracle, S, blk, raw_pos, full)
    assert (want[0][~ok] == -1).all() and (want[1][~ok] == 0).all() and (want[2][~ok] == 255).all()
    assert (want[0][clipped & ok] >= 1).sum() >= 3 and (want[0][clipped & ok] == -1).sum() >= 3, _kinds(want[0][clipped & ok])
    _lookup_checked(env, table, None, want, (S, mc, "clamped tiles"))
    moves, best = env.solve_bits(SOLVE_MAX_DEPTH)
    np.testing.assert_array_equal(moves.cpu().numpy()[ok], want[0][ok])
    np.testing.assert_array_equal(best.cpu().numpy()[ok], want[1][ok])


# ---------------------------------------------------------------------------------------------- streams
def test_step_build_lookup_and_solve_on_a_stream_of_their_own(torch_cuda, oracle):
    """2**18 boards, one extra stream, no host synchronisation until the end: step, build, lookup, solve are enqueued while the
    step still runs.  A launch that ignored its `stream` argument would read cells the step has not written yet."""
    torch = torch_cuda
    import table_reference as tref
    S, T, K, mc, distinct, copies = 4, 2, 2, False, 256, 1024
    n = distinct * copies
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(distinct, dtype=np.uint32))
    full = tref.table(oracle, S, mc, blk, tgt, T)
    tile = lambda a: np.ascontiguousarray(np.tile(a, (1, copies)))
    level = np.arange(n) % distinct
    twin = oracle.OracleBatch(S, mc, 100, tile(blk), tile(init), tile(tgt))
    twin.reset()
    act = oracle.fill_actions(n, seed=0x57EA, step_index=0)
    twin.step(act, obs=False)
    assert (twin.pos != twin.init).any(axis=0).sum() >= n // 4      # the step matters: the answers from the start cells differ
    want = tref.lookup(oracle, S, tile(blk), twin.pos, full, rows=level)
    start = tref.lookup(oracle, S, tile(blk), twin.init, full, rows=level)
    assert (want[0] != start[0]).sum() >= 1000 and min(_kinds(want[0])) >= 3
    env = _env(S, mc, tile(blk), tile(init), tile(tgt))
    actions = torch.from_numpy(act).to(env.device)
    side = torch.cuda.Stream(device=env.device)
    assert side.cuda_stream != torch.cuda.current_stream(env.device).cuda_stream
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        env.step(actions)
        table = env.build_table()
        got = env.lookup_bits(table)
        solved = env.solve_bits(SOLVE_MAX_DEPTH)
    side.synchronize()
    np.testing.assert_array_equal(env.positions.cpu().numpy(), twin.pos)
    np.testing.assert_array_equal(got[0].cpu().numpy(), want[0])
    np.testing.assert_array_equal(got[1].cpu().numpy(), want[1])
    np.testing.assert_array_equal(solved[0].cpu().numpy(), want[0])
    np.testing.assert_array_equal(solved[1].cpu().numpy(), want[1])
    dist = table.dist.cpu().numpy()
    np.testing.assert_array_equal(dist[:distinct], full)
    assert (dist.reshape(copies, distinct, -1) == full).all()
