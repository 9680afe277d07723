"""Every kernel of the reach and rtable libraries at occupancy, reachable sets of tens of thousands of states, and the probe at its
edges - against the CPU yardsticks (tests/reach_reference.py, tests/rtable_reference.py), exact equality everywhere.  The cases
are those of tests/reach_cases.py, pinned to the code objects by tests/test_reach_cpu.py and tests/test_rtable_cpu.py: more than
four tiles on every size that has room for them, keys beyond 2^32 on 6x6, 7x7 and 8x8.  The raw calls are those of
tests/test_gpu_reach.py and tests/test_gpu_rtable.py: outputs between guard bytes, prefilled with the complement of the yardstick's
answer, tables and workspaces prefilled with 0xA5.  What a test covers is decided from the yardstick's answer alone, before any GPU
call, and printed."""
import functools
import time

import numpy as np
import pytest

import reach_cases as cases
from test_gpu_reach import _raw, _same
from test_gpu_rtable import _env, _raw_build, _raw_lookup, _same_outputs

pytestmark = pytest.mark.gpu

KEY56 = np.uint64((1 << 56) - 1)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _oracle():
    from oracle import binding
    return binding


# ---------------------------------------------------------------------------------------------------- shared, computed once
@functools.lru_cache(maxsize=None)
def _levels(S, mc):
    return cases.levels(_oracle(), S, mc)


@functools.lru_cache(maxsize=None)
def _stepped(S, mc):
    return cases.stepped(_oracle(), S, mc, *_levels(S, mc))


@functools.lru_cache(maxsize=None)
def _yard_rtable(S, mc, root="init", max_depth=252, capacity=cases.CAPACITY):
    """The yardstick's Reference of the case's 128 levels.  Do not write to it."""
    import rtable_reference as rt
    blk, init, tgt = _levels(S, mc)
    return rt.build(_oracle(), S, mc, blk, tgt, init if root == "init" else _stepped(S, mc)[1], max_depth, capacity)


@functools.lru_cache(maxsize=None)
def _yard_reach(S, mc, max_depth=64, capacity=cases.CAPACITY):
    import reach_reference as reach
    blk, init, tgt = _levels(S, mc)
    return reach.solve(_oracle(), S, mc, blk, tgt, init, max_depth, capacity)


def _tile(a, n):
    """[..., L] -> [..., n]: board i is level i % L."""
    return np.ascontiguousarray(np.tile(a, (1,) * (a.ndim - 1) + (-(-n // a.shape[-1]),))[..., :n])


class _Tiled:
    """A Reference's outputs for n boards, board i a copy of level i % L (what _raw_build prefills against and _same_outputs compares)."""

    def __init__(self, ref, n):
        self.count, self.root_moves, self.deepest = (_tile(a, n) for a in (ref.count, ref.root_moves, ref.deepest))


def _pairs(ref, slots):
    """uint64 [L, slots]: the values entry << 48 | key of level l, sorted, at the end of row l; zeros before them."""
    L = len(ref.count)
    want = np.zeros((L, slots), np.uint64)
    vals = (ref.entry.astype(np.uint64) << np.uint64(48)) | ref.idx.astype(np.uint64)
    for l in range(L):
        v = np.sort(vals[ref.start[l]:ref.start[l + 1]])
        want[l, slots - v.size:] = v
    return want


def _same_pairs(rtab, ref, level, ctx):
    """The SET of (key, entry) pairs of every row that is not FULL is the yardstick's for its level: the table is copied to the host
    once and every row sorted there.  Every occupied slot is bit 63, an entry byte and a 48-bit key, every other slot is 0."""
    t = rtab.table.cpu().numpy().view(np.uint64)
    held = ref.count[level] >= 0
    t = t[held]
    assert ((t == 0) | ((t >> np.uint64(56)) == 0x80)).all(), f"a slot that is neither empty nor bit 63, an entry and a key: {ctx}"
    got = np.sort(t & KEY56, axis=1)
    want = _pairs(ref, t.shape[1])[level[held]]
    rows = np.flatnonzero((got != want).any(axis=1))
    assert rows.size == 0, f"the pairs of {rows.size} rows differ, the first is board {np.flatnonzero(held)[rows[0]]}: {ctx}"


def _free_cells(S, blk, l):
    cells = np.arange(S * S)
    return cells[((blk[cells // 32, l] >> (cells % 32).astype(np.uint32)) & 1) == 0]


def _random_placements(rng, S, T, blk, l, m):
    """[T, m]: uniformly random placements of T tiles on distinct free cells of level l."""
    free = _free_cells(S, blk, l)
    return free[np.argsort(rng.random((m, free.size)), axis=1)[:, :T]].T.astype(np.uint8)


def _kinds(moves):
    import rtable_reference as rt
    moves = np.asarray(moves)
    return dict(entry=int((moves >= 1).sum()), won=int((moves == 0).sum()), none=int((moves == rt.SOLVE_NONE).sum()),
                full=int((moves == rt.SOLVE_FULL).sum()), absent=int((moves == rt.SOLVE_ABSENT).sum()))


# ---------------------------------------------------------------------------------------------------- every kernel at occupancy
def _occupancy_reach(S):
    from tiler_slider_amd import _reach_cabi as rc
    n = cases.N_BUILD
    for mc in (False, True):
        blk, init, tgt = _levels(S, mc)
        s = cases.check_reach(S, _yard_reach(S, mc))
        print(f"k_reach<{S}> mc={mc}: {n} boards of {cases.DISTINCT} levels, T={init.shape[0]}: {s}")
        env = _env(S, mc, _tile(blk, n), _tile(init, n), _tile(tgt, n))
        assert rc.describe_reach(env._dims, 64, cases.CAPACITY)["boards_in_flight"] == cases.GRID
        for depth in (64, 3):
            want = tuple(_tile(a, n) for a in _yard_reach(S, mc, depth))
            _same(_raw(env, depth, cases.CAPACITY, want), want, (S, mc, depth))
        env.close()


def _occupancy_build(S):
    torch = __import__("torch")
    n = cases.N_BUILD
    level = np.arange(n) % cases.DISTINCT
    for mc in (False, True):
        blk, init, tgt = _levels(S, mc)
        s = cases.check_rtable(S, _yard_rtable(S, mc))
        print(f"k_rtable_build<{S}> mc={mc}: {n} levels, copies of {cases.DISTINCT}, T={init.shape[0]}: {s}")
        act, pos = _stepped(S, mc)
        env = _env(S, mc, _tile(blk, n), _tile(init, n), _tile(tgt, n), max_steps=1000)
        env.step(torch.from_numpy(_tile(act, n)))
        np.testing.assert_array_equal(env.positions.cpu().numpy(), _tile(pos, n))
        for root in ("init", "pos"):
            for depth in (252, 3):
                ref = _yard_rtable(S, mc, root, depth)
                rtab = _raw_build(env, _Tiled(ref, n), depth, cases.CAPACITY, root)
                _same_outputs(rtab, _Tiled(ref, n), (S, mc, root, depth))
                _same_pairs(rtab, ref, level, (S, mc, root, depth))
        env.close()


def _occupancy_lookup(S):
    import rtable_reference as rt
    n, L = cases.N_LOOKUP, cases.DISTINCT
    rng = np.random.default_rng(0x100C + S)
    for mc in (False, True):
        blk, init, tgt = _levels(S, mc)
        T = init.shape[0]
        ref = _yard_rtable(S, mc)
        cases.check_rtable(S, ref)
        level = np.arange(n) % L
        kind = rng.random(n)
        pos = np.ascontiguousarray(init[:, level])                      # a level without a state (won, FULL) and 1x1 without a target: its root
        for l in range(L):
            mine = np.flatnonzero(level == l)
            on_r, anywhere, on_tgt = mine[kind[mine] < 0.5], mine[(kind[mine] >= 0.5) & (kind[mine] < 0.75)], mine[kind[mine] >= 0.75]
            if ref.count[l] > 0:
                pos[:, on_r] = ref.cells(l)[:, rng.integers(0, ref.count[l], on_r.size)]
            pos[:, anywhere] = _random_placements(rng, S, T, blk, l, anywhere.size)
            if tgt.shape[0] == T:
                pos[:, on_tgt] = tgt[:, l:l + 1]
        rows = level.astype(np.int64)
        rows[rng.integers(0, n, 16)] = np.array([-1, L] * 8)
        b, t = _tile(blk, n), _tile(tgt, n)
        want = rt.lookup(_oracle(), ref, b, t, pos, rows=rows)
        kinds = _kinds(want[0])
        print(f"k_rtable_lookup<{S}> mc={mc}: {n} boards, T={T}: {kinds}, deepest {want[0].max()}, with a best move {(want[1] != 0).sum()}")
        if S >= 3:
            assert min(kinds.values()) >= 64, kinds
        elif S == 2:
            assert kinds["won"] and kinds["entry"] and kinds["absent"], kinds
        else:   # one cell: the tile sits on its target, or there is no target to sit on
            assert kinds["won" if mc else "none"] >= n - 16 and kinds["none"] >= 1, kinds
        small = _env(S, mc, blk, init, tgt)
        rtab = _raw_build(small, ref, 252, cases.CAPACITY)
        _same_outputs(rtab, ref, (S, mc, "the table of the lookups"))
        env = _env(S, mc, b, _tile(init, n), t, pos=pos)
        assert -(-n // 64) >= cases.LOOKUP_WAVES
        for name, g, w in zip(("moves", "best", "action"), _raw_lookup(env, rtab, rows, want), want):
            np.testing.assert_array_equal(g, w, err_msg=f"{name}: k_rtable_lookup<{S}> mc={mc}")
        env.close()
        small.close()


@pytest.mark.parametrize("name", sorted(cases.REACH_CASES) + sorted(cases.RTABLE_CASES))
def test_every_compiled_reach_and_rtable_kernel_at_occupancy(torch_cuda, oracle, name):
    """k_reach<S> and k_rtable_build<S>: 128 distinct levels tiled to 1,024 + 61 boards - a full grid of 1,024 blocks, each between
    two neighbours' slices, and a ragged second pass through 61 of the slices -; every copy of a level gets the yardstick's answer
    for it, at full depth and cut to 3, from both roots, the rows as SETS of (key, entry) pairs.  k_rtable_lookup<S>: one board per
    lane, 4,096 waves, through rows= into the table of the 128 levels built on the GPU: on states of R, on random placements, on
    the targets, in FULL rows and outside the table."""
    S = cases.REACH_CASES[name][0] if name in cases.REACH_CASES else cases.RTABLE_CASES[name][0]
    start = time.perf_counter()
    if name in cases.REACH_CASES:
        _occupancy_reach(S)
    elif "build" in name:
        _occupancy_build(S)
    else:
        _occupancy_lookup(S)
    print(f"{name}: {time.perf_counter() - start:.1f} s")


# ---------------------------------------------------------------------------------------------------- tens of thousands of states
BIG_CAPACITY = 65536
BIG = ((4, 6, 2), (6, 5, 6))   # size, tiles, obstacles: seeds 0 .. 7, targets where 14 moves leave the tiles


@functools.lru_cache(maxsize=None)
def _big_levels(S, T, K):
    orc = _oracle()
    blk, init, _ = orc.generate_mt19937(S, T, T, K, np.arange(8, dtype=np.uint32))
    return blk, init, cases.walked(orc, S, blk, init, 14)


def _every_state(ref):
    """(level, pos): a board on every state of every level's R."""
    n = len(ref.count)
    level = np.repeat(np.arange(n), np.maximum(ref.count, 0))
    return level, np.ascontiguousarray(np.concatenate([ref.cells(i) for i in range(n)], axis=1))


def _looked_up(S, mc, blk, init, tgt, ref, rtab, level, pos, ctx):
    import rtable_reference as rt
    b, i, t = (np.ascontiguousarray(a[:, level]) for a in (blk, init, tgt))
    want = rt.lookup(_oracle(), ref, b, t, pos, rows=level)
    env = _env(S, mc, b, i, t, pos=pos)
    for name, g, w in zip(("moves", "best", "action"), _raw_lookup(env, rtab, level, want), want):
        np.testing.assert_array_equal(g, w, err_msg=f"{name}: {ctx}")
    env.close()
    return want


@pytest.mark.parametrize("mc", (False, True))
@pytest.mark.parametrize("S,T,K", BIG)
def test_reachable_sets_of_tens_of_thousands_of_states(torch_cuda, oracle, S, T, K, mc):
    """Capacity 65,536 - rows of 2^17 slots, a log beyond 4,096 entries, frontiers of thousands of states dealt over 256 lanes,
    phase 2 over tens of thousands of successor entries: eight levels built, their pair sets, a lookup on every state of every R,
    and ts_reach_solve on the roots with the same capacity.  Then the largest level alone: capacity |R| holds it, |R| - 1 is FULL,
    and the hashed solver at |R| - 1 still reports the win it finds before the count passes the budget."""
    import reach_reference as reach
    import rtable_reference as rt
    start = time.perf_counter()
    orc = _oracle()
    blk, init, tgt = _big_levels(S, T, K)
    ref = rt.build(orc, S, mc, blk, tgt, init, 252, BIG_CAPACITY)
    finite, none = int(((ref.entry >= 1) & (ref.entry <= 252)).sum()), int((ref.entry == rt.NONE).sum())
    print(f"{S}x{S} T={T} K={K} mc={mc}: |R| {sorted(ref.count.tolist())}, deepest {ref.deepest.max()}, entries >= 1 {finite}, NONE {none}, root moves {ref.root_moves.tolist()}")
    assert (ref.count >= 5000).sum() >= 6 and (ref.count > 0).all() and ref.count.max() > 2 * 4096 and finite >= 1000
    env = _env(S, mc, blk, init, tgt)
    rtab = _raw_build(env, ref, 252, BIG_CAPACITY)
    assert rtab.slots == 1 << 17
    _same_outputs(rtab, ref, (S, T, mc))
    _same_pairs(rtab, ref, np.arange(8), (S, T, mc))
    level, pos = _every_state(ref)
    want = _looked_up(S, mc, blk, init, tgt, ref, rtab, level, pos, (S, T, mc, "every state"))
    assert len(level) == ref.count.sum() >= 50000 and (want[0] != rt.SOLVE_ABSENT).all()
    solved = reach.solve(orc, S, mc, blk, tgt, init, 64, BIG_CAPACITY)
    can = ref.root_moves >= 1   # the two yardsticks agree on the roots that can be won
    np.testing.assert_array_equal(solved[0][can], np.where(ref.root_moves[can] <= 64, ref.root_moves[can], reach.SOLVE_DEPTH))
    print(f"    ts_reach_solve: moves {solved[0].tolist()}, states {solved[2].tolist()}")
    _same(_raw(env, 64, BIG_CAPACITY, solved), solved, (S, T, mc, "the roots"))
    env.close()
    # the same roots with every target on one cell: no board can be won, the search expands all it reaches or runs out of the budget
    never = np.ascontiguousarray(np.repeat(tgt[:1], T, axis=0))
    whole = reach.solve(orc, S, mc, blk, never, init, 32767, BIG_CAPACITY)
    print(f"    ts_reach_solve on copies that cannot be won: moves {whole[0].tolist()}, states {whole[2].tolist()}")
    assert np.isin(whole[0], (reach.SOLVE_NONE, reach.SOLVE_FULL)).all() and (whole[2] >= 5000).sum() >= 6
    env = _env(S, mc, blk, init, never)
    _same(_raw(env, 32767, BIG_CAPACITY, whole), whole, (S, T, mc, "copies that cannot be won"))
    env.close()
    # the largest level alone, at the edge of its budget
    i = int(np.argmax(ref.count))
    R = int(ref.count[i])
    one = lambda a: np.ascontiguousarray(a[:, i:i + 1])
    env = _env(S, mc, one(blk), one(init), one(tgt))
    for cap in (R, R - 1):
        edge = rt.build(orc, S, mc, one(blk), one(tgt), one(init), 252, cap)
        assert edge.count.tolist() == [R if cap == R else rt.SOLVE_FULL]
        rtab = _raw_build(env, edge, 252, cap)
        _same_outputs(rtab, edge, (S, T, mc, i, cap))
        _same_pairs(rtab, edge, np.arange(1), (S, T, mc, i, cap))
        won = reach.solve(orc, S, mc, one(blk), one(tgt), one(init), 64, cap)
        _same(_raw(env, 64, cap, won), won, (S, T, mc, i, cap, "ts_reach_solve"))
    assert won[0].tolist() == [ref.root_moves[i]] or won[0].tolist() == [reach.SOLVE_FULL]
    print(f"    level {i} with |R| = {R}: at capacity |R| - 1 the table is FULL, ts_reach_solve answers {won[0].tolist()} after {won[2].tolist()} states")
    env.close()
    print(f"    {time.perf_counter() - start:.1f} s")


# ---------------------------------------------------------------------------------------------------- the probe at its edges
EDGE_SIZES = (5, 7, 8)
EDGE_CAPACITY = 4096   # the levels of up to so many states are looked at


def _home(keys, slots):
    """home(key) of include/tiler_slider_rtable.h restated: the multiplicative hash's bits 32 .. 63, their top log2(slots) bits."""
    h = (keys.astype(np.uint64) * np.uint64(0x9e3779b97f4a7c15)) >> np.uint64(32)
    return (h >> np.uint64(32 - (slots.bit_length() - 1))).astype(np.int64)


def _slots(capacity):
    return 1 << max(1, (2 * capacity - 1).bit_length())


@functools.lru_cache(maxsize=None)
def _edge_picks(S, mc):
    """(wrapped, full_load): levels of the case whose row, at capacity |R|, must hold a state whose probe wrapped past the end of
    the row - for some k <= 64 more than k keys have their home in the last k slots -, and levels at load exactly 0.5 (|R| a power
    of two) with the three of the highest load among those of 200 states and more.  From the yardstick's keys alone."""
    whole = _yard_rtable(S, mc, "init", 252, EDGE_CAPACITY)
    wrapped, pow2, load = [], [], []
    for l in range(cases.DISTINCT):
        R = int(whole.count[l])
        if R < 2:
            continue
        slots = _slots(R)
        home = _home(whole.keys(l), slots)
        if any((home >= slots - k).sum() > k for k in range(1, 65)):
            wrapped.append(l)
        if R & (R - 1) == 0:
            pow2.append(l)
        elif R >= 200:
            load.append((R / slots, l))
    return tuple(wrapped), tuple(pow2 + [l for _, l in sorted(load)[-3:]])


@pytest.mark.parametrize("mc", (False, True))
@pytest.mark.parametrize("S", EDGE_SIZES)
def test_probes_that_wrap_and_rows_at_full_load(torch_cuda, oracle, S, mc):
    """Each picked level in a one-level call of its own at capacity |R|: outputs, the pair set, a lookup on every state and on 256
    placements the row does not hold; and ts_reach_solve with the same capacity on a copy of the level that cannot be won - every
    target on one cell - which expands exactly its reachable set and ends SOLVE_NONE."""
    import reach_reference as reach
    import rtable_reference as rt
    start = time.perf_counter()
    orc = _oracle()
    every = {(s, m): _edge_picks(s, m) for s in EDGE_SIZES for m in (False, True)}
    for m in (False, True):
        assert sum(len(every[s, m][0]) for s in EDGE_SIZES) >= 3, "too few levels whose probes must wrap"
    wrapped, loaded = every[S, mc]
    whole = _yard_rtable(S, mc, "init", 252, EDGE_CAPACITY)
    sizes = lambda ls: [int(whole.count[l]) for l in ls]
    print(f"{S}x{S} mc={mc}: wrapped probes in levels {list(wrapped)} of {sizes(wrapped)} states; full load in levels {list(loaded)} of {sizes(loaded)} states, "
          f"load {[round(int(whole.count[l]) / _slots(int(whole.count[l])), 3) for l in loaded]}")
    assert any(r & (r - 1) == 0 for r in sizes(loaded)) and len(loaded) >= 4
    blk, init, tgt = _levels(S, mc)
    T = init.shape[0]
    rng = np.random.default_rng(0xED6E + S)
    same_set = 0
    for l in sorted(set(wrapped + loaded)):
        R = int(whole.count[l])
        one = lambda a: np.ascontiguousarray(a[:, l:l + 1])
        ref = rt.build(orc, S, mc, one(blk), one(tgt), one(init), 252, R)
        assert ref.count.tolist() == [R]
        np.testing.assert_array_equal(ref.keys(0), whole.keys(l))
        env = _env(S, mc, one(blk), one(init), one(tgt))
        rtab = _raw_build(env, ref, 252, R)
        assert rtab.slots == _slots(R)
        _same_outputs(rtab, ref, (S, mc, l, R))
        _same_pairs(rtab, ref, np.arange(1), (S, mc, l, R))
        off = _random_placements(rng, S, T, blk, l, 2048)
        off = off[:, ~np.isin(rt.keys_of(S, off), ref.keys(0))][:, :256]
        assert off.shape[1] == 256
        pos = np.ascontiguousarray(np.concatenate([ref.cells(0), off], axis=1))
        want = _looked_up(S, mc, one(blk), one(init), one(tgt), ref, rtab, np.zeros(pos.shape[1], np.int64), pos, (S, mc, l, R))
        absent = (want[0][R:] == rt.SOLVE_ABSENT).sum()
        assert (want[0][:R] != rt.SOLVE_ABSENT).all() and absent + (want[0][R:] == 0).sum() == 256 and absent >= 128
        env.close()
        # the copy that cannot be won: its reachable set holds R, and is R where no state of the level itself is next to a win -
        # then the search fills the same row with the same keys and ends NONE; else it runs out of this budget
        never = np.ascontiguousarray(np.repeat(one(tgt)[:1], T, axis=0))
        want = reach.solve(orc, S, mc, one(blk), never, one(init), 32767, R)
        assert want[0].tolist() in ([reach.SOLVE_NONE], [reach.SOLVE_FULL]) and (want[0][0] == reach.SOLVE_FULL or want[2].tolist() == [R])
        same_set += int(want[0][0] == reach.SOLVE_NONE)
        env = _env(S, mc, one(blk), one(init), never)
        _same(_raw(env, 32767, R, want), want, (S, mc, l, "the copy that cannot be won"))
        env.close()
    print(f"    {len(set(wrapped + loaded))} levels, ts_reach_solve ends SOLVE_NONE with |R| states in {same_set} of them; {time.perf_counter() - start:.1f} s")
    assert same_set >= 3
