"""ts_rtable_build and ts_rtable_lookup on the GPU against the CPU yardstick (tests/rtable_reference.py: the closure over the oracle
with sorted keys, the distances by rounds over searchsorted successors) and, on shapes both take, against ts_table_lookup on a
complete dense table and ts_reach_solve.  Exact equality everywhere.  Three things together show that a level's stored set is
exactly right: .entries() equals the yardstick's sorted (key, entry) pairs; count, root_moves and deepest equal the yardstick's;
boards placed on every state of R look up the yardstick's moves, best and action.  The raw C-ABI calls write into buffers between
guard bytes - outputs prefilled with the complement of the yardstick's answer, table and workspace with 0xA5, never zeroed."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAPACITY = 4096
N_SEEDS = 64
# size, tiles, obstacles, multi colour: shapes the dense tables refuse; the reference's random levels of seeds 0 .. 63
BEYOND = ((5, 4, 3, True), (5, 4, 3, False), (8, 3, 10, False), (7, 3, 8, False))
# size, tiles, obstacles, multi colour, walk length, boards: levels whose targets are where a random walk left the tiles
WALKED = ((5, 4, 3, True, 12, 64), (8, 8, 30, True, 10, 16))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _oracle():
    from oracle import binding
    return binding


def _seeded(S, T, K, n=N_SEEDS):
    from test_gpu_reach import _seeded as seeded
    return seeded(S, T, K, n)


def _walked(S, T, K, L, n):
    from test_gpu_reach import _walked as walked
    return walked(S, T, K, L, n)


@functools.lru_cache(maxsize=None)
def _yard_seeded(S, T, K, mc, n=N_SEEDS, max_depth=252, capacity=CAPACITY):
    """The yardstick's Reference of the seeded levels, computed once.  Do not write to it."""
    import rtable_reference as rt
    blk, init, tgt = _seeded(S, T, K, n)
    return rt.build(_oracle(), S, mc, blk, tgt, init, max_depth, capacity)


@functools.lru_cache(maxsize=None)
def _yard_walked(S, T, K, mc, L, n, max_depth=252, capacity=CAPACITY):
    import rtable_reference as rt
    blk, init, tgt = _walked(S, T, K, L, n)
    return rt.build(_oracle(), S, mc, blk, tgt, init, max_depth, capacity)


def _env(S, mc, blk, init, tgt, pos=None, **kw):
    import torch
    from tiler_slider_amd import VecTilerSliderEnv
    env = VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=mc, obs_dtype=None, **kw)
    env.reset()
    if pos is not None:
        env._pos.copy_(torch.from_numpy(np.ascontiguousarray(pos)).to(env._pos.device))
    return env


def _raw_build(env, ref=None, max_depth=252, capacity=CAPACITY, root="init", ask=(True, True), in_flight=None, stream=None):
    """ts_rtable_build through the C-ABI -> a ReachTable whose tensors are views of buffers the test owns.  Table: between guard
    bytes, prefilled with 0xA5.  count, root_moves, deepest: between guard bytes, prefilled with the bytewise complement of the
    yardstick's answer `ref` where the caller has it - an entry the kernel skips then differs by construction - else with 77.
    `ask` = (root_moves, deepest): an output not asked for is passed as NULL and its buffer must keep its fill.  Workspace:
    `in_flight` slices (default: as many as the library would use of 1 GiB) between guard bytes, prefilled with 0xA5."""
    import torch
    from table_harness import GUARD, guarded, payload
    from tiler_slider_amd import ReachTable, _rtable_cabi as xc
    n = env.num_envs
    slots = xc.slots(capacity)
    dts = (np.int32, np.int16, np.int32)
    want = None if ref is None else (ref.count, ref.root_moves, ref.deepest)
    fills = [np.full(n, 77, dt) if want is None else ~np.asarray(want[i]).astype(dt) for i, dt in enumerate(dts)]
    bufs = [guarded(torch, env.device, f) for f in fills]
    tbuf = torch.full((2 * GUARD + n * slots * 8,), 0xA5, dtype=torch.uint8, device=env.device)
    per_level = xc.workspace_bytes(env._dims, capacity, 1)
    if in_flight is None:
        in_flight = xc.describe_rtable_build(env._dims, max_depth, capacity)["levels_in_flight"]
    ws = torch.full((2 * GUARD + in_flight * per_level,), 0xA5, dtype=torch.uint8, device=env.device)
    assert (ws.data_ptr() + GUARD) % 8 == 0 and (tbuf.data_ptr() + GUARD) % 8 == 0
    cfg = xc.RtableCfg(int(max_depth), int(capacity), xc.ROOTS[root], ws.data_ptr() + GUARD, in_flight * per_level)
    d = xc.describe_rtable_build(env._dims, max_depth, capacity, in_flight * per_level, xc.ROOTS[root])
    assert d["blocks"] == d["levels_in_flight"] == min(n, in_flight, 1024) and d["name"] == f"k_rtable_build<{env.size}>"
    assert d["slots"] == slots and d["table_bytes"] == 8 * slots and d["workspace_bytes"] == per_level
    ptr = lambda i: bufs[i].data_ptr() + GUARD
    out = xc.RtableOut(tbuf.data_ptr() + GUARD, ptr(0), ptr(1) if ask[0] else None, ptr(2) if ask[1] else None)
    s = torch.cuda.current_stream(env.device) if stream is None else stream
    code = xc.lib().ts_rtable_build(C.byref(env._dims), C.byref(env._state), C.byref(cfg), C.byref(out), s.cuda_stream)
    assert code == 0, code
    s.synchronize()
    for name, b in (("workspace", ws), ("table", tbuf)):
        assert bool((b[:GUARD] == 0xA5).all()) and bool((b[b.numel() - GUARD:] == 0xA5).all()), f"a guard byte of the {name} was overwritten"
    got = [payload(b, dt, (n,)) for b, dt in zip(bufs, dts)]
    for i, asked in ((1, ask[0]), (2, ask[1])):
        if not asked:
            np.testing.assert_array_equal(got[i], fills[i], err_msg="an output that was not asked for was written")
    view = lambda i, dt: bufs[i][GUARD:bufs[i].numel() - GUARD].view(dt)
    table = tbuf[GUARD:tbuf.numel() - GUARD].view(torch.int64).view(n, slots)
    rtab = ReachTable(table, view(0, torch.int32), view(1, torch.int16) if ask[0] else None, view(2, torch.int32) if ask[1] else None, capacity,
                      env.size, env.n_tiles, env.n_targets, env.multi_color, max_depth, root)
    rtab._keep = (tbuf, bufs)
    return rtab


def _raw_lookup(env, rtab, rows=None, want=None, ask=(True, True, True), stream=None):
    """ts_rtable_lookup through the C-ABI: (moves, best, action), each between guard bytes, prefilled with the complement of `want`."""
    import torch
    from table_harness import GUARD, guarded, payload
    from tiler_slider_amd import _rtable_cabi as xc
    n = env.num_envs
    dts = (np.int16, np.uint8, np.uint8)
    fills = [np.full(n, 77, dt) if want is None else ~np.asarray(want[i]).astype(dt) for i, dt in enumerate(dts)]
    bufs = [guarded(torch, env.device, f) for f in fills]
    r = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(env.device)
    s = torch.cuda.current_stream(env.device) if stream is None else stream
    ptr = lambda i: bufs[i].data_ptr() + GUARD if ask[i] else None
    code = xc.lib().ts_rtable_lookup(C.byref(env._dims), C.byref(env._state), rtab.table.data_ptr(), rtab.slots, rtab.count.data_ptr(), len(rtab),
                                     None if r is None else r.data_ptr(), ptr(0), ptr(1), ptr(2), s.cuda_stream)
    assert code == 0, code
    s.synchronize()
    got = [payload(b, dt, (n,)) for b, dt in zip(bufs, dts)]
    for i in range(3):
        if not ask[i]:
            np.testing.assert_array_equal(got[i], fills[i], err_msg="an output that was not asked for was written")
    return tuple(got)


def _same_outputs(rtab, ref, ctx):
    for name, g, w in (("count", rtab.count, ref.count), ("root_moves", rtab.root_moves, ref.root_moves), ("deepest", rtab.deepest, ref.deepest)):
        if g is not None:
            np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=f"{name}: {ctx}")


def _same_entries(rtab, ref, ctx):
    """.entries() of every level equals the yardstick's sorted (key, entry) pairs; a FULL level gives none."""
    for lv in range(len(ref.count)):
        keys, entries = rtab.entries(lv)
        np.testing.assert_array_equal(keys.cpu().numpy(), ref.keys(lv), err_msg=f"keys of level {lv}: {ctx}")
        np.testing.assert_array_equal(entries.cpu().numpy(), ref.entries(lv), err_msg=f"entries of level {lv}: {ctx}")
    # an occupied slot is bit 63, an entry byte and a 48-bit key, every other slot is 0 (a FULL row: whatever it holds)
    t = rtab.table[rtab.count >= 0]
    assert bool(((t == 0) | ((t >> 56) == -128)).all()), ctx


def _boards(ref, blk, init, tgt):
    """(level, pos) of the boards a level is asked about: one on every state of its R, and one on its root - the only board of a
    level that is won as it stands or FULL."""
    n = len(ref.count)
    held = np.maximum(ref.count, 0)
    lv = np.concatenate([np.repeat(np.arange(n), held), np.arange(n)])
    C = ref.S * ref.S
    pos = np.concatenate([ref.cells(i) for i in range(n)] + [np.minimum(init, C - 1).astype(ref.cell_dtype)], axis=1)
    return lv, np.ascontiguousarray(pos)


def _same_lookups(rtab, ref, S, mc, blk, init, tgt, ctx, extra=None):
    """Boards on every state of R (and the roots; `extra` = (level, pos) adds more) look up the yardstick's answer through rows=."""
    import rtable_reference as rt
    lv, pos = _boards(ref, blk, init, tgt)
    if extra is not None:
        lv, pos = np.concatenate([lv, extra[0]]), np.ascontiguousarray(np.concatenate([pos, extra[1]], axis=1))
    b, i, t = (np.ascontiguousarray(a[:, lv]) for a in (blk, init, tgt))
    want = rt.lookup(_oracle(), ref, b, t, pos, rows=lv)
    env = _env(S, mc, b, i, t, pos=pos)
    got = _raw_lookup(env, rtab, lv, want)
    for name, g, w in zip(("moves", "best", "action"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{name}: {ctx}")
    return env, lv, want


def _check(S, mc, blk, init, tgt, ref, ctx, **build):
    rtab = _raw_build(_env(S, mc, blk, init, tgt), ref, **build)
    _same_outputs(rtab, ref, ctx)
    _same_entries(rtab, ref, ctx)
    return rtab, _same_lookups(rtab, ref, S, mc, blk, init, tgt, ctx)


# ---------------------------------------------------------------------------------------------------- against the existing libraries
@pytest.mark.parametrize("S,T,K,mc,n", ((4, 2, 2, False, 64), (4, 2, 2, True, 64), (3, 4, 1, False, 32), (4, 4, 2, True, 8),
                                         (3, 5, 1, False, 64), (3, 5, 1, True, 64)))
def test_equals_the_dense_table_and_the_hashed_solver_where_all_apply(torch_cuda, S, T, K, mc, n):
    """capacity = the index space: never FULL.  Every state of R reads what ts_table_lookup reads from a complete build_table(),
    and root_moves is ts_reach_solve's moves.  3x3 with five tiles is the one shape the dense tables take whose keys split into two
    halves, by a division that is no shift."""
    import rtable_reference as rt
    from test_gpu_reach import _drawn
    from tiler_slider_amd import TABLE_MAX_DEPTH
    torch = torch_cuda
    blk, init, tgt = _drawn(S, T, K, mc, n)
    space = (S * S) ** T
    ref = rt.build(_oracle(), S, mc, blk, tgt, init, 252, space)
    assert (ref.count >= 0).all() and (ref.count > 1).sum() >= n // 2
    rtab, (boards, lv, want) = _check(S, mc, blk, init, tgt, ref, (S, T, mc), capacity=space)
    dense = _env(S, mc, blk, init, tgt).build_table()
    assert bool(dense.complete.all())
    rows = torch.from_numpy(lv.astype(np.int32))
    moves, bits = boards.lookup_bits(dense, rows=rows)
    np.testing.assert_array_equal(moves.cpu().numpy(), want[0])
    np.testing.assert_array_equal(bits.cpu().numpy(), want[1])
    np.testing.assert_array_equal(boards.expert_actions_from(dense, rows=rows).cpu().numpy(), want[2])
    solved = _env(S, mc, blk, init, tgt).solve_reachable(max_depth=TABLE_MAX_DEPTH, capacity=space)
    np.testing.assert_array_equal(solved.moves.cpu().numpy(), ref.root_moves)


def test_equals_the_dense_table_on_the_smallest_boards(torch_cuda, oracle):
    """1x1 - the tile sits on its target, or there is none to sit on - and boards without tiles: one state, or none."""
    import rtable_reference as rt
    one = (np.zeros((1, 2), np.uint32), np.zeros((1, 2), np.uint8))
    cases = [(1, one[0], one[1], tgt) for tgt in (np.zeros((1, 2), np.uint8), np.zeros((0, 2), np.uint8))]
    for S, level in ((3, ([(1, 1)], [], [])), (3, ([(1, 1)], [], [(0, 0)])), (8, ([], [], [])), (8, ([(7, 7)], [], [(3, 3), (3, 3)]))):
        cases.append((S,) + tuple(oracle.pack_levels(S, [level])))
    for S, blk, init, tgt in cases:
        for mc in (False, True):
            ref = rt.build(oracle, S, mc, blk, tgt, init, 252, 1)
            assert set(ref.count.tolist()) <= {0, 1} and set(ref.root_moves.tolist()) <= {0, rt.SOLVE_NONE}
            env = _env(S, mc, blk, init, tgt)
            rtab, _ = _check(S, mc, blk, init, tgt, ref, (S, mc, tgt.shape), capacity=1)
            moves, bits = env.lookup_bits(env.build_table())
            got = _raw_lookup(env, rtab)
            np.testing.assert_array_equal(got[0], moves.cpu().numpy())
            np.testing.assert_array_equal(got[1], bits.cpu().numpy())
            np.testing.assert_array_equal(env.solve_reachable(252, 1).moves.cpu().numpy(), ref.root_moves)


# ---------------------------------------------------------------------------------------------------- beyond the dense tables
@pytest.mark.parametrize("S,T,K,mc", BEYOND)
def test_random_levels_beyond_the_index_space_of_the_dense_tables(torch_cuda, S, T, K, mc):
    import rtable_reference as rt
    from tiler_slider_amd import VecTilerSliderEnv, _table_cabi
    ref = _yard_seeded(S, T, K, mc)
    # properties of the YARDSTICK's answer: no level runs out of its budget, the sets are large, and a root can be won here and
    # there (none of the 7x7 ones), with hundreds of states a finite distance from the win
    assert (ref.count != rt.SOLVE_FULL).all() and ref.count.max() >= 1000 and (S == 7 or ((ref.root_moves >= 1).sum() >= 1 and (ref.entry <= 252).sum() >= 500))
    env = VecTilerSliderEnv.from_seeds(np.arange(N_SEEDS), size=S, num_tiles=T, num_obstacles=K, multi_color=mc, obs_dtype=None)
    assert _table_cabi.table_states(env._dims) == 0
    blk, init, tgt = _seeded(S, T, K)
    np.testing.assert_array_equal(env._init.cpu().numpy(), init)
    print(f"{S}x{S} T={T} K={K} mc={mc}: largest {ref.count.max()}, mean {ref.count.mean():.0f}, deepest {ref.deepest.max()}, can be won {(ref.root_moves >= 1).sum()}")
    _check(S, mc, blk, init, tgt, ref, (S, T, K, mc))


@pytest.mark.parametrize("S,T,K,mc,L,n", WALKED)
def test_walked_levels_with_long_keys_and_full_levels(torch_cuda, S, T, K, mc, L, n):
    """Targets where a random walk left the tiles: the roots can be won, the distances are spread; at 8x8 with 8 tiles the keys run
    up to 2^48 and most levels reach more than the budget."""
    import rtable_reference as rt
    ref = _yard_walked(S, T, K, mc, L, n)
    full = ref.count == rt.SOLVE_FULL
    if T == 8:
        # (of the 16 levels 9 are FULL, 4 are won as they stand - the walk moved nothing - and 3 hold 102, 289 and 353 states)
        assert (ref.count >= 100).sum() >= 3 and full.sum() >= 4 and ref.idx.max() >= 1 << 44
    else:
        assert not full.any() and ref.count.max() <= 3360 and (ref.root_moves >= 1).all() and len(set(ref.root_moves.tolist())) >= 3
    every = [_yard_walked(*case) for case in WALKED]
    assert sum(int((r.count >= 100).sum()) for r in every) >= 4 and sum(int((r.count == rt.SOLVE_FULL).sum()) for r in every) >= 4
    blk, init, tgt = _walked(S, T, K, L, n)
    print(f"{S}x{S} T={T} K={K} walk {L}: counts {sorted(ref.count.tolist())}, deepest {ref.deepest.max()}")
    _check(S, mc, blk, init, tgt, ref, (S, T, K, mc, L))


def test_the_edge_of_the_budget(torch_cuda):
    """Three levels of 5x5 / 4 tiles with |R| = R: capacity R holds them, capacity R - 1 is FULL; capacities 1, 2 and 3 are tables
    of 2, 4 and 8 slots, where every probe sequence wraps around."""
    import rtable_reference as rt
    S, T, K, mc = BEYOND[0]
    whole = _yard_seeded(S, T, K, mc)
    order = np.argsort(whole.count, kind="stable")
    order = order[whole.count[order] > 8]
    picks = order[[0, len(order) // 2, -1]]
    blk, init, tgt = _seeded(S, T, K)
    for i in picks:
        R = int(whole.count[i])
        one = lambda a: np.ascontiguousarray(a[:, i:i + 1])
        for cap in (R, R - 1, 1, 2, 3):
            ref = rt.build(_oracle(), S, mc, one(blk), one(tgt), one(init), 252, cap)
            assert ref.count.tolist() == [R if cap == R else rt.SOLVE_FULL] and ref.root_moves.tolist() == ([whole.root_moves[i]] if cap == R else [rt.SOLVE_FULL])
            _check(S, mc, one(blk), one(init), one(tgt), ref, (int(i), R, cap), capacity=cap)


@pytest.mark.parametrize("depth", (0, 3, 7))
def test_max_depth_cuts_the_rounds(torch_cuda, depth):
    """What lies within `depth` rounds keeps its distance; the rest is DEEP, or NONE where a round up to `depth` resolved nothing."""
    import rtable_reference as rt
    deep = none = 0
    for case in (WALKED[0], BEYOND[2]):
        S, T, K, mc = case[:4]
        blk, init, tgt = _walked(*case[:3], *case[4:]) if len(case) == 6 else _seeded(S, T, K)
        whole = (_yard_walked if len(case) == 6 else _yard_seeded)(*case)
        ref = (_yard_walked if len(case) == 6 else _yard_seeded)(*case, max_depth=depth)
        near = (whole.entry >= 1) & (whole.entry <= depth)
        np.testing.assert_array_equal(ref.entry[near], whole.entry[near])
        assert np.isin(ref.entry[~near], (rt.DEEP, rt.NONE)).all() and (ref.deepest <= depth).all()
        deep, none = deep + int((ref.entry == rt.DEEP).sum()), none + int((ref.entry == rt.NONE).sum())
        _check(S, mc, blk, init, tgt, ref, (case, depth), max_depth=depth)
    assert deep >= 100 and (none >= 100 if depth else none == 0)   # without a round nothing is found to be NONE


def test_the_deep_rounds(torch_cuda, oracle):
    """The five levels of tests/golden/deep_levels.npz, rooted (root="pos") on a placement at the level's deepest distance, 37 to 106
    moves from the win: root_moves is that distance, and so is deepest."""
    import deep_cases
    import rtable_reference as rt
    seen = []
    for lv in deep_cases.levels().values():
        dist = deep_cases.exact(oracle, lv)
        far = deep_cases.deepest(dist)
        start = deep_cases.cells_of(lv, np.flatnonzero(dist == far)[:1])
        ref = rt.build(oracle, lv.S, lv.mc, lv.blk, lv.tgt, start)
        assert ref.root_moves.tolist() == [far] == ref.deepest.tolist() == [lv.deepest] and ref.count[0] > far
        seen.append(far)
        env = _env(lv.S, lv.mc, lv.blk, lv.init, lv.tgt, pos=start)
        rtab = _raw_build(env, ref, root="pos", capacity=1 << 14)
        _same_outputs(rtab, ref, lv.name)
        _same_entries(rtab, ref, lv.name)
        _same_lookups(rtab, ref, lv.S, lv.mc, lv.blk, start, lv.tgt, lv.name)
    assert len(seen) == 5 and min(seen) == 37 and max(seen) == 106


def test_absent_placements_and_rows(torch_cuda, oracle):
    """Placements the dense table calls valid, some of them winnable, that play from the root never reaches: SOLVE_ABSENT, 0, 255.
    And rows=: boards in any order, several per level, rows outside the table -> SOLVE_NONE, 0, 255 whatever the board."""
    import rtable_reference as rt
    import table_reference as dense
    S, T, K, mc, n = 4, 4, 2, True, 8
    blk, init, tgt = _walked(S, T, K, 12, n)
    ref = rt.build(oracle, S, mc, blk, tgt, init)
    exact = dense.exact(oracle, S, mc, blk, tgt, T)
    lv, idx = [], []
    for i in range(n):
        valid = np.flatnonzero(exact[i] > 0)                                    # a placement, and not won
        off = np.setdiff1d(valid, ref.keys(i))
        off = off[::off.size // 200][:200]
        assert off.size == 200 and (exact[i, off] < dense.UNREACHABLE).sum() >= 40   # most of them can be won: the dense table says how
        lv.append(np.full(off.size, i)), idx.append(off)
    lv, idx = np.concatenate(lv), np.concatenate(idx)
    pos = rt.cells_of(S, T, idx, init.dtype)
    rtab = _raw_build(_env(S, mc, blk, init, tgt), ref)
    env, rows, want = _same_lookups(rtab, ref, S, mc, blk, init, tgt, "absent placements", extra=(lv, pos))
    tail = slice(len(rows) - len(lv), None)
    assert (want[0][tail] == rt.SOLVE_ABSENT).all() and (want[1][tail] == 0).all() and (want[2][tail] == 255).all()
    # rows out of range, on the same boards: every fifth board
    bad = rows.astype(np.int64).copy()
    bad[::5] = np.resize(np.array([-1, n, n + 1, 2**31 - 1, -2**31]), len(bad[::5]))
    want = rt.lookup(oracle, ref, np.ascontiguousarray(blk[:, rows]), np.ascontiguousarray(tgt[:, rows]), env._pos.cpu().numpy(), rows=bad)
    assert (want[0][::5] == rt.SOLVE_NONE).all() and (want[2][::5] == 255).all()
    got = _raw_lookup(env, rtab, bad.astype(np.int32), want)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    # an empty table: every row is out of range, and neither table nor count is read
    from tiler_slider_amd import _rtable_cabi as xc
    none = np.full(env.num_envs, 77, np.int16)
    out = torch_cuda.from_numpy(none.copy()).to(env.device)
    code = xc.lib().ts_rtable_lookup(C.byref(env._dims), C.byref(env._state), None, rtab.slots, None, 0, None, out.data_ptr(), None, None,
                                     torch_cuda.cuda.current_stream(env.device).cuda_stream)
    assert code == 0 and (out.cpu().numpy() == rt.SOLVE_NONE).all()


def test_a_table_written_by_the_header_alone_and_rows_of_arbitrary_bytes(torch_cuda):
    """A lookup is a probe by anyone: rows filled on the host from the yardstick's pairs by the header's format - bit 63, the entry,
    the key, the multiplicative hash, linear probing - are read like rows the build wrote.  And rows nobody wrote: all zero, and
    all 0xA5 - every slot occupied by a key no board has, so every probe walks the whole row and ends - answer SOLVE_ABSENT."""
    import rtable_reference as rt
    from tiler_slider_amd import ReachTable
    torch = torch_cuda
    S, T, K, mc = BEYOND[0]
    n, capacity = 8, CAPACITY
    whole = _yard_seeded(S, T, K, mc)
    blk, init, tgt = (np.ascontiguousarray(a[:, :n]) for a in _seeded(S, T, K))
    ref = rt.build(_oracle(), S, mc, blk, tgt, init, 252, capacity)
    np.testing.assert_array_equal(ref.count, whole.count[:n])
    slots = 1 << (2 * capacity - 1).bit_length()
    shift = 64 - (slots.bit_length() - 1)
    rows = np.zeros((n, slots), np.uint64)
    for lv in range(n):
        for key, entry in zip(ref.keys(lv).tolist()[::-1], ref.entries(lv).tolist()[::-1]):   # any order of insertion gives a valid row
            slot = ((key * 0x9e3779b97f4a7c15) & ((1 << 64) - 1)) >> shift
            while rows[lv, slot]:
                slot = (slot + 1) % slots
            rows[lv, slot] = (1 << 63) | (entry << 48) | key
    env = _env(S, mc, blk, init, tgt)
    made = lambda table, count: ReachTable(table.to(env.device), count.to(env.device), None, None, capacity, S, T, T, mc, 252, "init")
    by_hand = made(torch.from_numpy(rows.view(np.int64)), torch.from_numpy(ref.count))
    _same_entries(by_hand, ref, "a table written by the header alone")
    _same_lookups(by_hand, ref, S, mc, blk, init, tgt, "a table written by the header alone")
    for byte in (0x00, 0xA5):
        nobody = made(torch.full((n, slots), byte * 0x0101010101010101 - (1 << 64 if byte & 0x80 else 0), dtype=torch.int64),
                      torch.full((n,), byte * 0x01010101 - (1 << 32 if byte & 0x80 else 0), dtype=torch.int32))
        got = _raw_lookup(env, nobody)
        assert (got[0] == rt.SOLVE_ABSENT).all() and (got[1] == 0).all() and (got[2] == 255).all(), hex(byte)


def test_slices_are_reused_when_the_workspace_is_smaller_than_the_batch(torch_cuda):
    """257 levels through a workspace for 3 levels, and for 1: the results of 257 slices."""
    import rtable_reference as rt
    S, T, K, mc = BEYOND[0]
    ref = _yard_seeded(S, T, K, mc, 257)
    assert (ref.count != rt.SOLVE_FULL).all()
    blk, init, tgt = _seeded(S, T, K, 257)
    env = _env(S, mc, blk, init, tgt)
    for in_flight in (257, 3, 1):
        rtab = _raw_build(env, ref, in_flight=in_flight)
        _same_outputs(rtab, ref, f"{in_flight} levels in flight")
        _same_entries(rtab, ref, f"{in_flight} levels in flight")
    _same_lookups(rtab, ref, S, mc, blk, init, tgt, "one level in flight")


def test_targets_that_repeat_or_differ_in_number_and_cells_beyond_the_board(torch_cuda, oracle):
    """T != Tt (multi colour: never won; single colour: the sets of cells are compared), repeated targets, and cell ids >= S * S
    in the root and the targets, which read as S * S - 1: the yardstick clamps them."""
    import rtable_reference as rt
    S, T, K, n = 5, 4, 3, 24
    blk, init, tgt4 = (np.ascontiguousarray(a[:, :n]) for a in _walked(S, T, K, 12, 64))
    for mc in (False, True):
        for tgt in (np.concatenate([tgt4, tgt4[:1]]), tgt4[:3], np.repeat(tgt4[:1], 4, axis=0)):
            tgt = np.ascontiguousarray(tgt)
            ref = rt.build(oracle, S, mc, blk, tgt, init, 252, CAPACITY)
            _check(S, mc, blk, init, tgt, ref, (mc, tgt.shape))
        free = ((blk[0] >> 24) & 1) == 0                       # cell 24 holds no obstacle ...
        on24 = (init[:3] == 24).any(axis=0)                    # ... and no other tile
        edit = free & ~on24 & (np.arange(n) % 3 == 0)
        raw_init, raw_tgt = init.copy(), tgt4.copy()
        raw_init[3, edit] = 200
        raw_tgt[3, np.arange(n) % 4 == 0] = 255
        assert edit.sum() >= 3
        ref = rt.build(oracle, S, mc, blk, raw_tgt, raw_init, 252, CAPACITY)
        for root in ("init", "pos"):
            # reset() stores clamped cells: the ids beyond the board go in behind it, into the cells the root names
            env = _env(S, mc, blk, init, tgt4)
            (env._init if root == "init" else env._pos).copy_(torch_cuda.from_numpy(raw_init).to(env.device))
            env._tgt.copy_(torch_cuda.from_numpy(raw_tgt).to(env.device))
            rtab = _raw_build(env, ref, root=root)
            _same_outputs(rtab, ref, (mc, root, "ids beyond the board"))
            _same_entries(rtab, ref, (mc, root, "ids beyond the board"))
        _same_lookups(rtab, ref, S, mc, blk, raw_init, raw_tgt, (mc, "ids beyond the board"))


def test_two_builds_mid_episode_and_state_untouched(torch_cuda, oracle):
    """root="pos" after five random steps; a second build gives equal .entries() and equal lookups; no state byte changes, in the
    build or in the lookup; outputs that are not asked for keep their fill."""
    import rtable_reference as rt
    torch = torch_cuda
    S, T, K, mc, L, n = WALKED[0]
    blk, init, tgt = _walked(S, T, K, L, n)
    twin = oracle.OracleBatch(S, mc, 1000, blk, init, tgt)
    env = _env(S, mc, blk, init, tgt, max_steps=1000)
    twin.reset()
    for step in range(5):
        act = oracle.fill_actions(n, seed=0x27AB, step_index=step)
        env.step(torch.from_numpy(act))
        twin.step(act, obs=False)
    state = lambda: [t.clone() for t in (env._pos, env._step_count, env._done, env._init, env._tgt, env._blk)]
    before = state()
    ref = rt.build(oracle, S, mc, blk, tgt, twin.pos, 252, CAPACITY)
    first, second = _raw_build(env, ref, root="pos"), _raw_build(env, ref, root="pos")
    for ask in ((False, False), (True, False), (False, True)):
        _same_outputs(_raw_build(env, ref, root="pos", ask=ask), ref, ask)
    looked = []
    for rtab in (first, second):
        _same_outputs(rtab, ref, "mid episode")
        _same_entries(rtab, ref, "mid episode")
        want = rt.lookup(oracle, ref, blk, tgt, twin.pos)
        looked.append(_raw_lookup(env, rtab, None, want))
        for g, w in zip(looked[-1], want):
            np.testing.assert_array_equal(g, w)
        for ask in ((True, False, False), (False, True, False), (False, False, True)):
            got = _raw_lookup(env, rtab, None, want, ask=ask)
            np.testing.assert_array_equal(got[ask.index(True)], want[ask.index(True)])
    for lv in range(n):
        a, b = first.entries(lv), second.entries(lv)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for a, b in zip(before, state()):
        assert torch.equal(a, b)
    # the init-rooted table of the same boards is another table: where they stand now it answers as well, by the same definition
    at_start = _raw_build(env, _yard_walked(S, T, K, mc, L, n))
    want = rt.lookup(oracle, _yard_walked(S, T, K, mc, L, n), blk, tgt, twin.pos)
    for g, w in zip(_raw_lookup(env, at_start, None, want), want):
        np.testing.assert_array_equal(g, w)
    assert (want[0] != rt.SOLVE_ABSENT).all()   # they were reached by play from the root


def test_on_a_stream_of_its_own_behind_a_step(torch_cuda, oracle):
    """Both calls are asynchronous on THEIR stream: launched on a side stream that waits for the step, the build roots on the cells
    the step left and the lookup reads them."""
    import rtable_reference as rt
    torch = torch_cuda
    S, T, K, mc, L, n = WALKED[0]
    blk, init, tgt = _walked(S, T, K, L, n)
    env = _env(S, mc, blk, init, tgt)
    twin = oracle.OracleBatch(S, mc, 100, blk, init, tgt)
    twin.reset()
    act = oracle.fill_actions(n, seed=0x57EA, step_index=0)
    twin.step(act, obs=False)
    ref = rt.build(oracle, S, mc, blk, tgt, twin.pos, 252, CAPACITY)
    side = torch.cuda.Stream(env.device)
    env.step(torch.from_numpy(act))
    side.wait_stream(torch.cuda.current_stream(env.device))
    rtab = _raw_build(env, ref, root="pos", stream=side)
    _same_outputs(rtab, ref, "on a side stream")
    _same_entries(rtab, ref, "on a side stream")
    act = oracle.fill_actions(n, seed=0x57EA, step_index=1)
    twin.step(act, obs=False)
    want = rt.lookup(oracle, ref, blk, tgt, twin.pos)
    env.step(torch.from_numpy(act))
    side.wait_stream(torch.cuda.current_stream(env.device))
    for g, w in zip(_raw_lookup(env, rtab, None, want, stream=side), want):
        np.testing.assert_array_equal(g, w)


# ---------------------------------------------------------------------------------------------------- the Python path
def test_build_reach_table_and_the_expert_to_the_win_through_an_auto_reset(torch_cuda):
    """build_reach_table() against the yardstick - dtypes, shapes, .full, .entries() -; lookup(), lookup_bits() and
    expert_actions_from() dispatch on the table's type; stepped by the expert every board is won within root_moves steps, is put
    back by the auto-reset, and is won again from the same table."""
    import rtable_reference as rt
    torch = torch_cuda
    from tiler_slider_amd import SOLVE_FULL, ReachTable, _rtable_cabi as xc
    S, T, K, mc, L, n = WALKED[0]
    ref = _yard_walked(S, T, K, mc, L, n)
    blk, init, tgt = _walked(S, T, K, L, n)
    env = _env(S, mc, blk, init, tgt, max_steps=1000, auto_reset=True)
    rtab = env.build_reach_table()
    assert isinstance(rtab, ReachTable) and (rtab.table.dtype, rtab.count.dtype, rtab.root_moves.dtype, rtab.deepest.dtype, rtab.full.dtype) == (
        torch.int64, torch.int32, torch.int16, torch.int32, torch.bool)
    assert tuple(rtab.table.shape) == (n, xc.slots(CAPACITY)) and rtab.capacity == CAPACITY and len(rtab) == n and not bool(rtab.full.any())
    assert (rtab.shape_key, rtab.max_depth, rtab.root) == ((S, T, T, mc), 252, "init")
    _same_outputs(rtab, ref, "build_reach_table()")
    _same_entries(rtab, ref, "build_reach_table()")
    small = env.build_reach_table(workspace_bytes=3 * xc.workspace_bytes(env._dims, CAPACITY) + 100)
    _same_outputs(small, ref, "three slices")
    _same_entries(small, ref, "three slices")
    tight = env.build_reach_table(capacity=2)
    assert bool(tight.full.all()) and tight.count.tolist() == [SOLVE_FULL] * n and tight.entries(0)[0].numel() == 0
    assert env.lookup_bits(tight)[0].tolist() == [SOLVE_FULL] * n
    moves, best = env.lookup(rtab)
    bits = env.lookup_bits(rtab)[1]
    want = rt.lookup(_oracle(), ref, blk, tgt, init)
    np.testing.assert_array_equal(moves.cpu().numpy(), ref.root_moves)
    np.testing.assert_array_equal(bits.cpu().numpy(), want[1])
    np.testing.assert_array_equal(best.cpu().numpy(), (want[1][:, None] >> np.arange(4)) & 1 != 0)
    np.testing.assert_array_equal(env.expert_actions_from(rtab).cpu().numpy(), want[2])
    rows = torch.arange(n - 1, -1, -1)
    flipped = _env(S, mc, blk[:, ::-1].copy(), init[:, ::-1].copy(), tgt[:, ::-1].copy())
    np.testing.assert_array_equal(flipped.lookup_bits(rtab, rows=rows)[0].cpu().numpy(), ref.root_moves[::-1])
    # a board that is won when step() is called is put back on its root by that step, whatever the action (255 here)
    assert (ref.root_moves >= 1).all()
    root_moves = torch.from_numpy(ref.root_moves).to(env.device)
    left, wins = root_moves.clone(), torch.zeros(n, dtype=torch.int32, device=env.device)
    for step in range(2 * int(ref.root_moves.max()) + 1):
        assert torch.equal(env.lookup_bits(rtab)[0], left), step
        _, _, info = env.step(env.expert_actions_from(rtab))
        wins += info["success"].int()
        assert torch.equal(info["autoreset"], left == 0)
        left = torch.where(left >= 1, left - 1, root_moves)
    assert bool((wins >= 2).all())
    for kw, word in (({"max_depth": -1}, "max_depth"), ({"max_depth": 253}, "max_depth"), ({"capacity": 0}, "capacity"), ({"capacity": (1 << 30) + 1}, "capacity"),
                     ({"workspace_bytes": 1000}, "workspace"), ({"root": "start"}, "root"), ({"max_bytes": 1 << 20}, "rows=")):
        with pytest.raises(ValueError, match=word):
            env.build_reach_table(**kw)
    other = _env(4, mc, *_seeded(4, 2, 2, 8))
    with pytest.raises(ValueError, match="built for"):
        other.lookup(rtab)
    with pytest.raises(ValueError, match="rows"):
        flipped.lookup(rtab, rows=torch.arange(3))


def test_unsupported_shapes_raise_and_the_frozen_consumers_refuse_a_reach_table(torch_cuda):
    from tiler_slider_amd import VecTilerSliderEnv
    for S, T in ((9, 1), (8, 9), (6, 9)):
        env = VecTilerSliderEnv.random(4, size=S, num_tiles=T, num_obstacles=2, obs_dtype=None)
        with pytest.raises(ValueError, match="8x8 with up to 8 tiles"):
            env.build_reach_table()
    env = VecTilerSliderEnv.random(4, size=5, num_tiles=4, num_obstacles=3, obs_dtype=None)
    with pytest.raises(ValueError, match="65536"):
        env.build_table()
    env.reset()
    rtab = env.build_reach_table()
    assert env.lookup(rtab)[0].shape[0] == 4
    # out of scope: the libraries that read a dense table are frozen code objects, also on a shape they take
    env = VecTilerSliderEnv.random(4, size=4, num_tiles=2, num_obstacles=2, obs_dtype=None)
    env.reset()
    rtab = env.build_reach_table()
    assert torch_cuda.equal(env.lookup(rtab)[0], env.lookup(env.build_table())[0])
    with pytest.raises(TypeError, match="DistanceTable"):
        env.place_at_distance(rtab)
    with pytest.raises(TypeError, match="DistanceTable"):
        env.rollout(2, "table", table=rtab)
