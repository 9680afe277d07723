"""The deep rounds on the GPU: distances 36 .. 252 written by ts_table_build, ts_solve and ts_ptable_walk in both launch forms, and
read back by every consumer of a table, exact equality everywhere.  The levels are those of tests/golden/deep_levels.npz
(tests/deep_cases.py; tests/test_deep_cpu.py holds them to the yardsticks and lists their depths D = 37 .. 106), the long chains
those of deep_cases.chain_policy (L = 79, 137 and 341: beyond TS_TABLE_MAX_DEPTH, so TS_TABLE_DEEP stands next to 252 at the
default cut).  Raw calls write into memory the test owns, prefilled with the complement of the expected bytes between guard
bytes, through the helpers of the shallow suites (test_gpu_table, test_gpu_solver, test_gpu_ptable, test_gpu_starts)."""
import ctypes as C

import numpy as np
import pytest

import deep_cases as dc
import ptable_reference as xref
import table_reference as tref
import test_gpu_ptable as gp
import test_gpu_solver as gsol
import test_gpu_starts as gs
import test_gpu_table as gt
from table_harness import GUARD, _BLOCK_KNOBS, _WAVE_KNOBS, guarded as _guarded, knobs as _knobs, payload as _payload

pytestmark = pytest.mark.gpu

ALL = (dc.MULTI, dc.SINGLE, dc.REPEATED, dc.SMALL, dc.LARGE)
SOLVE_MAX_DEPTH = 32767


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _finite(d):
    return (d >= 0) & (d < tref.UNREACHABLE)


def _copies(lv, n, pos=None, **kw):
    """An environment of n boards of the level, standing on `pos` [T, n] (default: the level's deepest placement)."""
    blk, tgt = dc.tiled(lv, n)
    env = gt._env(lv.S, lv.mc, blk, np.ascontiguousarray(np.repeat(lv.init, n, axis=1)), tgt, **kw)
    if pos is not None:
        gt._put(env, "_pos", np.ascontiguousarray(pos))
    return env


def _dl(oracle, lv):
    """"D = ..., L = ..." of a level: its deepest distance and, where it has a chain policy, the longest chain."""
    D = dc.deepest(dc.exact(oracle, lv))
    return f"D = {D}" + (f", L = {dc.longest(dc.chain_policy(oracle, lv)[1])}" if lv.name in dc.CHAIN_SEED else "")


def _spread(a, k):
    """k elements of a, evenly spread (all of them where there are no more)."""
    return a if len(a) <= k else a[np.linspace(0, len(a) - 1, k).astype(np.int64)]


def _depths(D, *more):
    return sorted({d for d in (252, D + 1, D, D - 1, 64, 36) + more if 0 <= d <= 252}, reverse=True)


# ---------------------------------------------------------------------------------------------- the build
@pytest.mark.parametrize("name", ALL)
def test_build_in_both_forms_at_every_cut(torch_cuda, oracle, name):
    """max_depth 252 and D + 1 (the level ends first: NONE), D, D - 1, 64 and 36 (the cut falls inside the level: DEEP, and at D
    every distance is stored all the same): the whole table is the yardstick's cut(), on three copies of the level."""
    from tiler_slider_amd import _table_cabi as tc
    lv = dc.levels()[name]
    dist = dc.exact(oracle, lv)
    D = dc.deepest(dist)
    print(f"{name}: {_dl(oracle, lv)}")
    env = _copies(lv, 3)
    for form, knobs in (("wave", _WAVE_KNOBS), ("block", _BLOCK_KNOBS)):
        with _knobs(knobs):
            assert tc.describe_table_build(env._dims)["name"] == f"k_table_{form}<{lv.S}>"
            for depth in _depths(D):
                want = np.repeat(tref.cut(dist[None, :], depth), 3, axis=0)
                assert ((want == tref.DEEP).any(), (want == tref.NONE).any()) in ((depth <= D, depth > D), (False, False))
                np.testing.assert_array_equal(gt._build_raw(env, want, depth), want, err_msg=f"{name} {form} form, max_depth {depth}")
    env.close()


def test_build_with_a_deep_board_among_boards_that_stop_early_in_every_wave(torch_cuda, oracle):
    """Eight boards per wave (512 placements per lane), 43 boards: every wave - the ragged last one too - holds the 106-deep level
    beside a level of depth <= 3, one that is never won and one whose placements are won or stuck; the deep board moves through
    the lane groups from wave to wave.  The shallow boards stop a hundred rounds before their neighbour; every row is the
    yardstick's, at every cut."""
    from tiler_slider_amd import _table_cabi as tc
    lv = dc.levels()[dc.MULTI]
    others = dc.companions(lv)
    kinds = [lv, others["shallow"], others["never won"], others["won or stuck"]]
    n = 8 * 5 + 3
    which = (np.arange(n) + np.arange(n) // 8 + 3) % 4
    assert all(set(which[w:w + 8]) >= {0, 1} for w in range(0, n, 8)) and len({int(np.flatnonzero(which[w:w + 8] == 0)[0]) for w in range(0, n, 8)}) == 4
    cat = lambda field: np.ascontiguousarray(np.concatenate([getattr(kinds[k], field) for k in which], axis=1))
    dist = np.stack([dc.exact(oracle, kinds[k]) for k in which])
    D = dc.deepest(dist[which == 0][0])
    print(f"{lv.name}: {_dl(oracle, lv)} beside levels of depth {[dc.deepest(dc.exact(oracle, kinds[1])), None, 0]}")
    env = gt._env(lv.S, lv.mc, cat("blk"), cat("init"), cat("tgt"))
    with _knobs({**_WAVE_KNOBS, "TUNE_STATES_PER_LANE": 512}):
        d = tc.describe_table_build(env._dims)
        assert d["name"] == "k_table_wave<8>" and d["boards_per_block"] == 8 and d["lanes_per_board"] == 8 and n % 8 != 0
        for depth in _depths(D, 3, 1, 0):
            want = tref.cut(dist, depth)
            np.testing.assert_array_equal(gt._build_raw(env, want, depth), want, err_msg=f"max_depth {depth}")
    env.close()


# ---------------------------------------------------------------------------------------------- the solver
_solved = {}


def _solve_inputs(oracle, lv):
    """(pos [T, n], {max_depth: the yardstick's (moves, best)}) of boards at distance D, D - 1, 64, 36 and on unreachable
    placements; computed once per level."""
    import solver_reference as ref
    if lv.name not in _solved:
        dist = dc.exact(oracle, lv)
        D = dc.deepest(dist)
        idx = np.concatenate([_spread(np.flatnonzero(dist == d), 4) for d in sorted({D, D - 1, 64, 36}) if d <= D] + [_spread(np.flatnonzero(dist == tref.UNREACHABLE), 4)])
        pos = dc.cells_of(lv, idx)
        blk, tgt = dc.tiled(lv, len(idx))
        want = {depth: ref.solve(oracle, lv.S, lv.mc, blk, tgt, pos, depth) for depth in (D, D - 1, SOLVE_MAX_DEPTH)}
        # the two yardsticks agree: breadth-first search from the board finds the distance the relaxation gave its placement
        np.testing.assert_array_equal(want[SOLVE_MAX_DEPTH][0], np.where(_finite(dist[idx]), dist[idx], ref.SOLVE_NONE))
        np.testing.assert_array_equal(want[D][0][_finite(dist[idx])], dist[idx][_finite(dist[idx])])
        assert (want[D - 1][0][dist[idx] == D] == ref.SOLVE_DEPTH).all() and (want[D - 1][0][dist[idx] == D - 1] == D - 1).all()
        _solved[lv.name] = (pos, want, D)
    return _solved[lv.name]


@pytest.mark.parametrize("name,form,words_per_lane", ((dc.MULTI, "wave", 1), (dc.MULTI, "wave", 4), (dc.SINGLE, "wave", 1), (dc.REPEATED, "wave", 2),
                                                      (dc.SMALL, "wave", 1), (dc.SMALL, "block", 1), (dc.LARGE, "block", 1), (dc.LARGE, "wave", 1)))
def test_solve_from_deep_placements_in_both_forms(torch_cuda, oracle, name, form, words_per_lane):
    """ts_solve at max_depth D, D - 1 and TS_SOLVE_MAX_DEPTH: moves and every best bit are solver_reference's.  The block form is
    compiled for 3x3 .. 6x6, so the 5x5 levels run in both forms and the 8x8 ones in the wave form with one, two and four bitmap
    words per lane."""
    from tiler_slider_amd import _search_cabi as sc
    lv = dc.levels()[name]
    pos, want, D = _solve_inputs(oracle, lv)
    print(f"{name}: {_dl(oracle, lv)}, {pos.shape[1]} boards, moves {sorted(set(want[SOLVE_MAX_DEPTH][0].tolist()))}")
    env = _copies(lv, pos.shape[1], pos)
    L = sc.lib()
    saved = [L.ts_search_tuning(k, -1) for k in (sc.TUNE_WAVE_MAX_STATES, sc.TUNE_WORDS_PER_LANE)]
    try:
        L.ts_search_tuning(sc.TUNE_WAVE_MAX_STATES, 65536 if form == "wave" else 0)
        L.ts_search_tuning(sc.TUNE_WORDS_PER_LANE, words_per_lane)
        assert sc.describe_solve(env._dims)["name"] == f"k_solve_{form}<{lv.S}>"
        for depth in (D, D - 1, SOLVE_MAX_DEPTH):
            gsol._same(gsol._solve_raw(env, depth, want[depth]), want[depth], f"{name} {form} form, max_depth {depth}")
    finally:
        for k, v in zip((sc.TUNE_WAVE_MAX_STATES, sc.TUNE_WORDS_PER_LANE), saved):
            L.ts_search_tuning(k, v)
    env.close()


# ---------------------------------------------------------------------------------------------- playing a built table out
def _built(torch, oracle, lv):
    """The level's table from ts_table_build (into the complement of the yardstick's) as a DistanceTable of one row."""
    from tiler_slider_amd import DistanceTable
    one = _copies(lv, 1)
    full = tref.cut(dc.exact(oracle, lv)[None, :])
    got = gt._build_raw(one, full)
    np.testing.assert_array_equal(got, full)
    table = DistanceTable(torch.from_numpy(got.copy()).to(one.device), lv.S, lv.T, lv.Tt, lv.mc, tref.MAX_DEPTH)
    one.close()
    return table, full


@pytest.mark.parametrize("name", (dc.MULTI, dc.LARGE))
def test_playing_the_table_from_every_deep_placement_wins_after_exactly_its_distance(torch_cuda, oracle, name):
    """A board on every placement at distance >= 36: rollout(D, "table", epsilon=0) first wins at step `distance`, once; a twin
    stepped with expert_actions_from does the same, its `moves` falling by one on every step."""
    torch = torch_cuda
    lv = dc.levels()[name]
    dist = dc.exact(oracle, lv)
    D = dc.deepest(dist)
    idx = np.flatnonzero(_finite(dist) & (dist >= dc.DEEP_FROM))
    n, want = len(idx), dist[idx]
    print(f"{name}: {_dl(oracle, lv)}, {n} boards at distance >= {dc.DEEP_FROM}")
    table, _ = _built(torch, oracle, lv)
    env, twin = (_copies(lv, n, dc.cells_of(lv, idx), max_steps=1000) for _ in range(2))
    rows = torch.zeros(n, dtype=torch.int32, device=env.device)
    out = env.rollout(D, "table", table=table, rows=rows, epsilon=0.0, stats=("first_win", "wins", "win_moves"))
    np.testing.assert_array_equal(out.first_win.cpu().numpy(), want)
    np.testing.assert_array_equal(out.win_moves.cpu().numpy(), want)
    assert bool((out.wins == 1).all()) and bool(env.is_won().all())
    left, _ = twin.lookup_bits(table, rows=rows)
    np.testing.assert_array_equal(left.cpu().numpy(), want)
    won_at = torch.full((n,), -1, dtype=torch.int32, device=env.device)
    for step in range(1, D + 1):
        act = twin.expert_actions_from(table, rows=rows)
        assert torch.equal(act != 255, left >= 1)
        _, _, info = twin.step(act)
        now, _ = twin.lookup_bits(table, rows=rows)
        assert torch.equal(now[left >= 1], left[left >= 1] - 1) and bool((now[left < 1] == 0).all())
        won_at[(left == 1) & info["is_won"]] = step
        left = now
    np.testing.assert_array_equal(won_at.cpu().numpy(), want)
    assert torch.equal(twin.positions, env.positions)
    env.close()
    twin.close()


# ---------------------------------------------------------------------------------------------- the walk
def _walk_form(states, copies):
    return "block" if states > 1024 or (states >= 256 and copies < 32768) else "wave"


@pytest.mark.parametrize("name,copies", ((dc.MULTI, 1), (dc.MULTI, 3), (dc.LARGE, 1), (dc.SMALL, 1), (dc.SMALL, 32768)))
def test_walk_of_the_chain_policy_in_both_forms(torch_cuda, oracle, name, copies):
    """ts_ptable_walk over the chain policy at max_depth 252, 128, 127, L and L - 1 (those within 252), and ts_ptable_score of the
    walked table against the distances: ptable_reference's bytes.  The 5x5 level of two tiles is the one whose index space
    (625 <= 1024) lets the form change with the number of levels: a block per level below 32,768 levels, the wave form from there."""
    from tiler_slider_amd import _ptable_cabi as xc
    torch, dev = torch_cuda, gp._dev(torch_cuda)
    lv = dc.levels()[name]
    act, chain = dc.chain_policy(oracle, lv)
    L, states = dc.longest(chain), chain.size
    form = _walk_form(states, copies)
    print(f"{name}: {_dl(oracle, lv)}, {copies} levels, {form} form")
    assert xc.describe_ptable_walk(gp._dims(lv.S, lv.T, lv.Tt, lv.mc, copies))["name"] == f"k_ptable_walk_{form}<{lv.S}>"
    assert {_walk_form(625, 1), _walk_form(625, 32768)} == {"block", "wave"}
    blk, tgt = dc.tiled(lv, copies)
    rep = lambda a: np.ascontiguousarray(np.repeat(a, copies, axis=0))
    table = tref.cut(dc.exact(oracle, lv)[None, :])
    depths = [d for d in (252, 128, 127, L, L - 1) if d <= 252]
    for depth in depths if copies <= 3 else (252, L - 1):
        row = xref.walk(oracle, lv.S, lv.mc, lv.blk, lv.tgt, lv.T, act[None, :], depth)
        assert (row == tref.DEEP).any() if depth < L else depth == L or not (row == tref.DEEP).any()
        want = dict(dist=rep(row))
        if copies <= 3:
            want["score"] = rep(xref.score(oracle, lv.S, lv.mc, lv.blk, lv.tgt, lv.T, row, act[None, :], table))
        bad = gp._run_all(torch, dev, lv.S, lv.T, lv.Tt, lv.mc, blk, tgt, want, act_in=rep(act[None, :]), max_depth=depth, table=rep(table) if copies <= 3 else None)
        assert bad == [], (name, copies, depth)


@pytest.mark.parametrize("name", ALL)
def test_walking_the_expert_gives_the_built_distance_table(torch_cuda, oracle, name):
    """The expert's move on every placement (table_reference.lookup over the yardstick's table), walked at max_depth 252 and
    D - 1: the yardstick's cut(), which test_build_... holds ts_table_build to."""
    torch, dev = torch_cuda, gp._dev(torch_cuda)
    lv = dc.levels()[name]
    dist = dc.exact(oracle, lv)
    D = dc.deepest(dist)
    print(f"{name}: {_dl(oracle, lv)}")
    expert, _ = xref.expert_actions(oracle, lv.S, lv.mc, lv.blk, lv.tgt, lv.T, tref.cut(dist[None, :]))
    env = _copies(lv, 1)
    for depth in (252, D - 1):
        want = tref.cut(dist[None, :], depth)
        assert gp._run_all(torch, dev, lv.S, lv.T, lv.Tt, lv.mc, lv.blk, lv.tgt, dict(dist=want), act_in=expert, max_depth=depth) == [], depth
        np.testing.assert_array_equal(env.build_table(depth).dist.cpu().numpy(), want)
    env.close()


# ---------------------------------------------------------------------------------------------- consumers of entries >= 128 a kernel wrote
@pytest.fixture(scope="module")
def walked(torch_cuda, oracle):
    """name -> (PolicyTable from ts_ptable_walk at the default cut, its bytes, L): entries 128 .. 137 on the 8x8 level, 128 .. 252 and
    DEEP on the 5x5 level of three tiles.  The bytes are ptable_reference.walk's."""
    torch = torch_cuda
    made = {}

    def get(name):
        if name not in made:
            lv = dc.levels()[name]
            act, chain = dc.chain_policy(oracle, lv)
            env = _copies(lv, 1)
            pt = env.walk_actions(torch.from_numpy(act[None, :].copy()).to(env.device))
            got = pt.dist.cpu().numpy()
            np.testing.assert_array_equal(got, xref.walk(oracle, lv.S, lv.mc, lv.blk, lv.tgt, lv.T, act[None, :]))
            assert (got[got <= 252] >= 128).sum() >= 50
            made[name] = (pt, got, dc.longest(chain))
            env.close()
        return made[name]
    return get


@pytest.mark.parametrize("name", (dc.MULTI, dc.LARGE))
def test_lookup_on_a_walked_table(torch_cuda, oracle, walked, name):
    """A board on every valid placement: moves (int16: 128 and more stay positive), best and action are table_reference.lookup's."""
    torch = torch_cuda
    lv = dc.levels()[name]
    pt, tab, L = walked(name)
    idx = np.flatnonzero(dc.exact(oracle, lv) >= 0)
    pos, n = dc.cells_of(lv, idx), len(idx)
    rows = np.zeros(n, np.int32)
    want = tref.lookup(oracle, lv.S, dc.tiled(lv, n)[0], pos, tab, rows=rows)
    print(f"{name}: {_dl(oracle, lv)}, {n} boards, moves >= 128 on {(want[0] >= 128).sum()}, -2 on {(want[0] == -2).sum()}, with a best move {(want[1] != 0).sum()}")
    assert want[0].max() == min(L, 252) and (want[0] >= 128).sum() >= 50 and ((want[1] != 0) & (want[0] >= 129)).sum() >= 50
    assert (want[0] == -2).any() == (L > 252)
    env = _copies(lv, n, pos)
    gt._lookup_checked(env, pt.dist, torch.from_numpy(rows).to(env.device), want, name)
    env.close()


@pytest.mark.parametrize("name", (dc.MULTI, dc.LARGE))
def test_labels_of_a_logged_rollout_from_deep_placements(torch_cuda, oracle, walked, name):
    """Six logged steps of the table policy over the WALKED table from boards at chain length >= 128: the GPU's log is the
    yardstick's, and ts_traj_labels on it, into guarded memory, gives targets_reference.labels."""
    import rollout_reference as rref
    import targets_reference as gr
    from tiler_slider_amd import _cabi, _targets_cabi as gc
    torch = torch_cuda
    lv = dc.levels()[name]
    pt, tab, L = walked(name)
    K = 6
    idx = _spread(np.flatnonzero((tab >= 128) & (tab <= 252)), 200)
    pos, n = dc.cells_of(lv, idx), len(idx)
    blk, tgt = dc.tiled(lv, n)
    rows = np.zeros(n, np.int32)
    log = rref.rollout(oracle, lv.S, lv.mc, 1000, blk, pos, tgt, K, rref.TABLE, 0, table=tab, rows=rows, threshold=0, seed=1)
    want = gr.labels(oracle, lv.S, blk, pos, log["pos_log"], tab, rows)
    print(f"{name}: {_dl(oracle, lv)}, {n} boards, labels {want[0].min()} .. {want[0].max()}")
    assert want[0].min() >= 128 - K and want[0].max() >= 128 and (want[2] != 255).all() and log["source"].tolist() == [K * n, 0, 0]
    np.testing.assert_array_equal(want[0], tab[0, idx][None, :].astype(np.int16) - np.arange(K)[:, None])     # one link a step
    env = _copies(lv, n, pos, max_steps=1000)
    dev = env.device
    out = env.rollout(K, "table", table=pt, rows=torch.from_numpy(rows).to(dev), epsilon=0.0, seed=1, log=("start", "pos", "act"), stats=False)
    np.testing.assert_array_equal(out.pos_log.cpu().numpy(), log["pos_log"])
    np.testing.assert_array_equal(out.act_log.cpu().numpy(), log["act_log"])
    comp = lambda a: np.ascontiguousarray(~np.ascontiguousarray(a).view(np.uint8)).view(a.dtype).reshape(a.shape)
    outs = dict(zip(("moves", "best", "action"), want))
    g = {k: _guarded(torch, dev, v) for k, v in dict(blk=blk, first=pos, pos_log=log["pos_log"][:K - 1], rows=rows).items()}
    g.update({k: _guarded(torch, dev, comp(v)) for k, v in outs.items()})
    at = lambda k: g[k].data_ptr() + GUARD
    st = _cabi.State(None, None, None, at("blk"), None, None, None)
    tin = gc.LabelsIn(at("first"), at("pos_log"), pt.dist.data_ptr(), at("rows"), 1, K, 0)
    tout = gc.LabelsOut(at("moves"), at("best"), at("action"))
    assert gc.lib().ts_traj_labels(C.byref(env._dims), C.byref(st), C.byref(tin), C.byref(tout), torch.cuda.current_stream(dev).cuda_stream) == 0
    for k, v in outs.items():
        np.testing.assert_array_equal(_payload(g[k], v.dtype, v.shape), v, err_msg=f"{name}: {k}")
    env.close()


@pytest.mark.parametrize("name", (dc.MULTI, dc.LARGE))
def test_starts_in_deep_bands(torch_cuda, oracle, walked, name):
    """ts_starts_place over the walked table with the bands [128, 252], [L, L], [L + 1, 252] (empty: nothing is placed) and a band
    per board, and over the built distance table with [36, D]: count, dist, deepest, the cells and every other byte of the state
    are starts_reference's, and every placed board stands at a distance inside its band."""
    import starts_reference as sref
    from tiler_slider_amd import _cabi, _starts_cabi as sc
    torch, dev = torch_cuda, gp._dev(torch_cuda)
    lv = dc.levels()[name]
    pt, tab, L = walked(name)
    built, full = _built(torch, oracle, lv)
    D = dc.deepest(dc.exact(oracle, lv))
    top = min(L, 252)                                                   # the largest distance the walked table holds
    print(f"{name}: {_dl(oracle, lv)}")
    N, C_, T = 257, lv.S * lv.S, lv.T
    rng = np.random.default_rng(L)
    per_board = np.stack([rng.integers(100, top + 4, N), np.zeros(N, np.int64)]).astype(np.uint8)
    per_board[1] = np.minimum(per_board[0].astype(np.int64) + rng.integers(-2, 12, N), 255)
    per_board[1, ::9] = rng.integers(253, 256, len(per_board[1, ::9]))
    cases = [("walked", 128, 252, None), ("walked", top, top, None), ("built", 36, D, None), ("walked", 1, 252, per_board)]
    if top < 252:
        cases.append(("walked", top + 1, 252, None))
    dims = _cabi.Dims(N, lv.S, lv.T, lv.Tt, int(lv.mc), 100, 0)
    rows = np.zeros(N, np.int32)
    for which, lo, hi, band in cases:
        t, bytes_ = (pt.dist, tab) if which == "walked" else (built.dist, full)
        ref = sref.place(bytes_, C_, T, N, lo, hi, band=band, rows=rows, seed=gs.SEED, step_index=5, board_offset=1000)
        los, his = (band[0].astype(np.int64), np.minimum(band[1], 252).astype(np.int64)) if band is not None else (np.full(N, lo), np.full(N, hi))
        e = bytes_[0].astype(np.int64)
        np.testing.assert_array_equal(ref["count"], ((e[None, :] >= los[:, None]) & (e[None, :] <= his[:, None])).sum(axis=1))
        placed = ref["placed"]
        assert (ref["deepest"] == (top if which == "walked" else D)).all() and np.array_equal(placed, ref["count"] > 0)
        assert ((ref["dist"][placed] >= los[placed]) & (ref["dist"][placed] <= his[placed])).all() and (ref["dist"][~placed] == 255).all()
        assert np.array_equal(bytes_[0, tref.index_of(lv.S, ref["cells"][:, placed])], ref["dist"][placed])
        if band is None:
            assert placed.all() == (lo <= top if which == "walked" else True) and placed.any() == placed.all()
            assert lo >= top or len(set(ref["idx"].tolist())) > 20
        else:
            assert placed.sum() >= 20 and (~placed).sum() >= 20 and (ref["dist"][placed] >= 128).sum() >= 20
        before = gs._state(rng, C_, T, N)
        before["rows"] = rows
        if band is not None:
            before["band"] = band
        arena = gs._Arena(before)
        buf = torch.from_numpy(arena.build(before)).to(dev)
        kw = dict(lo=lo, hi=hi, where=sc.ALL, write_pos=1, write_init=1, seed=gs.SEED, step_index=5, board_offset=1000)
        assert gs._raw_call(torch, dev, dims, arena, buf, t.data_ptr(), 1, kw, True, band is not None) == 0
        after = dict(before)
        after["pos"], after["init"], after["step_count"], after["done"] = sref.apply(ref, before["pos"], before["init"], before["step_count"], before["done"], 1, 1)
        after["count"], after["dist"], after["deepest"] = ref["count"], ref["dist"], ref["deepest"]
        assert not arena.differing(buf.cpu().numpy(), arena.build(after)), (name, which, lo, hi)
