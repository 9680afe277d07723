"""ts_starts_place on the GPU, exact equality everywhere, against the NumPy definition (tests/starts_reference.py).  Every raw
call works on memory the test owns: all state and output arrays lie in ONE buffer with 256 guard bytes before, between and
after them, and the whole buffer - guards, arrays the call may not write, boards that are not placed - is compared byte for byte
with the same buffer built from the yardstick's answer; the table lies between guards of its own and is compared afterwards."""
import ctypes as C

import numpy as np
import pytest

import starts_reference as sref
from table_harness import GUARD, GUARD_BYTE, guarded as _guarded, payload as _payload

pytestmark = pytest.mark.gpu

SEED = 0xF00DFACE12345678      # above 2^63: the seed is unsigned
SHAPES = ((1, 1), (2, 2), (3, 1), (3, 2), (5, 2), (6, 2), (7, 1), (4, 2), (8, 1), (4, 3), (8, 2), (3, 5))      # states 1 .. 59,049, mostly odd; every size
BOARDS = (1, 63, 257)
BANDS = ((0, 0), (1, 252), (2, 4), (5, 3), "per board")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


class _Arena:
    """Named arrays in one uint8 buffer: GUARD guard bytes, an array, guard bytes up to the next multiple of 16, GUARD guard
    bytes, the next array, ...  `build` lays out any dict of arrays of the same shapes and dtypes the same way."""

    def __init__(self, arrays):
        self.names = list(arrays)
        self.at, off = {}, GUARD
        for name, a in arrays.items():
            self.at[name] = (off, a.dtype, a.shape)
            off += a.nbytes + (-a.nbytes) % 16 + GUARD
        self.nbytes = off

    def build(self, arrays):
        host = np.full(self.nbytes, GUARD_BYTE, np.uint8)
        for name in self.names:
            off, dtype, shape = self.at[name]
            a = np.ascontiguousarray(arrays[name], dtype)
            assert a.shape == shape
            host[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
        return host

    def ptr(self, buf, name):
        return buf.data_ptr() + self.at[name][0]

    def differing(self, got, want):
        """The names of the arrays that differ, 'guard' for a byte between them."""
        bad, covered = [], np.zeros(self.nbytes, bool)
        for name in self.names:
            off, dtype, shape = self.at[name]
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            covered[off:off + n] = True
            if not np.array_equal(got[off:off + n], want[off:off + n]):
                bad.append(name)
        if not np.array_equal(got[~covered], want[~covered]):
            bad.append("guard")
        return bad


def _raw_call(torch, dev, dims, arena, buf, table_ptr, n_rows, cfg_kw, use_rows, use_band, outputs=("count", "dist", "deepest"), with_state=True):
    from tiler_slider_amd import _cabi, _starts_cabi as sc
    st = _cabi.State(arena.ptr(buf, "pos"), arena.ptr(buf, "init"), None, None, arena.ptr(buf, "step_count"), arena.ptr(buf, "done"), None)
    cfg = sc.StartsCfg(band=arena.ptr(buf, "band") if use_band else None, reserved=0, **cfg_kw)
    out = sc.StartsOut(**{k: arena.ptr(buf, k) for k in outputs})
    return sc.lib().ts_starts_place(C.byref(dims), C.byref(st) if with_state else None, table_ptr, n_rows, arena.ptr(buf, "rows") if use_rows else None,
                                    C.byref(cfg), C.byref(out), torch.cuda.current_stream(dev).cuda_stream)


def _state(rng, C_, T, N):
    """A state nobody reset and outputs nobody cleared: random cells, counters and flags; random bytes where the answers go."""
    return dict(pos=rng.integers(0, C_, (T, N)).astype(np.uint8), init=rng.integers(0, C_, (T, N)).astype(np.uint8),
                step_count=rng.integers(0, 100, N).astype(np.int32), done=rng.integers(0, 2, N).astype(np.uint8),
                count=rng.integers(-9, 9, N).astype(np.int32), dist=rng.integers(0, 256, N).astype(np.uint8),
                deepest=rng.integers(0, 256, N).astype(np.uint8), band=np.zeros((2, N), np.uint8), rows=np.zeros(N, np.int32))


def _made_up_table(rng, n_rows, states, lo, hi):
    """A table nobody built: random bytes; in every third row every entry, and in every other third a third of the entries, are
    forced into the band (where it is not empty), and one row holds no distance at all - counts run from 0 to the whole row."""
    tab = rng.integers(0, 256, (n_rows, states), dtype=np.uint8)
    if lo <= hi:
        inside = rng.integers(lo, hi + 1, (n_rows, states), dtype=np.uint8)
        tab[0::3] = inside[0::3]
        third = rng.integers(0, 3, inside[1::3].shape, dtype=np.uint8) == 0
        tab[1::3] = np.where(third, inside[1::3], tab[1::3])
    if n_rows > 3:
        tab[3] = rng.integers(253, 256, states, dtype=np.uint8)
    return tab


@pytest.mark.parametrize("S,T", SHAPES)
def test_the_scan_at_every_alignment(torch_cuda, S, T):
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _starts_cabi as sc
    dev = torch.device("cuda", torch.cuda.current_device())
    C_, states = S * S, (S * S) ** T
    rng = np.random.default_rng(1000 * S + T)
    placed_total = unplaced_total = 0
    counts_seen = set()
    for N in BOARDS:
        dims = _cabi.Dims(N, S, T, T, 0, 100, 0)
        for case in ("rows=None", "rows with repeats", "rows out of range"):
            n_rows = N if case == "rows=None" else max(1, min(N // 3, 40))
            rows = None
            if case != "rows=None":
                rows = rng.integers(0, n_rows, N).astype(np.int32)
                if case == "rows out of range":
                    rows[rng.integers(0, N)] = n_rows
                    rows[rng.integers(0, N)] = -1
            # an odd shift of the table in its allocation: rows then start at every residue of 16 whatever `states` is
            shift = 0 if case == "rows=None" else 5
            for band_case in BANDS:
                band = None
                lo, hi = (1, 252) if band_case == "per board" else band_case
                if band_case == "per board":
                    band = rng.integers(0, 256, (2, N)).astype(np.uint8)
                    band[1, ::2] = np.maximum(band[1, ::2], band[0, ::2])     # half of the bands are not empty
                    band[1, ::5] = rng.integers(253, 256, len(band[1, ::5]))  # bytes above the largest distance
                    band[0, 3::7] = rng.integers(253, 256, len(band[0, 3::7]))
                tab = _made_up_table(rng, n_rows, states, lo, hi)
                # the bytes before the shifted table are distances inside every band that is not empty, as the guard byte 165 is inside [1, 252]
                tbuf = _guarded(torch, dev, np.concatenate([np.full(shift, 3 if (lo, hi) == (2, 4) else lo, np.uint8), tab.reshape(-1)]))
                ref = sref.place(tab, C_, T, N, lo, hi, band=band, rows=rows, seed=SEED, step_index=5, board_offset=1000)
                placed_total += int(ref["placed"].sum())
                unplaced_total += int((~ref["placed"]).sum())
                counts_seen |= set(ref["count"].tolist())
                before = _state(rng, C_, T, N)
                if band is not None:
                    before["band"] = band
                if rows is not None:
                    before["rows"] = rows
                arena = _Arena(before)
                for write_pos in (0, 1):
                    for write_init in (0, 1):
                        buf = torch.from_numpy(arena.build(before)).to(dev)
                        kw = dict(lo=lo, hi=hi, where=sc.ALL, write_pos=write_pos, write_init=write_init, seed=SEED, step_index=5, board_offset=1000)
                        rc = _raw_call(torch, dev, dims, arena, buf, tbuf.data_ptr() + GUARD + shift, n_rows, kw, rows is not None, band is not None)
                        assert rc == 0, rc
                        after = dict(before)
                        after["pos"], after["init"], after["step_count"], after["done"] = sref.apply(
                            ref, before["pos"], before["init"], before["step_count"], before["done"], write_pos, write_init)
                        after["count"], after["dist"], after["deepest"] = ref["count"], ref["dist"], ref["deepest"]
                        bad = arena.differing(buf.cpu().numpy(), arena.build(after))
                        assert not bad, (S, T, N, case, band_case, write_pos, write_init, bad)
                np.testing.assert_array_equal(_payload(tbuf, np.uint8, (shift + n_rows * states,))[shift:], tab.reshape(-1))
    assert placed_total > 0 and unplaced_total > 0
    assert 0 in counts_seen and states in counts_seen and (states <= 2 or len(counts_seen) > 3)      # from nothing to the whole row


@pytest.mark.parametrize("name", sorted(sref.OCCUPANCY_CASES))
def test_every_compiled_starts_kernel_at_occupancy(torch_cuda, name):
    """Every kernel of the starts library at 4,096 one-wave blocks and more, the last one ragged where a block holds several
    boards: a made-up table of 128 rows read through rows=, a band per board, every byte of state, outputs and guards against the
    yardstick's."""
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _starts_cabi as sc
    dev = torch.device("cuda", torch.cuda.current_device())
    S, T = sref.OCCUPANCY_CASES[name]
    C_, states = S * S, (S * S) ** T
    rng = np.random.default_rng(0x0CC + S)
    per_block = sc.describe_starts_place(_cabi.Dims(1, S, T, T, 0, 100, 0))["boards_per_block"]
    N = sref.occupancy_boards(per_block)
    dims = _cabi.Dims(N, S, T, T, 0, 100, 0)
    d = sc.describe_starts_place(dims)
    assert d["name"] == name and d["threads_per_block"] == 64 and d["blocks"] >= sref.OCC_BLOCKS and (per_block == 1 or N % per_block != 0)
    n_rows = sref.OCC_ROWS
    tab = _made_up_table(rng, n_rows, states, 1, 252)
    rows = rng.integers(0, n_rows, N).astype(np.int32)
    rows[rng.integers(0, N, 8)] = np.array([-1, n_rows] * 4, np.int32)
    band = rng.integers(0, 256, (2, N)).astype(np.uint8)
    band[1, ::2] = np.maximum(band[1, ::2], band[0, ::2])     # half of the bands are not empty
    band[1, ::5] = rng.integers(253, 256, len(band[1, ::5]))  # bytes above the largest distance
    ref = sref.place(tab, C_, T, N, band=band, rows=rows, seed=SEED, step_index=5, board_offset=1000)
    placed, counts = int(ref["placed"].sum()), set(ref["count"].tolist())
    print(f"{name}: {N} boards in {d['blocks']} blocks of {per_block}, {placed} placed, {N - placed} not, counts {min(counts)} .. {max(counts)} of {states}")
    assert placed >= 64 and N - placed >= 64 and 0 in counts and (states <= 2 or len(counts) > 3)
    tbuf = _guarded(torch, dev, tab)
    before = _state(rng, C_, T, N)
    before["band"], before["rows"] = band, rows
    arena = _Arena(before)
    buf = torch.from_numpy(arena.build(before)).to(dev)
    kw = dict(lo=1, hi=252, where=sc.ALL, write_pos=1, write_init=1, seed=SEED, step_index=5, board_offset=1000)
    assert _raw_call(torch, dev, dims, arena, buf, tbuf.data_ptr() + GUARD, n_rows, kw, True, True) == 0
    after = dict(before)
    after["pos"], after["init"], after["step_count"], after["done"] = sref.apply(ref, before["pos"], before["init"], before["step_count"], before["done"], 1, 1)
    after["count"], after["dist"], after["deepest"] = ref["count"], ref["dist"], ref["deepest"]
    bad = arena.differing(buf.cpu().numpy(), arena.build(after))
    assert not bad, (name, bad)
    np.testing.assert_array_equal(_payload(tbuf, np.uint8, (n_rows * states,)), tab.reshape(-1))


def test_starts_done_places_exactly_the_boards_that_are_done(torch_cuda):
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _starts_cabi as sc
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(77)
    for S, T, N in ((4, 2, 257), (3, 2, 63), (5, 2, 130)):
        C_, states = S * S, (S * S) ** T
        dims = _cabi.Dims(N, S, T, T, 0, 100, 0)
        tab = _made_up_table(rng, N, states, 1, 9)
        tab[1] = 255         # a done board without a placement in the band stays as it is
        tbuf = _guarded(torch, dev, tab)
        before = _state(rng, C_, T, N)
        before["done"] = (rng.integers(0, 3, N) * 127).astype(np.uint8)      # 0, 127 or 254: any byte but 0 is done
        before["done"][1] = 1
        sel = before["done"] != 0
        ref = sref.place(tab, C_, T, N, 1, 9, selected=sel, seed=3, step_index=2)
        assert ref["placed"][sel & (ref["count"] > 0)].all() and not ref["placed"][~sel].any() and not ref["placed"][1]
        assert ref["placed"].sum() >= N // 4 and (~sel).sum() >= N // 5 and (ref["count"][~sel] > 0).any()
        arena = _Arena(before)
        buf = torch.from_numpy(arena.build(before)).to(dev)
        kw = dict(lo=1, hi=9, where=sc.DONE, write_pos=1, write_init=1, seed=3, step_index=2, board_offset=0)
        assert _raw_call(torch, dev, dims, arena, buf, tbuf.data_ptr() + GUARD, N, kw, False, False) == 0
        after = dict(before)
        after["pos"], after["init"], after["step_count"], after["done"] = sref.apply(ref, before["pos"], before["init"], before["step_count"], before["done"], 1, 1)
        after["count"], after["dist"], after["deepest"] = ref["count"], ref["dist"], ref["deepest"]
        assert not arena.differing(buf.cpu().numpy(), arena.build(after)), (S, T, N)
        # boards that are not done keep every byte; boards that are done and placed are not done afterwards
        assert (after["done"][~sel] == 0).all() and (after["done"][ref["placed"]] == 0).all() and after["done"][1] == 1


def test_empty_inputs_launch_nothing_and_write_nothing(torch_cuda):
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _starts_cabi as sc
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(5)
    before = _state(rng, 16, 2, 63)
    arena = _Arena(before)
    tab = _made_up_table(rng, 63, 256, 1, 252)
    tbuf = _guarded(torch, dev, tab)
    kw = dict(lo=1, hi=252, where=sc.ALL, write_pos=1, write_init=1, seed=1, step_index=0, board_offset=0)
    for n_boards, n_rows, table_ptr in ((0, 63, tbuf.data_ptr() + GUARD), (63, 0, tbuf.data_ptr() + GUARD), (63, 0, None), (0, 0, None)):
        buf = torch.from_numpy(arena.build(before)).to(dev)
        dims = _cabi.Dims(n_boards, 4, 2, 2, 0, 100, 0)
        assert _raw_call(torch, dev, dims, arena, buf, table_ptr, n_rows, kw, False, False) == 0
        assert np.array_equal(buf.cpu().numpy(), arena.build(before)), (n_boards, n_rows)
    assert _raw_call(torch, dev, _cabi.Dims(0, 4, 2, 2, 0, 100, 0), arena, buf, None, 0, kw, False, False, outputs=(), with_state=False) == 0
    assert sc.lib().ts_starts_last_hip_error() == 0


# ------------------------------------------------------------------------------------------------------------- the environment
REAL = ((4, 2, 2, False), (4, 2, 2, True), (3, 2, 1, False))


@pytest.fixture(scope="module")
def real_levels(oracle):
    """(S, T, mc) -> (blk, init, tgt, the yardstick's table): 300 seeded levels each, solved once on the CPU."""
    import table_reference as tref
    out = {}
    for S, T, K, mc in REAL:
        blk, init, tgt = oracle.generate(S, T, T, K, 300, seed=0x5EED)
        out[S, T, mc] = (blk, init, tgt, tref.table(oracle, S, mc, blk, tgt, T))
    return out


def _env(S, mc, blk, init, tgt, **kw):
    from tiler_slider_amd import VecTilerSliderEnv
    kw.setdefault("obs_dtype", None)
    return VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=mc, **kw)


@pytest.mark.parametrize("S,T,K,mc", REAL)
@pytest.mark.parametrize("lo,hi", ((1, 252), (2, 4)))
def test_real_tables_place_boards_where_the_lookup_reads_the_same_distance(torch_cuda, real_levels, S, T, K, mc, lo, hi):
    torch = torch_cuda
    blk, init, tgt, tab = real_levels[S, T, mc]
    n = tab.shape[0]
    ref = sref.place(tab, S * S, T, n, lo, hi, seed=0xBEEF, step_index=1)
    share = ref["placed"].mean()
    print(f"{S}x{S} mc={mc} band [{lo}, {hi}]: {share:.0%} of {n} boards are placed, deepest of a row up to {ref['deepest'][ref['deepest'] != 255].max()}")
    assert 0.1 <= share <= 0.9, share      # the test cannot pass on empty bands alone, nor on full ones
    env = _env(S, mc, blk, init, tgt)
    env.reset()
    table = env.build_table()
    np.testing.assert_array_equal(table.dist.cpu().numpy(), tab)
    info = env.place_at_distance(table, lo, hi, seed=0xBEEF, step_index=1)
    assert (info.count.dtype, info.dist.dtype, info.deepest.dtype, info.placed.dtype) == (torch.int32, torch.uint8, torch.uint8, torch.bool)
    for name in ("count", "dist", "deepest", "placed"):
        np.testing.assert_array_equal(getattr(info, name).cpu().numpy(), ref[name], err_msg=name)
    p = ref["placed"]
    pos = env.positions.cpu().numpy()
    np.testing.assert_array_equal(pos[:, p], ref["cells"][:, p])
    np.testing.assert_array_equal(pos[:, ~p], init[:, ~p])                       # not placed: where they stood
    np.testing.assert_array_equal(env._init.cpu().numpy(), np.where(p, ref["cells"], init))
    moves = env.lookup(table)[0].cpu().numpy()
    np.testing.assert_array_equal(moves[p], ref["dist"][p].astype(np.int16))
    assert ((moves[p] >= lo) & (moves[p] <= hi)).all()
    # set_initial=False moves the boards and leaves the level's start alone; rows= reads the same rows in another order
    env2 = _env(S, mc, blk[:, ::-1], init[:, ::-1], tgt[:, ::-1])
    env2.reset()
    back = torch.arange(n - 1, -1, -1, dtype=torch.int32, device=env2.device)
    info2 = env2.place_at_distance(table, lo, hi, rows=back, seed=0xBEEF, step_index=1, set_initial=False)
    ref2 = sref.place(tab, S * S, T, n, lo, hi, rows=np.arange(n)[::-1], seed=0xBEEF, step_index=1)
    np.testing.assert_array_equal(info2.count.cpu().numpy(), ref["count"][::-1])
    np.testing.assert_array_equal(info2.dist.cpu().numpy(), ref2["dist"])
    np.testing.assert_array_equal(env2.positions.cpu().numpy(), np.where(ref2["placed"], ref2["cells"], init[:, ::-1]))
    np.testing.assert_array_equal(env2._init.cpu().numpy(), init[:, ::-1])


@pytest.mark.parametrize("kind", ("float32", "uint8", "none", "inplace"))
def test_the_observation_and_the_restart_follow_the_placement(torch_cuda, oracle, real_levels, kind):
    """An environment placed with set_initial=True is, from then on, the environment built on the placed cells: six steps in
    auto-reset mode with three moves per episode - every board finishes and restarts - against that twin."""
    torch = torch_cuda
    from tiler_slider_amd import _cabi
    S, T, mc = 4, 2, True
    blk, init, tgt, tab = real_levels[S, T, mc]
    n = tab.shape[0]
    kw = dict(max_steps=3, auto_reset=True, obs_dtype=None if kind == "none" else "float32" if kind == "inplace" else kind,
              obs_update="inplace" if kind == "inplace" else "auto")
    env = _env(S, mc, blk, init, tgt, **kw)
    assert env._in_place == (kind == "inplace")
    env.reset()
    table = env.build_table()
    for k in range(2):       # the buffer shows other cells than the start's when the boards are placed
        env.step(torch.from_numpy(oracle.fill_actions(n, seed=9, step_index=k)))
    env.reset()
    flags_before = env._flags.clone()
    info = env.place_at_distance(table, 1, 252, seed=0x0B5, set_initial=True)
    assert torch.equal(env._flags, flags_before)                               # the last step's info is left as it is
    ref = sref.place(tab, S * S, T, n, 1, 252, seed=0x0B5)
    placed_init = np.where(ref["placed"], ref["cells"], init)
    assert ref["placed"].sum() >= n // 10 and (placed_init != init).any()
    np.testing.assert_array_equal(info.placed.cpu().numpy(), ref["placed"])
    twin = _env(S, mc, blk, placed_init, tgt, **kw)
    want = twin.reset()
    if kind != "none":
        assert torch.equal(env._obs, want), "the buffer shows the placed cells"
    restarted = np.zeros(n, bool)
    for k in range(6):
        act = torch.from_numpy(oracle.fill_actions(n, seed=0x57A7, step_index=k))
        obs, done, step_info = env.step(act)
        tobs, tdone, tinfo = twin.step(act)
        if kind != "none":
            assert torch.equal(obs, tobs), (kind, k, "obs")
        assert torch.equal(step_info["flags"], tinfo["flags"]) and torch.equal(done, tdone), (kind, k)
        assert torch.equal(env.positions, twin.positions) and torch.equal(env.step_count, twin.step_count), (kind, k)
        restarted |= (step_info["flags"].cpu().numpy() & _cabi.FLAG_AUTORESET) != 0
    assert restarted.all()       # every board finished and restarted - on the placed cells, or the twin would differ
    env.reset()
    np.testing.assert_array_equal(env.positions.cpu().numpy(), placed_init)


def test_same_bits_on_every_run_and_another_step_index_draws_again(torch_cuda, real_levels):
    torch = torch_cuda
    S, T, mc = 4, 2, False
    blk, init, tgt, tab = real_levels[S, T, mc]
    env = _env(S, mc, blk, init, tgt)
    env.reset()
    table = env.build_table()
    runs = []
    for step_index in (0, 0, 1):
        env._pos.copy_(env._init)
        info = env.place_at_distance(table, 1, 252, seed=21, step_index=step_index, set_initial=False)
        runs.append([t.clone() for t in (info.count, info.dist, info.deepest, info.placed, env.positions)])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert torch.equal(runs[0][0], runs[2][0]) and torch.equal(runs[0][2], runs[2][2]) and torch.equal(runs[0][3], runs[2][3])
    assert not torch.equal(runs[0][4], runs[2][4])        # the draw changed; count, deepest and who is placed did not
    # board_offset shifts the stream: boards 100 .. of a run at offset 0 are boards 0 .. of a run at offset 100
    ref = sref.place(tab, S * S, T, 300, 1, 252, seed=21, board_offset=100)
    env._pos.copy_(env._init)
    info = env.place_at_distance(table, 1, 252, seed=21, board_offset=100, set_initial=False)
    np.testing.assert_array_equal(info.dist.cpu().numpy(), ref["dist"])
    np.testing.assert_array_equal(env.positions.cpu().numpy(), np.where(ref["placed"], ref["cells"], init))


def test_band_per_board_and_only_done_through_the_wrapper(torch_cuda, oracle, real_levels):
    torch = torch_cuda
    S, T, mc = 4, 2, False
    blk, init, tgt, tab = real_levels[S, T, mc]
    n = tab.shape[0]
    env = _env(S, mc, blk, init, tgt, max_steps=2)
    env.reset()
    table = env.build_table()
    for k in range(2):
        env.step(torch.from_numpy(oracle.fill_actions(n, seed=4, step_index=k)))
    assert bool(env.done.all())                       # strict mode, two moves per episode: everything is done
    env._done[::2] = 0
    done = env.done.cpu().numpy()
    rng = np.random.default_rng(8)
    band = np.sort(rng.integers(0, 8, (2, n)), axis=0).astype(np.uint8)
    pos, steps = env.positions.cpu().numpy().copy(), env.step_count.cpu().numpy().copy()
    info = env.place_at_distance(table, band=torch.from_numpy(band).to(env.device), seed=6, only_done=True, set_initial=False)
    ref = sref.place(tab, S * S, T, n, band=band, selected=done, seed=6)
    assert ref["placed"].sum() >= n // 10 and not ref["placed"][::2].any()
    for name in ("count", "dist", "deepest", "placed"):
        np.testing.assert_array_equal(getattr(info, name).cpu().numpy(), ref[name], err_msg=name)
    want = sref.apply(ref, pos, init, steps, done.astype(np.uint8), True, False)
    np.testing.assert_array_equal(env.positions.cpu().numpy(), want[0])
    np.testing.assert_array_equal(env.step_count.cpu().numpy(), want[2])
    np.testing.assert_array_equal(env.done.cpu().numpy(), want[3] != 0)


def test_the_wrapper_refuses_what_it_cannot_place(torch_cuda, real_levels):
    torch = torch_cuda
    blk, init, tgt, _ = real_levels[4, 2, False]
    env = _env(4, False, blk, init, tgt)
    table = env.build_table()
    b3, i3, t3, _ = real_levels[3, 2, False]
    other = _env(3, False, b3, i3, t3)
    with pytest.raises(ValueError):
        other.place_at_distance(table)                                       # a table of another shape
    with pytest.raises(TypeError):
        env.place_at_distance(table.dist)
    n = env.num_envs
    good = torch.ones((2, n), dtype=torch.uint8, device=env.device)
    for band in (good[:, :-1], good[0], good.to(torch.int32), good.cpu(), good.cpu().numpy()):
        with pytest.raises(ValueError):
            env.place_at_distance(table, band=band)
    for kw in (dict(min_moves=-1), dict(min_moves=253), dict(max_moves=253), dict(max_moves=-1)):
        with pytest.raises(ValueError):
            env.place_at_distance(table, **kw)
    with pytest.raises(ValueError):
        env.place_at_distance(table, rows=torch.zeros(n - 1, dtype=torch.int32))
    pos = env.positions.clone()
    assert int(env.place_at_distance(table, 5, 3).count.sum()) == 0 and torch.equal(env.positions, pos)       # an empty band is no error
    env.close()
    with pytest.raises(RuntimeError):
        env.place_at_distance(table)
