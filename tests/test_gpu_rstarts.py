"""ts_rstarts_index and ts_rstarts_place on the GPU, exact equality everywhere, against the NumPy definition
(tests/rstarts_reference.py) and, for the index, against torch.sort of the table.  Every raw call works on memory the test owns:
outputs lie between 256 guard bytes; the index is prefilled with 0xA5, the placement's outputs with the complement of the
yardstick's answer, and the whole buffer - guards, arrays the call may not write, boards that are not placed - is compared byte
for byte with the same buffer built from the yardstick's answer."""
import ctypes as C
import functools

import numpy as np
import pytest

import reach_cases as cases
import rstarts_reference as rs
import starts_reference as sref
from table_harness import GUARD, GUARD_BYTE, guarded as _guarded, payload as _payload

pytestmark = pytest.mark.gpu

SEED = 0xF00DFACE12345678      # above 2^63: the seed is unsigned
SIZES = (2, 3, 5, 8)
BOARDS = (1, 63, 257)
BANDS = ((0, 0), (1, 252), (2, 4), (5, 3), (100, 252), "per board")
FLOOR = 10                     # levels of a case that hold a placement in a band: tests/test_rstarts_cpu.py checks it on the CPU


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _oracle():
    from oracle import binding
    return binding


def _env(S, mc, blk, init, tgt, **kw):
    from tiler_slider_amd import VecTilerSliderEnv
    kw.setdefault("obs_dtype", None)
    return VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=mc, **kw)


def _u64(t):
    """An int64 tensor as the uint64 words it holds."""
    return t.cpu().numpy().view(np.uint64)


def _index_raw(torch, table, count, W):
    """ts_rstarts_index into buffers of 0xA5 between guards: (sorted uint64 [L, W], first int32 [L, 256]); the inputs are compared
    with what they held."""
    from tiler_slider_amd import _rstarts_cabi as xs
    L, slots = table.shape
    dev = table.device
    sbuf = torch.full((2 * GUARD + L * W * 8,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    fbuf = torch.full((2 * GUARD + L * xs.FIRST * 4,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    t0, c0 = table.clone(), count.clone()
    rc = xs.lib().ts_rstarts_index(table.data_ptr(), slots, count.data_ptr(), L, W, sbuf.data_ptr() + GUARD, fbuf.data_ptr() + GUARD,
                                   torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    out = _payload(sbuf, np.uint64, (L, W)), _payload(fbuf, np.int32, (L, xs.FIRST))
    assert torch.equal(table, t0) and torch.equal(count, c0)
    return out


def _by_torch_sort(torch, table, count, W):
    """What the parent commit offers: torch.sort of the rows - as int64 the occupied words are negative and come first, in their
    unsigned order -, a slice, and the lower bounds of the distances."""
    srt = torch.sort(table, dim=1).values[:, :W].clone()
    ok = ((count >= 0) & (count <= W)).unsqueeze(1)
    srt = torch.where(ok & (srt < 0), srt, torch.zeros_like(srt))
    entry = torch.where(srt < 0, (srt >> 48) & 0xFF, torch.full_like(srt, 256))
    first = torch.searchsorted(entry.contiguous(), torch.arange(256, device=table.device).repeat(table.shape[0], 1))
    return _u64(srt), first.to(torch.int32).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ the index
@pytest.mark.parametrize("mc", (False, True))
@pytest.mark.parametrize("S", SIZES)
def test_the_index_is_the_yardsticks_and_torch_sorts(torch_cuda, oracle, S, mc):
    """The levels of reach_cases at capacity 1,024, FULL levels and won roots among them: the same words in the same order from
    the kernel, the yardstick and torch.sort; and two builds of the table give the same index bits."""
    torch = torch_cuda
    blk, init, tgt, ref, want_sorted, want_first = rs.case(oracle, S, mc)
    assert S < 3 or ((ref.count < 0).sum() >= 3 and (ref.count == 0).sum() >= 3)
    env = _env(S, mc, blk, init, tgt)
    rtab = env.build_reach_table(capacity=cases.CAPACITY)
    np.testing.assert_array_equal(rtab.count.cpu().numpy(), ref.count)
    got_sorted, got_first = _index_raw(torch, rtab.table, rtab.count, cases.CAPACITY)
    np.testing.assert_array_equal(got_sorted, want_sorted)
    np.testing.assert_array_equal(got_first, want_first)
    by_sort = _by_torch_sort(torch, rtab.table, rtab.count, cases.CAPACITY)
    np.testing.assert_array_equal(got_sorted, by_sort[0])
    np.testing.assert_array_equal(got_first, by_sort[1])
    # through the wrapper, and from another build of the same table
    a, b = env.build_reach_index(rtab), env.build_reach_index(env.build_reach_table(capacity=cases.CAPACITY))
    assert torch.equal(a.sorted, b.sorted) and torch.equal(a.first, b.first) and len(a) == cases.DISTINCT and a.capacity == cases.CAPACITY
    np.testing.assert_array_equal(_u64(a.sorted), want_sorted)
    np.testing.assert_array_equal(a.first.cpu().numpy(), want_first)
    for lo, hi in ((1, 252), (2, 4), (1, 1), (5, 3), (0, 0), (100, 300)):
        np.testing.assert_array_equal(a.band_count(lo, hi).cpu().numpy(), rs.place(want_sorted, want_first, S * S, 0, cases.DISTINCT, lo, min(hi, 252))["count"])


def _host_rows(torch, dev, sizes, capacity, seed):
    """One host-filled row per size - synthetic (key, entry) pairs in slots = pow2ceil(2 * capacity) -, the yardstick's index of
    each, and the launch's."""
    slots = 2
    while slots < 2 * capacity:
        slots *= 2
    rows, want_sorted, want_first = [], [], []
    for i, n in enumerate(sizes):
        keys, entries = rs.synthetic_pairs(n, seed + i)
        rows.append(rs.fill_row(keys, entries, slots))
        s, f = rs.index_of_pairs(keys, entries, capacity)
        want_sorted.append(s)
        want_first.append(f)
    table = torch.from_numpy(np.stack(rows).view(np.int64)).to(dev)
    count = torch.tensor(list(sizes), dtype=torch.int32, device=dev)
    got = _index_raw(torch, table, count, capacity)
    return got, (np.stack(want_sorted), np.stack(want_first)), table, count


def test_host_filled_rows_at_the_padding_edges_of_the_network(torch_cuda):
    torch = torch_cuda
    dev = torch.device("cuda", torch.cuda.current_device())
    sizes = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 4095, 4096)
    got, want, table, count = _host_rows(torch, dev, sizes, 4096, 100)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    by_sort = _by_torch_sort(torch, table, count, 4096)
    np.testing.assert_array_equal(got[0], by_sort[0])
    np.testing.assert_array_equal(got[1], by_sort[1])


def test_both_forms_of_the_index_on_either_side_of_the_threshold(torch_cuda):
    """Capacity 65,536 takes k_rstarts_index<true>: levels up to lds_states are sorted in LDS, larger ones in their own row."""
    torch = torch_cuda
    from tiler_slider_amd import _rstarts_cabi as xs
    dev = torch.device("cuda", torch.cuda.current_device())
    W = 65536
    d = xs.describe_rstarts_index(5, 2 * W, W)
    lds = d["lds_states"]
    assert d["form"] == xs.FORM_GLOBAL and d["name"] == "k_rstarts_index<true>" and 64 <= lds < 20000
    sizes = (lds - 1, lds, lds + 1, 20000, W)
    got, want, table, count = _host_rows(torch, dev, sizes, W, 200)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    # a count that is not the row's: FULL, and one above the width - empty indices, whatever the rows hold
    for bad in (-3, W + 1):
        count2 = count.clone()
        count2[1::2] = bad
        again = _index_raw(torch, table, count2, W)
        np.testing.assert_array_equal(again[0][0::2], want[0][0::2])
        assert not again[0][1::2].any() and not again[1][1::2].any()


def test_a_real_level_of_tens_of_thousands_of_states(torch_cuda, oracle):
    """6x6 / 5 tiles / 6 obstacles at capacity 65,536, the levels of tests/test_gpu_reach_occupancy.py: against torch.sort."""
    torch = torch_cuda
    S, T, K = 6, 5, 6
    blk, init, _ = oracle.generate_mt19937(S, T, T, K, np.arange(8, dtype=np.uint32))
    tgt = cases.walked(oracle, S, blk, init, 14)
    env = _env(S, True, blk, init, tgt)
    rtab = env.build_reach_table(capacity=65536)
    count = rtab.count.cpu().numpy()
    print("states per level:", count.tolist())
    assert (count > 2 * 4096).any() and (count >= 0).all()
    got = _index_raw(torch, rtab.table, rtab.count, 65536)
    by_sort = _by_torch_sort(torch, rtab.table, rtab.count, 65536)
    np.testing.assert_array_equal(got[0], by_sort[0])
    np.testing.assert_array_equal(got[1], by_sort[1])
    assert got[1][:, 253].max() >= 1000      # distances, not only TABLE_NONE
    index = env.build_reach_index(rtab)
    np.testing.assert_array_equal(_u64(index.sorted), got[0])


def _check_kept(row_in, sorted_out, first_out, at_most):
    """What the header promises over arbitrary bytes: the kept words are occupied words of the row, no more of each than the row
    holds and at most `at_most` in all, in ascending order, zeros behind them; `first` is their lower bounds."""
    m = int((sorted_out != 0).sum())
    kept = sorted_out[:m]
    assert m <= at_most and not sorted_out[m:].any() and (kept >> np.uint64(63)).all() and (kept[1:] >= kept[:-1]).all()
    words, held = np.unique(row_in[(row_in >> np.uint64(63)) != 0], return_counts=True)
    mine, n_mine = np.unique(kept, return_counts=True)
    at = np.searchsorted(words, mine)
    assert (at < len(words)).all() and (words[np.minimum(at, len(words) - 1)] == mine).all() and (n_mine <= held[at]).all()
    masked = kept & ~rs.OCC
    np.testing.assert_array_equal(first_out, np.searchsorted(masked, np.arange(256, dtype=np.uint64) << np.uint64(48), side="left"))
    return m


def test_a_full_grid_a_ragged_second_pass_and_rows_of_arbitrary_bytes(torch_cuda, oracle):
    torch = torch_cuda
    from tiler_slider_amd import _rstarts_cabi as xs
    dev = torch.device("cuda", torch.cuda.current_device())
    S, mc = 5, True
    blk, init, tgt, ref, want_sorted, want_first = rs.case(oracle, S, mc)
    rtab = _env(S, mc, blk, init, tgt).build_reach_table(capacity=cases.CAPACITY)
    which = torch.arange(cases.N_BUILD, device=dev) % cases.DISTINCT
    assert cases.N_BUILD == 1085 and xs.describe_rstarts_index(cases.N_BUILD, rtab.slots, cases.CAPACITY)["blocks"] == 1024
    got = _index_raw(torch, rtab.table[which].contiguous(), rtab.count[which].contiguous(), cases.CAPACITY)
    np.testing.assert_array_equal(got[0], want_sorted[which.cpu().numpy()])
    np.testing.assert_array_equal(got[1], want_first[which.cpu().numpy()])
    # rows nobody built: the call ends, the guards are intact (_index_raw), what is kept is of the row
    rng = np.random.default_rng(12)
    lds = xs.describe_rstarts_index(1, 2, 1)["lds_states"]
    for W, slots in ((1024, 2048), (2 * lds, 4 * lds)):
        rows = np.stack([np.zeros(slots, np.uint64), np.full(slots, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(slots, 2 ** 64 - 1, np.uint64),
                         rng.integers(0, 2 ** 64, slots, dtype=np.uint64), rng.integers(0, 2 ** 64, slots, dtype=np.uint64)])
        table = torch.from_numpy(rows.view(np.int64)).to(dev)
        for counts in ((0, 0, 0, 0, 0), (5, W, W, W, 7), (W, 1, lds, lds + 1, W), (-3, W + 1, -1, 2 ** 31 - 1, -2 ** 31)):
            out = _index_raw(torch, table, torch.tensor(counts, dtype=torch.int32, device=dev), W)
            for i, c in enumerate(counts):
                if not 0 <= c <= W:
                    assert not out[0][i].any() and not out[1][i].any()
                    continue
                m = _check_kept(rows[i], out[0][i], out[1][i], W)
                occupied = int((rows[i] >> np.uint64(63)).sum())
                assert m == min(occupied, W if c > lds else min(W, lds)), (W, counts, i, m, occupied)


# ------------------------------------------------------------------------------------------------------------- the placement
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

    def get(self, host, name):
        off, dtype, shape = self.at[name]
        return host[off:off + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)

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


def _raw_place(torch, dev, dims, arena, buf, index, W, n_rows, cfg_kw, use_rows, use_band, outputs=("count", "dist", "deepest"), with_state=True):
    from tiler_slider_amd import _cabi, _rstarts_cabi as xs
    st = _cabi.State(arena.ptr(buf, "pos"), arena.ptr(buf, "init"), None, None, arena.ptr(buf, "step_count"), arena.ptr(buf, "done"), None)
    cfg = xs.StartsCfg(band=arena.ptr(buf, "band") if use_band else None, reserved=0, **cfg_kw)
    out = xs.StartsOut(**{k: arena.ptr(buf, k) for k in outputs})
    srt, first = index if index is not None else (None, None)
    return xs.lib().ts_rstarts_place(C.byref(dims), C.byref(st) if with_state else None, srt.data_ptr() + GUARD if srt is not None else None,
                                     first.data_ptr() + GUARD if first is not None else None, W, n_rows, arena.ptr(buf, "rows") if use_rows else None,
                                     C.byref(cfg), C.byref(out), torch.cuda.current_stream(dev).cuda_stream)


def _state(rng, C_, T, N, ref=None):
    """A state nobody reset: random cells, counters and flags; where the answers go, the complement of the yardstick's (random
    bytes where there is none)."""
    want = ref if ref is not None else dict(count=rng.integers(-9, 9, N), dist=rng.integers(0, 256, N), deepest=rng.integers(0, 256, N))
    return dict(pos=rng.integers(0, C_, (T, N)).astype(np.uint8), init=rng.integers(0, C_, (T, N)).astype(np.uint8),
                step_count=rng.integers(1, 100, N).astype(np.int32), done=rng.integers(0, 2, N).astype(np.uint8),
                count=~want["count"].astype(np.int32), dist=~want["dist"].astype(np.uint8), deepest=~want["deepest"].astype(np.uint8),
                band=np.zeros((2, N), np.uint8), rows=np.zeros(N, np.int32))


def _after(before, ref, write_pos, write_init):
    after = dict(before)
    after["pos"], after["init"], after["step_count"], after["done"] = sref.apply(ref, before["pos"], before["init"], before["step_count"], before["done"],
                                                                                write_pos, write_init)
    after["count"], after["dist"], after["deepest"] = ref["count"], ref["dist"], ref["deepest"]
    return after


def _upload(torch, dev, srt, first):
    return _guarded(torch, dev, srt), _guarded(torch, dev, first)


def _per_board_band(rng, N, top=12):
    band = rng.integers(0, top, (2, N)).astype(np.uint8)
    band[1, ::2] = np.maximum(band[1, ::2], band[0, ::2])     # half of the bands are not empty
    band[1, ::5] = rng.integers(253, 256, len(band[1, ::5]))  # bytes above the largest distance
    band[0, 3::7] = rng.integers(253, 256, len(band[0, 3::7]))
    return band


@pytest.mark.parametrize("N", BOARDS)
@pytest.mark.parametrize("S", SIZES)
def test_the_placement_through_the_raw_abi(torch_cuda, oracle, S, N):
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _rstarts_cabi as xs
    dev = torch.device("cuda", torch.cuda.current_device())
    T, C_, W = cases.SHAPES[S][0], S * S, cases.CAPACITY
    _, _, _, _, full_sorted, full_first = rs.case(oracle, S, True)
    rng = np.random.default_rng(1000 * S + N)
    placed_total = unplaced_total = 0
    dims = _cabi.Dims(N, S, T, T, 1, 100, 0)
    for case in ("rows=None", "rows with repeats", "rows out of range"):
        rows = None
        if case == "rows=None":       # board n reads row n: the levels that hold most, first
            order = np.argsort(-full_first[:, 253], kind="stable")[np.arange(N) % cases.DISTINCT]
            srt, first = full_sorted[order], full_first[order]
        else:
            srt, first = full_sorted, full_first
            rows = rng.integers(0, cases.DISTINCT, N).astype(np.int32)
            if case == "rows out of range":
                rows[rng.integers(0, N)] = cases.DISTINCT
                rows[rng.integers(0, N)] = -1
        n_rows = srt.shape[0]
        index = _upload(torch, dev, srt, first)
        for band_case in BANDS:
            band = _per_board_band(rng, N) if band_case == "per board" else None
            lo, hi = (1, 252) if band_case == "per board" else band_case
            ref = rs.place(srt, first, C_, T, N, lo, hi, band=band, rows=rows, seed=SEED, step_index=5, board_offset=1000)
            if band_case in ((0, 0), (5, 3), (100, 252)):
                assert not ref["placed"].any()     # a reach table stores no won placement; the deepest entry of the cases is 45
            placed_total += int(ref["placed"].sum())
            unplaced_total += int((~ref["placed"]).sum())
            before = _state(rng, C_, T, N, ref)
            if band is not None:
                before["band"] = band
            if rows is not None:
                before["rows"] = rows
            arena = _Arena(before)
            for write_pos in (0, 1):
                for write_init in (0, 1):
                    buf = torch.from_numpy(arena.build(before)).to(dev)
                    kw = dict(lo=lo, hi=hi, where=xs.ALL, write_pos=write_pos, write_init=write_init, seed=SEED, step_index=5, board_offset=1000)
                    rc = _raw_place(torch, dev, dims, arena, buf, index, W, n_rows, kw, rows is not None, band is not None)
                    assert rc == 0, rc
                    bad = arena.differing(buf.cpu().numpy(), arena.build(_after(before, ref, write_pos, write_init)))
                    assert not bad, (S, N, case, band_case, write_pos, write_init, bad)
        np.testing.assert_array_equal(_payload(index[0], np.uint64, srt.shape), srt)
        np.testing.assert_array_equal(_payload(index[1], np.int32, first.shape), first)
    assert placed_total > 0 and unplaced_total > 0


def test_starts_done_places_exactly_the_boards_that_are_done(torch_cuda, oracle):
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _rstarts_cabi as xs
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(77)
    for S, N in ((5, 257), (3, 63), (8, 130)):
        T, C_ = cases.SHAPES[S][0], S * S
        _, _, _, _, srt, first = rs.case(oracle, S, True)
        rows = rng.integers(0, cases.DISTINCT, N).astype(np.int32)
        index = _upload(torch, dev, srt, first)
        done = (rng.integers(0, 3, N) * 127).astype(np.uint8)      # 0, 127 or 254: any byte but 0 is done
        sel = done != 0
        ref = rs.place(srt, first, C_, T, N, 1, 9, rows=rows, selected=sel, seed=3, step_index=2)
        assert ref["placed"][sel & (ref["count"] > 0)].all() and not ref["placed"][~sel].any()
        assert ref["placed"].sum() >= 5 and (~sel).sum() >= N // 5 and (ref["count"][~sel] > 0).any() and (sel & (ref["count"] == 0)).any()
        before = _state(rng, C_, T, N, ref)
        before["done"], before["rows"] = done, rows
        arena = _Arena(before)
        buf = torch.from_numpy(arena.build(before)).to(dev)
        kw = dict(lo=1, hi=9, where=xs.DONE, write_pos=1, write_init=1, seed=3, step_index=2, board_offset=0)
        assert _raw_place(torch, dev, _cabi.Dims(N, S, T, T, 1, 100, 0), arena, buf, index, cases.CAPACITY, cases.DISTINCT, kw, True, False) == 0
        after = _after(before, ref, 1, 1)
        assert not arena.differing(buf.cpu().numpy(), arena.build(after)), (S, N)
        assert (after["done"][ref["placed"]] == 0).all() and (after["done"][sel & ~ref["placed"]] != 0).all()


def test_an_index_nobody_built_is_read_inside_its_buffers(torch_cuda):
    """`first` of arbitrary words - above W, negative, decreasing - and `sorted` of arbitrary words: every cell written is below C,
    every count is 0 .. W, the guards are intact."""
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _rstarts_cabi as xs
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(31)
    for S, T, W, n_rows, N in ((3, 5, 7, 9, 257), (5, 6, 64, 5, 300), (8, 8, 1, 3, 63), (1, 1, 5, 4, 70), (7, 6, 33, 6, 129)):
        C_ = S * S
        srt = rng.integers(0, 2 ** 64, (n_rows, W), dtype=np.uint64)
        first = rng.integers(-2 ** 31, 2 ** 31, (n_rows, 256)).astype(np.int32)
        first[0] = rng.integers(-3, W + 4, 256)          # around the edges of the row
        first[1] = np.sort(rng.integers(0, W + 1, 256))  # as a built one
        index = _upload(torch, dev, srt, first)
        before = _state(rng, C_, T, N)
        before["band"], before["rows"] = rng.integers(0, 256, (2, N)).astype(np.uint8), rng.integers(-1, n_rows + 1, N).astype(np.int32)
        arena = _Arena(before)
        buf = torch.from_numpy(arena.build(before)).to(dev)
        kw = dict(lo=1, hi=252, where=xs.ALL, write_pos=1, write_init=1, seed=S, step_index=0, board_offset=0)
        assert _raw_place(torch, dev, _cabi.Dims(N, S, T, T, 1, 100, 0), arena, buf, index, W, n_rows, kw, True, True) == 0
        host = buf.cpu().numpy()
        want = arena.build(before)
        assert arena.differing(host, want) != [] and "guard" not in arena.differing(host, want) and "band" not in arena.differing(host, want)
        count, dist = arena.get(host, "count"), arena.get(host, "dist")
        assert (arena.get(host, "pos") < C_).all() and (arena.get(host, "init") < C_).all() and ((count >= 0) & (count <= W)).all()
        placed = dist != 255
        assert placed.any() and np.array_equal(arena.get(host, "pos")[:, ~placed & (count == 0)], before["pos"][:, ~placed & (count == 0)])
        assert (arena.get(host, "step_count")[count > 0] == 0).all()
        np.testing.assert_array_equal(_payload(index[0], np.uint64, srt.shape), srt)
        np.testing.assert_array_equal(_payload(index[1], np.int32, first.shape), first)


def test_empty_inputs_launch_nothing_and_write_nothing(torch_cuda, oracle):
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _rstarts_cabi as xs
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(5)
    S, T = 5, cases.SHAPES[5][0]
    _, _, _, _, srt, first = rs.case(oracle, S, True)
    before = _state(rng, S * S, T, 63)
    arena = _Arena(before)
    index = _upload(torch, dev, srt[:63], first[:63])
    kw = dict(lo=1, hi=252, where=xs.ALL, write_pos=1, write_init=1, seed=1, step_index=0, board_offset=0)
    for n_boards, n_rows, idx in ((0, 63, index), (63, 0, index), (63, 0, None), (0, 0, None)):
        buf = torch.from_numpy(arena.build(before)).to(dev)
        assert _raw_place(torch, dev, _cabi.Dims(n_boards, S, T, T, 1, 100, 0), arena, buf, idx, cases.CAPACITY, n_rows, kw, False, False) == 0
        assert np.array_equal(buf.cpu().numpy(), arena.build(before)), (n_boards, n_rows)
    assert _raw_place(torch, dev, _cabi.Dims(0, S, T, T, 1, 100, 0), arena, buf, None, 1, 0, kw, False, False, outputs=(), with_state=False) == 0
    assert xs.lib().ts_rstarts_index(None, 2, None, 0, 1, None, None, None) == 0
    assert xs.lib().ts_rstarts_last_hip_error() == 0


@pytest.mark.parametrize("name", sorted(rs.occupancy_cases()))
def test_every_compiled_placement_kernel_at_occupancy(torch_cuda, oracle, name):
    """Every k_rstarts_place<S> at 262,141 boards - 4,096 waves, the last one ragged - through rows= onto the 128 levels of
    reach_cases, a band per board: every byte of state, outputs and guards against the yardstick's."""
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _rstarts_cabi as xs
    dev = torch.device("cuda", torch.cuda.current_device())
    S, T, _ = rs.occupancy_cases()[name]
    C_, N = S * S, rs.N_OCC
    _, _, _, _, srt, first = rs.case(oracle, S, True)
    dims = _cabi.Dims(N, S, T, T, 1, 100, 0)
    d = xs.describe_rstarts_place(dims)
    assert d["name"] == name and d["blocks"] * d["threads_per_block"] // 64 == 4096 and N % 64 != 0
    rng = np.random.default_rng(0x0CC + S)
    rows = rng.integers(0, cases.DISTINCT, N).astype(np.int32)
    rows[rng.integers(0, N, 8)] = np.array([-1, cases.DISTINCT] * 4, np.int32)
    band = _per_board_band(rng, N)
    ref = rs.place_many(srt, first, C_, T, N, band=band, rows=rows, seed=SEED, step_index=5, board_offset=1000)
    placed = int(ref["placed"].sum())
    print(f"{name}: {N} boards in {d['blocks']} blocks, {placed} placed, {N - placed} not, counts up to {ref['count'].max()}")
    assert N - placed >= 64 and (S < 3 or placed >= 1000)
    index = _upload(torch, dev, srt, first)
    before = _state(rng, C_, T, N, ref)
    before["band"], before["rows"] = band, rows
    arena = _Arena(before)
    buf = torch.from_numpy(arena.build(before)).to(dev)
    kw = dict(lo=1, hi=252, where=xs.ALL, write_pos=1, write_init=1, seed=SEED, step_index=5, board_offset=1000)
    assert _raw_place(torch, dev, dims, arena, buf, index, cases.CAPACITY, cases.DISTINCT, kw, True, True) == 0
    bad = arena.differing(buf.cpu().numpy(), arena.build(_after(before, ref, 1, 1)))
    assert not bad, (name, bad)


# ------------------------------------------------------------------------------------------------------------- the environment
REAL = ((5, 4, 3), (8, 3, 10))
N_REAL, REAL_CAPACITY = 96, 4096


@functools.lru_cache(maxsize=None)
def _real(S, T, K, mc=True):
    """(blk, init, tgt, Reference, sorted, first): 96 seeded levels, the odd-numbered ones with their targets where ten moves leave
    the tiles - random levels of these shapes can hardly ever be won -, solved once on the CPU."""
    import rtable_reference as rt
    orc = _oracle()
    blk, init, tgt = orc.generate_mt19937(S, T, T, K, np.arange(N_REAL, dtype=np.uint32))
    tgt = tgt.copy()
    tgt[:, 1::2] = cases.walked(orc, S, blk, init)[:, 1::2]
    ref = rt.build(orc, S, mc, blk, tgt, init, 252, REAL_CAPACITY)
    return (blk, init, np.ascontiguousarray(tgt), ref) + rs.index(ref, REAL_CAPACITY)


def _placed_env(S, mc, blk, init, tgt, **kw):
    env = _env(S, mc, blk, init, tgt, **kw)
    env.reset()
    rtab = env.build_reach_table(capacity=REAL_CAPACITY)
    return env, rtab, env.build_reach_index(rtab)


@pytest.mark.parametrize("S,T,K", REAL)
@pytest.mark.parametrize("lo,hi", ((1, 252), (2, 4)))
def test_boards_are_placed_where_the_lookup_reads_the_same_distance(torch_cuda, S, T, K, lo, hi):
    torch = torch_cuda
    blk, init, tgt, ref, srt, first = _real(S, T, K)
    n = N_REAL
    want = rs.place(srt, first, S * S, T, n, lo, hi, seed=0xBEEF, step_index=1)
    print(f"{S}x{S} / {T} band [{lo}, {hi}]: {want['placed'].sum()} of {n} boards are placed, {(ref.count < 0).sum()} levels FULL")
    assert FLOOR <= want["placed"].sum() <= n - FLOOR
    env, rtab, ridx = _placed_env(S, True, blk, init, tgt)
    np.testing.assert_array_equal(_u64(ridx.sorted), srt)
    info = env.place_at_distance(ridx, lo, hi, seed=0xBEEF, step_index=1)
    assert (info.count.dtype, info.dist.dtype, info.deepest.dtype, info.placed.dtype) == (torch.int32, torch.uint8, torch.uint8, torch.bool)
    for name in ("count", "dist", "deepest", "placed"):
        np.testing.assert_array_equal(getattr(info, name).cpu().numpy(), want[name], err_msg=name)
    p = want["placed"]
    pos = env.positions.cpu().numpy()
    np.testing.assert_array_equal(pos[:, p], want["cells"][:, p])
    np.testing.assert_array_equal(pos[:, ~p], init[:, ~p])                       # not placed: where they stood
    np.testing.assert_array_equal(env._init.cpu().numpy(), np.where(p, want["cells"], init))
    moves = env.lookup(rtab)[0].cpu().numpy()
    np.testing.assert_array_equal(moves[p], want["dist"][p].astype(np.int16))    # on every placed board
    assert ((moves[p] >= lo) & (moves[p] <= hi)).all()
    # set_initial=False moves the boards and leaves the level's start alone; rows= reads the same rows in another order
    env2 = _env(S, True, blk[:, ::-1], init[:, ::-1], tgt[:, ::-1])
    env2.reset()
    back = torch.arange(n - 1, -1, -1, dtype=torch.int32, device=env2.device)
    info2 = env2.place_at_distance(ridx, lo, hi, rows=back, seed=0xBEEF, step_index=1, set_initial=False)
    want2 = rs.place(srt, first, S * S, T, n, lo, hi, rows=np.arange(n)[::-1], seed=0xBEEF, step_index=1)
    np.testing.assert_array_equal(info2.count.cpu().numpy(), want["count"][::-1])
    np.testing.assert_array_equal(info2.dist.cpu().numpy(), want2["dist"])
    np.testing.assert_array_equal(env2.positions.cpu().numpy(), np.where(want2["placed"], want2["cells"], init[:, ::-1]))
    np.testing.assert_array_equal(env2._init.cpu().numpy(), init[:, ::-1])


@pytest.mark.parametrize("kind", ("float32", "uint8", "none", "inplace"))
def test_the_observation_and_the_restart_follow_the_placement(torch_cuda, oracle, kind):
    """An environment placed with set_initial=True is, from then on, the environment built on the placed cells: six steps in
    auto-reset mode with three moves per episode - every board finishes and restarts - against that twin."""
    torch = torch_cuda
    from tiler_slider_amd import _cabi
    S, T, K = REAL[0]
    blk, init, tgt, ref, srt, first = _real(S, T, K)
    n = N_REAL
    kw = dict(max_steps=3, auto_reset=True, obs_dtype=None if kind == "none" else "float32" if kind == "inplace" else kind,
              obs_update="inplace" if kind == "inplace" else "auto")
    env, rtab, ridx = _placed_env(S, True, blk, init, tgt, **kw)
    assert env._in_place == (kind == "inplace")
    for k in range(2):       # the buffer shows other cells than the start's when the boards are placed
        env.step(torch.from_numpy(oracle.fill_actions(n, seed=9, step_index=k)))
    env.reset()
    flags_before = env._flags.clone()
    info = env.place_at_distance(ridx, 1, 252, seed=0x0B5, set_initial=True)
    assert torch.equal(env._flags, flags_before)                               # the last step's info is left as it is
    want = rs.place(srt, first, S * S, T, n, 1, 252, seed=0x0B5)
    placed_init = np.where(want["placed"], want["cells"], init)
    assert want["placed"].sum() >= FLOOR and (placed_init != init).any()
    np.testing.assert_array_equal(info.placed.cpu().numpy(), want["placed"])
    twin = _env(S, True, blk, placed_init, tgt, **kw)
    shown = twin.reset()
    if kind != "none":
        assert torch.equal(env._obs, shown), "the buffer shows the placed cells"
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


def test_same_bits_on_every_run_and_another_step_index_draws_again(torch_cuda):
    torch = torch_cuda
    S, T, K = REAL[0]
    blk, init, tgt, ref, srt, first = _real(S, T, K)
    env, rtab, ridx = _placed_env(S, True, blk, init, tgt)
    runs = []
    for step_index in (0, 0, 1):
        env._pos.copy_(env._init)
        info = env.place_at_distance(ridx, 1, 252, seed=21, step_index=step_index, set_initial=False)
        runs.append([t.clone() for t in (info.count, info.dist, info.deepest, info.placed, env.positions)])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert torch.equal(runs[0][0], runs[2][0]) and torch.equal(runs[0][2], runs[2][2]) and torch.equal(runs[0][3], runs[2][3])
    assert not torch.equal(runs[0][4], runs[2][4])        # the draw changed; count, deepest and who is placed did not
    # board_offset shifts the stream
    want = rs.place(srt, first, S * S, T, N_REAL, 1, 252, seed=21, board_offset=100)
    env._pos.copy_(env._init)
    info = env.place_at_distance(ridx, 1, 252, seed=21, board_offset=100, set_initial=False)
    np.testing.assert_array_equal(info.dist.cpu().numpy(), want["dist"])
    np.testing.assert_array_equal(env.positions.cpu().numpy(), np.where(want["placed"], want["cells"], init))


def test_band_per_board_and_only_done_through_the_wrapper(torch_cuda, oracle):
    torch = torch_cuda
    S, T, K = REAL[0]
    blk, init, tgt, ref, srt, first = _real(S, T, K)
    n = N_REAL
    env, rtab, ridx = _placed_env(S, True, blk, init, tgt, max_steps=2)
    for k in range(2):
        env.step(torch.from_numpy(oracle.fill_actions(n, seed=4, step_index=k)))
    assert bool(env.done.all())                       # strict mode, two moves per episode: everything is done
    env._done[::3] = 0
    done = env.done.cpu().numpy()
    rng = np.random.default_rng(8)
    band = np.sort(rng.integers(0, 8, (2, n)), axis=0).astype(np.uint8)
    pos, steps = env.positions.cpu().numpy().copy(), env.step_count.cpu().numpy().copy()
    info = env.place_at_distance(ridx, band=torch.from_numpy(band).to(env.device), seed=6, only_done=True, set_initial=False)
    want = rs.place(srt, first, S * S, T, n, band=band, selected=done, seed=6)
    assert want["placed"].sum() >= FLOOR and not want["placed"][::3].any()
    for name in ("count", "dist", "deepest", "placed"):
        np.testing.assert_array_equal(getattr(info, name).cpu().numpy(), want[name], err_msg=name)
    after = sref.apply(want, pos, init, steps, done.astype(np.uint8), True, False)
    np.testing.assert_array_equal(env.positions.cpu().numpy(), after[0])
    np.testing.assert_array_equal(env.step_count.cpu().numpy(), after[2])
    np.testing.assert_array_equal(env.done.cpu().numpy(), after[3] != 0)
    np.testing.assert_array_equal(env._init.cpu().numpy(), init)


def test_the_wrapper_refuses_what_it_cannot_place(torch_cuda):
    torch = torch_cuda
    from tiler_slider_amd import ReachIndex, VecTilerSliderEnv
    S, T, K = REAL[0]
    blk, init, tgt, ref, srt, first = _real(S, T, K)
    env, rtab, ridx = _placed_env(S, True, blk, init, tgt)
    assert isinstance(ridx, ReachIndex) and "96 levels" in repr(ridx) and ridx.shape_key == rtab.shape_key
    other = VecTilerSliderEnv.random(N_REAL, size=4, num_tiles=2, num_obstacles=2, obs_dtype=None)
    with pytest.raises(ValueError, match="built for"):
        other.place_at_distance(ridx)                                        # an index of another shape
    with pytest.raises(ValueError, match="built for"):
        other.build_reach_index(rtab)
    elsewhere = ReachIndex(ridx.sorted.cpu(), ridx.first.cpu(), ridx.capacity, *ridx.shape_key)
    with pytest.raises(ValueError, match="lives on"):
        env.place_at_distance(elsewhere)                                     # another device
    with pytest.raises(TypeError, match="DistanceTable"):
        env.place_at_distance(rtab)                                          # a bare ReachTable
    with pytest.raises(TypeError, match="build_reach_index"):
        env.place_at_distance(rtab)
    with pytest.raises(TypeError, match="ReachTable"):
        env.build_reach_index(ridx)
    with pytest.raises(ValueError, match="max_bytes"):
        env.build_reach_index(rtab, max_bytes=1 << 20)
    n = env.num_envs
    good = torch.ones((2, n), dtype=torch.uint8, device=env.device)
    for band in (good[:, :-1], good[0], good.to(torch.int32), good.cpu()):
        with pytest.raises(ValueError):
            env.place_at_distance(ridx, band=band)
    for kw in (dict(min_moves=-1), dict(min_moves=253), dict(max_moves=253), dict(max_moves=-1)):
        with pytest.raises(ValueError):
            env.place_at_distance(ridx, **kw)
    with pytest.raises(ValueError):
        env.place_at_distance(ridx, rows=torch.zeros(n - 1, dtype=torch.int32))
    pos = env.positions.clone()
    assert int(env.place_at_distance(ridx, 5, 3).count.sum()) == 0 and torch.equal(env.positions, pos)       # an empty band is no error
    assert int(env.place_at_distance(ridx, 0, 0).count.sum()) == 0 and torch.equal(env.positions, pos)       # no won placement is stored
    env.close()
    with pytest.raises(RuntimeError):
        env.place_at_distance(ridx)


@pytest.mark.parametrize("S,T,K", REAL)
def test_a_curriculum_round_trip(torch_cuda, S, T, K):
    """Boards that are done are put one or two moves from the win; the table's expert, without exploration, then wins every one
    of them within two moves."""
    torch = torch_cuda
    blk, init, tgt, ref, srt, first = _real(S, T, K)
    n = N_REAL
    env, rtab, ridx = _placed_env(S, True, blk, init, tgt, max_steps=4)
    env.rollout(4, "random", seed=3)
    assert bool(env.done.all())                      # strict mode, four moves per episode
    info = env.place_at_distance(ridx, 1, 2, seed=12, only_done=True)
    placed = info.placed
    assert int(placed.sum()) >= FLOOR and int((~placed).sum()) >= FLOOR
    assert not bool(env.done[placed].any()) and bool(env.done[~placed].all())
    out = env.rollout(2, "reach", table=rtab, epsilon=0.0, seed=5)
    assert torch.equal(out.wins[placed], torch.ones_like(out.wins[placed]))
    assert torch.equal(out.first_win[placed].to(torch.uint8), info.dist[placed])      # in exactly `dist` moves
    assert int(out.wins[~placed].sum()) == 0
