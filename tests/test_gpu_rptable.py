"""The reach policy tables on the GPU (lib/libtiler_slider_rptable.so), exact equality everywhere, against the NumPy definition
(tests/rptable_reference.py).  Every raw call writes into ONE buffer the test owns - act, logits, the output table, root_moves,
deepest and score between guard bytes - prefilled with the complement of the expected bytes, and the whole buffer is compared with
the same buffer built from the yardstick's answer: every byte is written, and none beside.  tests/test_rptable_cpu.py asserts, on
the yardstick alone, that the inputs used here are not degenerate."""
import ctypes as C

import numpy as np
import pytest

import policy_reference as pref
import reach_cases as cases
import rptable_reference as xr
import rstarts_reference as rs
import rtable_reference as rt
from table_harness import GUARD, GUARD_BYTE

pytestmark = pytest.mark.gpu

SLOTS = 2 * cases.CAPACITY
HIDDEN = (1, 7, 16, 64)
KEY_MASK = (1 << 48) - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _dev(torch):
    return torch.device("cuda", torch.cuda.current_device())


def _stream(torch, dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _Arena:
    """Named arrays in one uint8 device buffer: GUARD guard bytes, an array, guard bytes up to the next multiple of 16, GUARD guard
    bytes, the next array, ...  Arrays start 16-byte aligned."""

    def __init__(self, arrays):
        self.names, self.at, off = list(arrays), {}, GUARD
        for name, a in arrays.items():
            self.at[name] = (off, a.dtype, a.shape, a.nbytes)
            off += a.nbytes + (-a.nbytes) % 16 + GUARD
        self.nbytes = off

    def build(self, arrays, complement=False, fill=None):
        host = np.full(self.nbytes, GUARD_BYTE, np.uint8)
        for name in self.names:
            off, dtype, shape, nbytes = self.at[name]
            a = np.ascontiguousarray(arrays[name], dtype)
            assert a.shape == shape
            raw = a.reshape(-1).view(np.uint8)
            host[off:off + nbytes] = fill if fill is not None else ~raw if complement else raw
        return host

    def ptr(self, buf, name):
        return buf.data_ptr() + self.at[name][0] if name in self.at else None

    def get(self, host, name):
        off, dtype, shape, nbytes = self.at[name]
        return host[off:off + nbytes].view(dtype).reshape(shape)

    def guards_intact(self, host):
        covered = np.zeros(self.nbytes, bool)
        for off, _, _, n in self.at.values():
            covered[off:off + n] = True
        return bool((host[~covered] == GUARD_BYTE).all())

    def differing(self, got, want):
        bad = [(name, int(np.flatnonzero(self.get(got, name).reshape(-1) != self.get(want, name).reshape(-1))[0]))
               for name in self.names if not np.array_equal(self.get(got, name), self.get(want, name))]
        return bad + ([] if self.guards_intact(got) else ["guard"])


def _state(torch, dev, blk, tgt, init=None, pos=None):
    from tiler_slider_amd import _cabi
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    keep = (up(np.ascontiguousarray(blk).view(np.int32)), up(tgt), up(init), up(pos))
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    return _cabi.State(p(keep[3]), p(keep[2]), p(keep[1]), p(keep[0]), None, None, None), keep


def _mlp(torch, dev, mlp):
    """ts_mlp of (w1 [H, D], b1, w2 [4, H], b2) in the kernel layout, and the tensors that keep it alive."""
    from tiler_slider_amd import _policy_cabi as pc
    w1, b1, w2, b2 = mlp
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (w1.T, b1, w2.T, b2)]
    return pc.Mlp(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), w1.shape[0], 0), t


def _dims(S, T, Tt, mc, L):
    from tiler_slider_amd import _cabi
    return _cabi.Dims(L, S, T, Tt, int(mc), 100, 0)


def _run(torch, dev, S, mc, blk, tgt, cells, rows, count, want, mlp=None, act_in=None, ptable_in=None, max_depth=252, root=0, prefill=None):
    """ts_rptable_actions (with `mlp`) or a given action table, ts_rptable_walk where `want` has a table, ts_rptable_score where it
    has a score, all into one arena prefilled with the complement of `want` (or with `prefill`); returns (arena, the buffer back on
    the host, the same buffer built from `want`)."""
    from tiler_slider_amd import _rptable_cabi as xc
    L, slots = rows.shape
    dims = _dims(S, cells.shape[0], tgt.shape[0], mc, L)
    st, keep = _state(torch, dev, blk, tgt, init=cells if root == 0 else None, pos=cells if root == 1 else None)
    arena = _Arena(want)
    buf = torch.from_numpy(arena.build(want, complement=prefill is None, fill=prefill)).to(dev)
    d_rows, d_count = torch.from_numpy(rows.view(np.int64)).to(dev), torch.from_numpy(np.ascontiguousarray(count, np.int32)).to(dev)
    lib, stream = xc.lib(), _stream(torch, dev)
    if mlp is not None:
        m, keep_m = _mlp(torch, dev, mlp)
        rc = lib.ts_rptable_actions(C.byref(dims), C.byref(st), C.byref(m), d_rows.data_ptr(), slots, d_count.data_ptr(), arena.ptr(buf, "act"),
                                    arena.ptr(buf, "logits"), stream)
        assert rc == 0, rc
        act_ptr = arena.ptr(buf, "act")
    else:
        d_act = torch.from_numpy(np.ascontiguousarray(act_in)).to(dev)
        act_ptr = d_act.data_ptr()
    ptable_ptr = arena.ptr(buf, "table")
    if "table" in want:
        cfg = xc.RptableCfg(max_depth, root)
        out = xc.RptableOut(arena.ptr(buf, "table"), arena.ptr(buf, "root_moves"), arena.ptr(buf, "deepest"))
        rc = lib.ts_rptable_walk(C.byref(dims), C.byref(st), d_rows.data_ptr(), slots, d_count.data_ptr(), act_ptr, C.byref(cfg), C.byref(out), stream)
        assert rc == 0, rc
    elif ptable_in is not None:
        d_pt = torch.from_numpy(np.ascontiguousarray(ptable_in).view(np.int64)).to(dev)
        ptable_ptr = d_pt.data_ptr()
    if "score" in want:
        rc = lib.ts_rptable_score(C.byref(dims), C.byref(st), ptable_ptr, act_ptr, d_rows.data_ptr(), slots, d_count.data_ptr(), arena.ptr(buf, "score"), stream)
        assert rc == 0, rc
    return arena, buf.cpu().numpy(), arena.build(want)


def _want(ref, slot, slots, act, logits, entry, root_moves, deepest, score):
    """The yardstick's flat answers laid out as the calls write them; None leaves an array out."""
    w = {}
    if act is not None:
        w["act"] = xr.scatter(ref, slot, act, slots, 255)
    if logits is not None:
        w["logits"] = xr.scatter(ref, slot, logits, slots, 0.0)
    if entry is not None:
        w["table"] = xr.scatter(ref, slot, xr.table_words(ref, entry), slots, 0)
        w["root_moves"], w["deepest"] = root_moves, deepest
    if score is not None:
        w["score"] = score
    return w


_NETS = {}


def _network(orc, S, mc):
    """(mlp, act, logits) of an integer network on the case of size S: H drawn from HIDDEN, computed once and shared."""
    if (S, mc) not in _NETS:
        blk, init, tgt, ref = rs.case(orc, S, mc)[:4]
        rng = np.random.default_rng(100 * S + mc)
        T, Tt = init.shape[0], tgt.shape[0]
        D = (1 + T + Tt if mc else 3) * S * S
        mlp = pref.random_mlp(rng, D, int(rng.choice(HIDDEN)), "int")
        _NETS[S, mc] = (mlp,) + xr.actions(orc, ref, blk, tgt, mlp)
    return _NETS[S, mc]


# ------------------------------------------------------------------------------------------------ 1. integer networks, host-filled rows
@pytest.mark.parametrize("S", range(1, 9))
def test_integer_networks_on_host_filled_rows_every_byte(torch_cuda, oracle, S):
    torch, dev = torch_cuda, _dev(torch_cuda)
    for mc in (False, True):
        blk, init, tgt, ref = rs.case(oracle, S, mc)[:4]
        mlp, act, logits = _network(oracle, S, mc)
        _, pos = cases.stepped(oracle, S, mc, blk, init, tgt)
        rows, slot = xr.rows_of(ref, SLOTS)
        scores = {}
        for order, depth, root, with_logits in (("forward", 252, 0, True), ("reversed", 252, 0, False), ("forward", 3, 1, True), ("forward", 0, 1, False)):
            r, s = (rows, slot) if order == "forward" else xr.rows_of(ref, SLOTS, "reversed")
            cells = init if root == 0 else pos
            e, deepest, _ = xr.walk(ref, act, depth)
            sc = xr.score(ref, e, act)
            want = _want(ref, s, SLOTS, act, logits if with_logits else None, e, xr.root_moves(oracle, ref, blk, tgt, cells, e), deepest, sc)
            arena, got, expect = _run(torch, dev, S, mc, blk, tgt, cells, r, ref.count, want, mlp=mlp, max_depth=depth, root=root)
            assert arena.differing(got, expect) == [], (S, mc, order, depth, root)
            scores[order, depth] = arena.get(got, "score").copy()
        assert np.array_equal(scores["forward", 252], scores["reversed", 252])       # other slots, the same sets, the same bits
        if S >= 3:
            assert (ref.count < 0).any() and (scores["forward", 252][ref.count < 0] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. the mixed policy through the wrapper
def _env(S, mc, blk, init, tgt, **kw):
    from tiler_slider_amd import VecTilerSliderEnv
    kw.setdefault("obs_dtype", None)
    return VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=mc, **kw)


def _flat_of(table, count, *others):
    """The live slots of host rows in the yardstick's order (level, key): (level, key, entry, others at those slots...)."""
    words = table.view(np.uint64)
    live = (count >= 0)[:, None] & ((words >> np.uint64(63)) != 0)
    lv, sl = np.nonzero(live)
    key = (words[lv, sl] & np.uint64(KEY_MASK)).astype(np.int64)
    order = np.lexsort((key, lv))
    lv, sl, key = lv[order], sl[order], key[order]
    return (lv, key, ((words[lv, sl] >> np.uint64(48)) & np.uint64(0xff)).astype(np.uint8)) + tuple(o[lv, sl] for o in others) + (sl,)


def _act_rows(ref, rt_table, rt_count, act, seed=0):
    """uint8 [L, slots]: the flat `act` of the yardstick in the slots the GPU's table gave its states, random bytes elsewhere."""
    lv, key, _, sl = _flat_of(rt_table, rt_count)
    assert np.array_equal(lv, ref.level) and np.array_equal(key, ref.idx), "the GPU's table holds other states than the yardstick's"
    rows = np.random.default_rng(seed).integers(0, 256, rt_table.shape).astype(np.uint8)
    rows[lv, sl] = act
    return rows


@pytest.mark.parametrize("S", range(3, 9))
def test_the_mixed_tabular_policy_on_a_table_the_gpu_built(torch_cuda, oracle, S):
    torch, dev = torch_cuda, _dev(torch_cuda)
    from tiler_slider_amd import ReachPolicyTable
    for mc in (False, True):
        blk, init, tgt, ref = rs.case(oracle, S, mc)[:4]
        env = _env(S, mc, blk, init, tgt, device=dev)
        table = env.build_reach_table(capacity=cases.CAPACITY)
        act = xr.mixed_policy(ref, 7 + S)
        act_rows = torch.from_numpy(_act_rows(ref, table.table.cpu().numpy(), table.count.cpu().numpy(), act)).to(dev)
        for depth in (252, 3):
            e, deepest, _ = xr.walk(ref, act, depth)
            pt = env.walk_actions(act_rows, max_depth=depth, table=table)
            assert isinstance(pt, ReachPolicyTable) and pt.count is table.count and pt.act is act_rows and pt.logits is None and pt.max_depth == depth
            lv, key, got_e, got_a, _ = _flat_of(pt.table.cpu().numpy(), pt.count.cpu().numpy(), pt.act.cpu().numpy())
            assert np.array_equal(lv, ref.level) and np.array_equal(key, ref.idx) and np.array_equal(got_e, e) and np.array_equal(got_a, act)
            assert np.array_equal(pt.deepest.cpu().numpy(), deepest)
            assert np.array_equal(pt.root_moves.cpu().numpy(), xr.root_moves(oracle, ref, blk, tgt, init, e))
            assert np.array_equal(env.score_policy(pt, table).columns.cpu().numpy(), xr.score(ref, e, act))
            assert torch.equal((pt.table != 0), (table.table < 0) & (table.count >= 0)[:, None])      # the same slots, nothing else
        n = int(np.flatnonzero(ref.count > 100)[0])
        keys, entries = pt.entries(n)
        keys2, acts = pt.actions(n)
        assert np.array_equal(keys.cpu().numpy(), ref.keys(n)) and torch.equal(keys, keys2)
        assert np.array_equal(entries.cpu().numpy(), e[ref.start[n]:ref.start[n + 1]]) and np.array_equal(acts.cpu().numpy(), act[ref.start[n]:ref.start[n + 1]])
        full = int(np.flatnonzero(ref.count < 0)[0])
        assert pt.actions(full)[0].numel() == 0 and not bool(pt.table[full].any())


# ------------------------------------------------------------------------------------------------ 3. the deep levels
@pytest.mark.parametrize("which", ("MULTI", "SMALL", "LARGE"))
def test_the_deep_levels_with_their_chain_policies(torch_cuda, oracle, which):
    """Each level alone and in a batch - beside copies of itself that are walked with an empty policy (they stop at round 1 while
    their neighbour goes on) and, on 8x8, deep_cases.companions -, at max_depth 252, the longest chain and one less."""
    import deep_cases as deep
    import table_reference as tref
    torch, dev = torch_cuda, _dev(torch_cuda)
    lv = deep.levels()[getattr(deep, which)]
    ref1, act1, chain = xr.deep_reference(oracle, lv)
    longest = int(chain[chain < tref.UNREACHABLE].max())
    others = list(deep.companions(lv).values()) if which == "MULTI" else []
    for alone in (True, False):
        group = [lv] if alone else [lv, lv] + others + [lv]
        blk, tgt, init = (np.ascontiguousarray(np.concatenate([getattr(g, f) for g in group], axis=1)) for f in ("blk", "tgt", "init"))
        ref = ref1 if alone else rt.build(oracle, lv.S, lv.mc, blk, tgt, init)
        act = xr.expert(ref)
        act[ref.level == 0] = act1
        act[ref.level == 1] = 255          # an empty policy on the same level
        env = _env(lv.S, lv.mc, blk, init, tgt, device=dev)
        table = env.build_reach_table()
        assert table.slots == 8192
        act_rows = torch.from_numpy(_act_rows(ref, table.table.cpu().numpy(), table.count.cpu().numpy(), act)).to(dev)
        for depth in sorted({252, min(longest, 252), min(longest, 252) - 1}):
            e, deepest, _ = xr.walk(ref, act, depth)
            pt = env.walk_actions(act_rows, max_depth=depth, table=table)
            got = _flat_of(pt.table.cpu().numpy(), pt.count.cpu().numpy())
            assert np.array_equal(got[1], ref.idx) and np.array_equal(got[2], e), (which, alone, depth)
            assert np.array_equal(pt.deepest.cpu().numpy(), deepest) and deepest[0] == min(longest, depth)
            assert np.array_equal(pt.root_moves.cpu().numpy(), xr.root_moves(oracle, ref, blk, tgt, init, e))
            if which == "LARGE" and depth == 252:       # exactly the long chains are DEEP, and nothing else
                first = ref.level == 0
                assert (e[first] == 254).sum() == 389 and np.array_equal(e[first] == 254, chain > 252)
            if not alone:
                assert (e[ref.level == 1] == 255).all() and deepest[1] == 0


# ------------------------------------------------------------------------------------------------ 4. against the dense kernels
@pytest.mark.parametrize("S,T,K,H", ((4, 2, 2, 7), (4, 2, 2, 64), (5, 3, 3, 7), (5, 3, 3, 64)))
def test_against_the_dense_policy_tables_where_both_exist(torch_cuda, oracle, S, T, K, H):
    """For every state of R: act and the logits' bits are the dense table's at that key, and the entry is the dense one where the
    dense one is finite.  An unresolved state is only required to be unresolved: the dense walk stops at the first distance no VALID
    placement lies at, the reach walk at the first distance no state of R lies at - different sets, so one may say NONE where the
    other, cut at max_depth, says DEEP.  5x5 with three tiles at capacity 16,384 is walked by the global form."""
    torch, dev = torch_cuda, _dev(torch_cuda)
    from tiler_slider_amd import MlpPolicy, _rptable_cabi as xc
    L, mc = 24, True
    blk, init, _ = oracle.generate_mt19937(S, T, T, K, np.arange(L, dtype=np.uint32))
    tgt = np.ascontiguousarray(cases.walked(oracle, S, blk, init))     # the targets where ten moves leave the tiles: the levels can be won
    env = _env(S, mc, blk, init, tgt, device=dev)
    table = env.build_reach_table(capacity=16384 if T == 3 else 256)
    assert xc.describe_rptable_walk(env._dims, table.slots)["form"] == (xc.FORM_GLOBAL if T == 3 else xc.FORM_LDS) and not bool(table.full.any())
    D = (1 + 2 * T) * S * S
    mlp = pref.random_mlp(np.random.default_rng(S * 100 + H), D, H, "gauss")
    policy = MlpPolicy(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in mlp))
    for depth in (252, 2):
        dense = env.build_policy_table(policy, max_depth=depth, logits=True)
        reach = env.build_policy_table(policy, max_depth=depth, logits=True, table=table)
        live = reach.table < 0
        assert torch.equal(live, table.table < 0) and int(live.sum()) == int(table.count.sum()) > 10 * L
        key = torch.where(live, reach.table & KEY_MASK, torch.zeros_like(reach.table))
        assert torch.equal(torch.where(live, dense.act.gather(1, key), torch.full_like(reach.act, 255)), reach.act)
        z = dense.logits.view(torch.int32).gather(1, key[:, :, None].expand(-1, -1, 4))
        assert torch.equal(torch.where(live[:, :, None], z, torch.zeros_like(z)), reach.logits.view(torch.int32))
        e_dense, e_reach = dense.dist.gather(1, key).long(), (reach.table >> 48) & 0xff
        finite = live & (e_dense >= 1) & (e_dense <= 252)
        assert torch.equal(finite, live & (e_reach >= 1) & (e_reach <= 252)) and torch.equal(e_dense[finite], e_reach[finite])
        assert bool((e_reach[live & ~finite] >= 254).all()) and not bool((e_dense[live] == 0).any())
        assert int(finite.sum()) > 0


# ------------------------------------------------------------------------------------------------ 5. bit-equal logits, reach-only shapes
@pytest.mark.parametrize("S,T,K,staged", ((5, 4, 3, 1), (8, 8, 10, 0)))
def test_the_logits_are_policy_logits_bits_on_either_side_of_weights_in_lds(torch_cuda, oracle, S, T, K, staged):
    torch, dev = torch_cuda, _dev(torch_cuda)
    from tiler_slider_amd import MlpPolicy, _rptable_cabi as xc
    L, mc, H = 32, True, 64
    if S == 8:      # eight tiles reach a few hundred states only between many obstacles: the levels of reach_cases
        assert cases.SHAPES[8][0] == T
        blk, init, tgt = (np.ascontiguousarray(a[:, :L]) for a in cases.levels(oracle, 8, mc))
    else:
        blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(L, dtype=np.uint32))
    env = _env(S, mc, blk, init, tgt, device=dev)
    table = env.build_reach_table(capacity=2048)
    assert xc.describe_rptable_actions(env._dims, H, table.slots)["weights_in_lds"] == staged
    mlp = pref.random_mlp(np.random.default_rng(S), (1 + 2 * T) * S * S, H, "gauss")
    policy = MlpPolicy(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in mlp))
    pt = env.build_policy_table(policy, logits=True, table=table)
    lv, key, _, act, z, _ = _flat_of(pt.table.cpu().numpy(), pt.count.cpu().numpy(), pt.act.cpu().numpy(), pt.logits.cpu().numpy())
    assert lv.size >= 500 and (act <= 3).all()
    cells = rt.cells_of(S, T, key, np.uint8)
    boards = _env(S, mc, np.ascontiguousarray(blk[:, lv]), cells, np.ascontiguousarray(tgt[:, lv]), device=dev)
    boards.reset()
    want = boards.policy_logits(policy).cpu().numpy()
    assert np.array_equal(want.view(np.int32), z.view(np.int32))
    assert np.array_equal(act, pref.select(want, None, pref.GREEDY))
    assert not bool(pt.logits[pt.table == 0].any()) and bool((pt.act[pt.table == 0] == 255).all())


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_end_to_end_policy_table_index_placement_rollout(torch_cuda, oracle):
    torch, dev = torch_cuda, _dev(torch_cuda)
    from tiler_slider_amd import MlpPolicy
    S, mc = 5, True
    blk, init, tgt, ref = rs.case(oracle, S, mc)[:4]
    T = init.shape[0]
    env = _env(S, mc, blk, init, tgt, device=dev, max_steps=1000)
    table = env.build_reach_table(capacity=cases.CAPACITY)
    mlp = pref.random_mlp(np.random.default_rng(3), (1 + 2 * T) * S * S, 16, "gauss")
    policy = MlpPolicy(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in mlp))
    pt = env.build_policy_table(policy, table=table)
    ridx = env.build_reach_index(pt)
    placed_any = 0
    for d in (1, 2, 3):
        env.reset()
        info = env.place_at_distance(ridx, d, d, seed=d)
        placed = info.placed
        assert torch.equal(info.dist[placed], torch.full_like(info.dist[placed], d))
        assert torch.equal(env.lookup(pt)[0][placed], torch.full_like(env.lookup(pt)[0][placed], d))     # lookup(ptable) answers the moves
        out = env.rollout_policy(d + 2, policy, select="greedy")
        assert torch.equal(out.first_win[placed], torch.full_like(out.first_win[placed], d)), d
        placed_any += int(placed.sum())
    assert placed_any >= 10
    # a board placed on a NONE state of the policy table has not won after 252 steps
    lv, key, e, _ = _flat_of(pt.table.cpu().numpy(), pt.count.cpu().numpy())
    none = e == 255
    levels, first = np.unique(lv[none], return_index=True)
    assert levels.size >= 20
    cells = init.copy()
    cells[:, levels] = rt.cells_of(S, T, key[none][first], init.dtype)
    env.reset()
    env._pos.copy_(torch.from_numpy(cells).to(dev))
    out = env.rollout_policy(252, policy, select="greedy")
    assert not bool(out.wins[torch.from_numpy(levels).to(dev)].any())


# ------------------------------------------------------------------------------------------------ 7. arbitrary bytes
@pytest.mark.parametrize("S,T,Tt,mc", ((5, 4, 4, True), (8, 8, 8, False), (3, 5, 5, True), (1, 1, 1, True)))
def test_rows_act_and_ptable_of_arbitrary_bytes(torch_cuda, oracle, S, T, Tt, mc):
    """The kernels are specified to stay in bounds over any bits: a bounds check of outputs the test owns, not a fault test.  Every
    call returns, the guards are intact, every output byte is written (two prefills give the same bytes), act of a live slot is
    <= 3 and every entry is a legal code."""
    torch, dev = torch_cuda, _dev(torch_cuda)
    rng = np.random.default_rng(S)
    L, slots = 67, 512
    blk = rng.integers(0, 1 << 32, ((S * S + 31) // 32, L), dtype=np.uint64).astype(np.uint32)
    tgt, cells = rng.integers(0, 256, (Tt, L)).astype(np.uint8), rng.integers(0, 256, (T, L)).astype(np.uint8)
    rows = rng.integers(0, 1 << 64, (L, slots), dtype=np.uint64)
    rows[::3] &= np.uint64((1 << 63) | (0xff << 48) | ((S * S) ** T - 1 if (S * S) ** T < (1 << 48) else KEY_MASK))
    rows[1::4, ::2] = 0
    count = rng.integers(-3, slots, L).astype(np.int32)
    D = (1 + T + Tt if mc else 3) * S * S
    mlp = pref.random_mlp(rng, D, 16, "gauss")
    mlp[2][0, 0] = np.nan
    shapes = dict(act=np.zeros((L, slots), np.uint8), logits=np.zeros((L, slots, 4), np.float32), table=np.zeros((L, slots), np.uint64),
                  root_moves=np.zeros(L, np.int16), deepest=np.zeros(L, np.int32), score=np.zeros((L, 8), np.int32))
    for depth, root in ((252, 0), (5, 1)):
        runs = [_run(torch, dev, S, mc, blk, tgt, cells, rows, count, shapes, mlp=mlp, max_depth=depth, root=root, prefill=p) for p in (0x00, 0xff)]
        arena, a, b = runs[0][0], runs[0][1], runs[1][1]
        assert arena.guards_intact(a) and arena.guards_intact(b) and np.array_equal(a, b)
        live = (count >= 0)[:, None] & ((rows >> np.uint64(63)) != 0)
        act, table, z = arena.get(a, "act"), arena.get(a, "table"), arena.get(a, "logits")
        assert (act[live] <= 3).all() and (act[~live] == 255).all() and not z[~live].view(np.int32).any()
        entry = (table >> np.uint64(48)) & np.uint64(0xff)
        assert np.array_equal(table != 0, live) and ((entry[live] >= 1) & (entry[live] != 253)).all()
        assert np.array_equal(table[live] & np.uint64(~(0xff << 48) & ((1 << 64) - 1)), (rows[live] & np.uint64(KEY_MASK)) | np.uint64(1 << 63))
        sc = arena.get(a, "score")
        assert np.array_equal(sc[:, 0], live.sum(axis=1)) and (sc[count < 0] == 0).all() and (arena.get(a, "deepest") <= depth).all()
    # a second walk over act bytes of any kind, and the score over random ptable / act bytes
    act_any = rng.integers(0, 256, (L, slots)).astype(np.uint8)
    del shapes["act"], shapes["logits"]
    runs = [_run(torch, dev, S, mc, blk, tgt, cells, rows, count, shapes, act_in=act_any, prefill=p) for p in (0x00, 0xff)]
    assert runs[0][0].guards_intact(runs[0][1]) and np.array_equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("S", (3, 6, 8))
def test_the_score_of_random_ptable_and_act_bytes_on_a_built_table(torch_cuda, oracle, S):
    torch, dev = torch_cuda, _dev(torch_cuda)
    mc = True
    blk, init, tgt, ref = rs.case(oracle, S, mc)[:4]
    rows, slot = xr.rows_of(ref, SLOTS)
    rng = np.random.default_rng(S)
    M = ref.idx.size
    p = rng.choice(np.array([0, 1, 2, 3, 7, 252, 253, 254, 255], np.uint8), M)
    p = np.where(rng.random(M) < 0.3, ref.entry, p).astype(np.uint8)
    act = np.where(rng.random(M) < 0.5, xr.expert(ref), rng.integers(0, 256, M)).astype(np.uint8)
    ptable = rng.integers(0, 1 << 48, (len(ref.count), SLOTS), dtype=np.uint64) | (rng.integers(0, 128, (len(ref.count), SLOTS), dtype=np.uint64) << np.uint64(56))
    ptable[ref.level, slot] = (ptable[ref.level, slot] & np.uint64(~(0xff << 48) & ((1 << 64) - 1))) | (p.astype(np.uint64) << np.uint64(48))
    act_rows = rng.integers(0, 256, (len(ref.count), SLOTS)).astype(np.uint8)
    act_rows[ref.level, slot] = act
    want = dict(score=xr.score(ref, p, act))
    assert want["score"][:, 4].sum() > 100 and want["score"][:, 7].sum() > 100 and (want["score"][:, 5] < 0).any()
    arena, got, expect = _run(torch, dev, S, mc, blk, tgt, init, rows, ref.count, want, act_in=act_rows, ptable_in=ptable)
    assert arena.differing(got, expect) == []


# ------------------------------------------------------------------------------------------------ 8. the wrapper's refusals
def test_wrapper_refusals_and_a_stream_of_its_own(torch_cuda, oracle):
    torch, dev = torch_cuda, _dev(torch_cuda)
    from tiler_slider_amd import MlpPolicy, ReachPolicyTable
    S, T, K, L, mc = 5, 4, 3, 8, True
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(L, dtype=np.uint32))
    env = _env(S, mc, blk, init, tgt, device=dev, obs_dtype="float32")
    env.reset()
    table = env.build_reach_table(capacity=512)
    policy = MlpPolicy(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in pref.random_mlp(np.random.default_rng(0), (1 + 2 * T) * S * S, 7, "gauss")))
    act = torch.zeros((L, table.slots), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="65536"):          # table=None on a reach shape: today's message
        env.build_policy_table(policy)
    with pytest.raises(ValueError, match="65536"):
        env.walk_actions(act)
    fewer = _env(S, mc, blk[:, :5], init[:, :5], tgt[:, :5], device=dev)
    other = _env(S, mc, *oracle.generate_mt19937(S, 3, 3, K, np.arange(L, dtype=np.uint32)), device=dev)
    for e, exc in ((fewer, "levels"), (other, "built for")):
        with pytest.raises(ValueError, match=exc):
            e.build_policy_table(policy, table=table)
        with pytest.raises(ValueError, match=exc):
            e.walk_actions(act, table=table)
    with pytest.raises(ValueError, match="lives on"):
        env.build_policy_table(policy, table=type(table)(table.table.cpu(), table.count.cpu(), None, None, 512, S, T, T, mc, 252, "init"))
    with pytest.raises(ValueError, match="contiguous"):
        env.walk_actions(torch.zeros((table.slots, L), dtype=torch.uint8, device=dev).t(), table=table)
    with pytest.raises(TypeError):
        env.walk_actions(act.int(), table=table)
    with pytest.raises(ValueError, match="max_depth"):
        env.walk_actions(act, max_depth=253, table=table)
    with pytest.raises(ValueError, match="max_bytes"):
        env.build_policy_table(policy, table=table, logits=True, max_bytes=25 * L * table.slots - 1)
    with pytest.raises(TypeError):
        env.build_policy_table(policy, table=object())
    mapped = _env(S, mc, blk, init, tgt, device=dev, host_mapped=True)
    with pytest.raises(ValueError, match="host_mapped"):
        mapped.walk_actions(act, table=table)
    pt = env.build_policy_table(policy, table=table, logits=True, max_bytes=25 * L * table.slots)
    assert isinstance(pt, ReachPolicyTable) and tuple(pt.logits.shape) == (L, table.slots, 4) and pt.root == "init" and pt.capacity == 512
    small = _env(4, mc, *oracle.generate_mt19937(4, 2, 2, 2, np.arange(L, dtype=np.uint32)), device=dev)
    dense_table = small.build_table()
    dense_pt = small.walk_actions(torch.zeros((L, 256), dtype=torch.uint8, device=dev))
    with pytest.raises(TypeError):
        env.score_policy(pt, dense_table)
    with pytest.raises(TypeError):
        small.score_policy(dense_pt, small.build_reach_table(capacity=64))
    with pytest.raises(ValueError, match="slots"):
        env.score_policy(pt, env.build_reach_table(capacity=1024))
    # a call on a stream of its own behind a step()
    want = env.score_policy(pt, table).columns.clone()
    side = torch.cuda.Stream(device=dev)
    env.step(torch.zeros(L, dtype=torch.uint8, device=dev))
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        again = env.build_policy_table(policy, table=table, logits=True)
        score = env.score_policy(again, table).columns
    side.synchronize()
    assert torch.equal(again.table, pt.table) and torch.equal(again.act, pt.act) and torch.equal(again.logits, pt.logits) and torch.equal(score, want)


# ------------------------------------------------------------------------------------------------ 9. every kernel at 4,096 waves
@pytest.mark.parametrize("S", range(1, 9))
def test_the_walk_and_the_score_over_a_full_grid_and_a_ragged_second_pass(torch_cuda, oracle, S):
    """cases.N_BUILD levels - the 128 of the case over and over -: a full grid of 1,024 blocks and 61 that take a second level.
    (The actions kernel runs at 128 levels x 2,048 slots in the first test of this file.)"""
    torch, dev = torch_cuda, _dev(torch_cuda)
    mc = S % 2 == 1
    blk, init, tgt, ref = rs.case(oracle, S, mc)[:4]
    act = xr.mixed_policy(ref, 7 + S)
    rows, slot = xr.rows_of(ref, SLOTS)
    e, deepest, _ = xr.walk(ref, act)
    want = _want(ref, slot, SLOTS, None, None, e, xr.root_moves(oracle, ref, blk, tgt, init, e), deepest, xr.score(ref, e, act))
    rep = np.arange(cases.N_BUILD) % cases.DISTINCT
    tile = lambda a, axis=0: np.ascontiguousarray(np.take(a, rep, axis=axis))
    act_rows = np.random.default_rng(S).integers(0, 256, rows.shape).astype(np.uint8)
    act_rows[ref.level, slot] = act
    arena, got, expect = _run(torch, dev, S, mc, tile(blk, 1), tile(tgt, 1), tile(init, 1), tile(rows), tile(ref.count),
                              {k: tile(v) for k, v in want.items()}, act_in=tile(act_rows))
    assert arena.differing(got, expect) == []


# ------------------------------------------------------------------------------------------------ 10. the global form of the walk
GLOBAL_SLOTS = 16384        # above lds_slots: the (succ, entry) pairs live in the output row


@pytest.mark.parametrize("S", range(1, 9))
def test_the_global_form_of_the_walk_every_byte(torch_cuda, oracle, S):
    """k_rptable_walk<S, true> for every S against the yardstick, byte for byte: the rows of the case filled on the host into
    16,384 slots, FULL levels (rows of random bits) among them, the mixed policy in the states' slots and random bytes in every
    other, max_depth 252, 3 (levels that stop by each rule: tests/test_rptable_cpu.py) and 0, both roots - table, root_moves,
    deepest, the score of the table just written, and the guards.  7x7 also at cases.N_BUILD levels: a full grid and a ragged
    second pass."""
    torch, dev = torch_cuda, _dev(torch_cuda)
    from tiler_slider_amd import _rptable_cabi as xc
    for mc in (False, True):
        blk, init, tgt, ref = rs.case(oracle, S, mc)[:4]
        d = xc.describe_rptable_walk(_dims(S, init.shape[0], tgt.shape[0], mc, cases.DISTINCT), GLOBAL_SLOTS)
        assert (d["form"], d["name"]) == (xc.FORM_GLOBAL, f"k_rptable_walk<{S}, true>") and GLOBAL_SLOTS > d["lds_slots"]
        _, pos = cases.stepped(oracle, S, mc, blk, init, tgt)
        act = xr.mixed_policy(ref, 7 + S)
        rows, slot = xr.rows_of(ref, GLOBAL_SLOTS)
        act_rows = np.random.default_rng(S).integers(0, 256, rows.shape).astype(np.uint8)
        act_rows[ref.level, slot] = act
        for depth, root in ((252, 0), (3, 1), (0, 1), (3, 0)):
            cells = init if root == 0 else pos
            e, deepest, exhausted = xr.walk(ref, act, depth)
            want = _want(ref, slot, GLOBAL_SLOTS, None, None, e, xr.root_moves(oracle, ref, blk, tgt, cells, e), deepest, xr.score(ref, e, act))
            if S >= 3:
                assert (ref.count < 0).any() and not want["table"][ref.count < 0].any()
                if depth == 3:
                    held = ref.count > 0
                    assert (exhausted & held).sum() >= 2 and (~exhausted & held).sum() >= 2 and (e == 254).any() and (e == 255).any()
            arena, got, expect = _run(torch, dev, S, mc, blk, tgt, cells, rows, ref.count, want, act_in=act_rows, max_depth=depth, root=root)
            assert arena.differing(got, expect) == [], (S, mc, depth, root)
        if S == 7 and mc:
            rep = np.arange(cases.N_BUILD) % cases.DISTINCT
            tile = lambda a, axis=0: np.ascontiguousarray(np.take(a, rep, axis=axis))
            arena, got, expect = _run(torch, dev, S, mc, tile(blk, 1), tile(tgt, 1), tile(cells, 1), tile(rows), tile(ref.count),
                                      {k: tile(v) for k, v in want.items()}, act_in=tile(act_rows), max_depth=depth, root=root)
            assert arena.differing(got, expect) == []


def test_walk_actions_forwards_max_bytes(torch_cuda, oracle):
    torch, dev = torch_cuda, _dev(torch_cuda)
    S, T, K, L, mc = 5, 4, 3, 8, True
    blk, init, tgt = oracle.generate_mt19937(S, T, T, K, np.arange(L, dtype=np.uint32))
    env = _env(S, mc, blk, init, tgt, device=dev)
    table = env.build_reach_table(capacity=512)
    act = torch.zeros((L, table.slots), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="max_bytes"):
        env.walk_actions(act, table=table, max_bytes=9 * L * table.slots - 1)
    assert len(env.walk_actions(act, table=table, max_bytes=9 * L * table.slots)) == L
