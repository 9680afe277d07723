"""The policy tables on the GPU (lib/libtiler_slider_ptable.so), exact equality everywhere unless said, against the NumPy
definition (tests/ptable_reference.py).  Every raw call writes into ONE buffer the test owns - act, logits, dist and score between
guard bytes - prefilled with the complement of the expected bytes, and the whole buffer is compared with the same buffer built
from the yardstick's answer: every byte is written, and none beside."""
import ctypes as C

import numpy as np
import pytest

import policy_reference as pref
import ptable_reference as xref
import table_reference as tref
from table_harness import GUARD, GUARD_BYTE

pytestmark = pytest.mark.gpu

# (S, T, Tt, obstacles, multi colour): the index spaces 1 .. 65,536, single and multi colour, T != Tt
SHAPES = ((1, 1, 1, 0, False), (3, 0, 0, 1, True), (2, 2, 2, 0, True), (3, 2, 2, 1, False), (4, 2, 2, 2, False), (4, 2, 2, 2, True),
          (5, 2, 2, 3, True), (3, 3, 3, 1, True), (8, 1, 1, 10, False), (8, 2, 2, 10, False), (3, 5, 5, 1, False), (4, 4, 4, 2, True),
          (4, 2, 3, 2, False), (4, 2, 1, 2, True), (4, 1, 2, 2, True))
LEVELS = (1, 3, 65, 257)
HIDDEN = (1, 7, 16, 64)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _dev(torch):
    return torch.device("cuda", torch.cuda.current_device())


class _Arena:
    """Named arrays in one uint8 device buffer: GUARD guard bytes, `shift` more, an array, guard bytes up to the next multiple of 16,
    GUARD guard bytes, the next array, ...  Arrays start 16-byte aligned plus `shift`."""

    def __init__(self, arrays, shift=0):
        self.names, self.at, off = list(arrays), {}, GUARD
        for name, a in arrays.items():
            off += shift
            self.at[name] = (off, a.dtype, a.shape, a.nbytes)
            off += a.nbytes + (-(a.nbytes + shift)) % 16 + GUARD
        self.nbytes = off

    def build(self, arrays, complement=False):
        host = np.full(self.nbytes, GUARD_BYTE, np.uint8)
        for name in self.names:
            off, dtype, shape, nbytes = self.at[name]
            a = np.ascontiguousarray(arrays[name], dtype)
            assert a.shape == shape
            raw = a.reshape(-1).view(np.uint8)
            host[off:off + nbytes] = ~raw if complement else raw
        return host

    def ptr(self, buf, name):
        return buf.data_ptr() + self.at[name][0]

    def differing(self, got, want):
        bad, covered = [], np.zeros(self.nbytes, bool)
        for name in self.names:
            off, _, _, n = self.at[name]
            covered[off:off + n] = True
            if not np.array_equal(got[off:off + n], want[off:off + n]):
                bad.append((name, int(np.flatnonzero(got[off:off + n] != want[off:off + n])[0])))
        if not np.array_equal(got[~covered], want[~covered]):
            bad.append("guard")
        return bad


def _levels(orc, S, T, Tt, K, L, seed, variant=None):
    """L random levels (blk, tgt) of any shape: obstacles, tiles and targets side by side where they fit, else the obstacles drawn
    apart from the targets; one cell: nothing to draw."""
    if S == 1:
        blk, tgt = np.zeros((1, L), np.uint32), np.zeros((Tt, L), np.uint8)
    elif T + Tt + K <= S * S:
        blk, _, tgt = orc.generate(S, T, Tt, K, L, seed=seed)
    else:
        blk, _, _ = orc.generate(S, T, 0, K, L, seed=seed)
        _, _, tgt = orc.generate(S, 0, Tt, 0, L, seed=seed + 1)
    if variant == "repeated targets" and Tt >= 2:
        tgt[1] = tgt[0]
    if variant == "targets beyond the board" and Tt >= 1:
        tgt[0, ::2] = 200 + (np.arange(len(tgt[0, ::2])) % 50)     # clamped to S * S - 1
    return blk, tgt


def _mixed_actions(orc, rng, S, T, mc, blk, tgt):
    """A tabular policy of any bytes that still gets somewhere: the expert's move on two placements of three, a random byte 0 .. 255
    on the others, a random move on every fifth - chains, detours, dead ends, cycles and bytes that are no move."""
    tgt = _clamped(S, tgt)
    expert, _ = xref.expert_actions(orc, S, mc, blk, tgt, T, tref.table(orc, S, mc, blk, tgt, T))
    act = np.where(rng.random(expert.shape) < 2 / 3, expert, rng.integers(0, 256, expert.shape)).astype(np.uint8)
    act[:, 1::5] = rng.integers(0, 4, act[:, 1::5].shape)
    return act


def _clamped(S, tgt):
    return np.minimum(tgt, S * S - 1).astype(tgt.dtype)


def _state(torch, dev, blk, tgt):
    from tiler_slider_amd import _cabi
    dblk = torch.from_numpy(np.ascontiguousarray(blk).view(np.int32)).to(dev)
    dtgt = torch.from_numpy(np.ascontiguousarray(tgt)).to(dev)
    st = _cabi.State(None, None, dtgt.data_ptr() if dtgt.numel() else None, dblk.data_ptr(), None, None, None)
    return st, (dblk, dtgt)


def _mlp(torch, dev, mlp):
    """ts_mlp of (w1 [H, D], b1, w2 [4, H], b2) in the kernel layout, and the tensors that keep it alive."""
    from tiler_slider_amd import _policy_cabi as pc
    w1, b1, w2, b2 = mlp
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (w1.T, b1, w2.T, b2)]
    return pc.Mlp(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), w1.shape[0], 0), t


def _dims(S, T, Tt, mc, L):
    from tiler_slider_amd import _cabi
    return _cabi.Dims(L, S, T, Tt, int(mc), 100, 0)


def _stream(torch, dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _run_all(torch, dev, S, T, Tt, mc, blk, tgt, want, mlp=None, act_in=None, max_depth=252, shift=0, table=None, with_logits=True):
    """ts_ptable_actions (with `mlp`) or a given action table, ts_ptable_walk, and ts_ptable_score against `table`, all into one
    arena prefilled with the complement of `want`; returns the names of the arrays that differ."""
    from tiler_slider_amd import _ptable_cabi as xc
    L = blk.shape[1]
    dims = _dims(S, T, Tt, mc, L)
    st, keep = _state(torch, dev, blk, tgt)
    arena = _Arena(want, shift)
    buf = torch.from_numpy(arena.build(want, complement=True)).to(dev)
    lib = xc.lib()
    if mlp is not None:
        m, keep_m = _mlp(torch, dev, mlp)
        rc = lib.ts_ptable_actions(C.byref(dims), C.byref(st), C.byref(m), arena.ptr(buf, "act"), arena.ptr(buf, "logits") if with_logits else None,
                                   _stream(torch, dev))
        assert rc == 0, rc
        act_ptr = arena.ptr(buf, "act")
    else:
        d_act = torch.from_numpy(act_in).to(dev)
        act_ptr = d_act.data_ptr()
    if "dist" in want:
        assert lib.ts_ptable_walk(C.byref(dims), C.byref(st), act_ptr, max_depth, arena.ptr(buf, "dist"), _stream(torch, dev)) == 0
    if "score" in want:
        d_table = torch.from_numpy(table).to(dev)
        assert lib.ts_ptable_score(C.byref(dims), C.byref(st), arena.ptr(buf, "dist"), act_ptr, d_table.data_ptr(), arena.ptr(buf, "score"),
                                   _stream(torch, dev)) == 0
    got = buf.cpu().numpy()
    del keep
    return arena.differing(got, arena.build(want))


@pytest.mark.parametrize("S,T,Tt,K,mc", SHAPES)
def test_actions_walk_and_score_of_integer_networks(torch_cuda, oracle, S, T, Tt, K, mc):
    """Random integer networks (float32 is exact on them), every H, every L the index space allows, max_depth 252, 2 and 0."""
    torch, dev = torch_cuda, _dev(torch_cuda)
    states = (S * S) ** T
    rng = np.random.default_rng(100 * S + T)
    D = (1 + T + Tt if mc else 3) * S * S
    solved = valid = 0
    for i, L in enumerate(l for l in LEVELS if l <= 3 or states < 59049):
        H = HIDDEN[(i + S + T) % 4]
        variant = (None, "repeated targets", "targets beyond the board", None)[i] if (S, T) == (4, 2) else None
        blk, tgt = _levels(oracle, S, T, Tt, K, L, seed=17 * S + L, variant=variant)
        mlp = pref.random_mlp(rng, D, H, "int")
        max_depth = (252, 2, 0, 252)[i]
        ctgt = _clamped(S, tgt)
        act, z, _ = xref.actions(oracle, S, mc, blk, ctgt, T, mlp, True)
        dist = xref.walk(oracle, S, mc, blk, ctgt, T, act, max_depth)
        table = tref.table(oracle, S, mc, blk, ctgt, T)
        want = dict(act=act, logits=z, dist=dist, score=xref.score(oracle, S, mc, blk, ctgt, T, dist, act, table))
        assert _run_all(torch, dev, S, T, Tt, mc, blk, tgt, want, mlp=mlp, max_depth=max_depth, table=table) == [], (L, H, max_depth)
        solved += int(want["score"][:, 2].sum())
        valid += int(want["score"][:, 0].sum())
    print(f"{S}x{S} / {T}: {valid} valid placements, {solved} solved by the random networks")
    assert valid > 0


@pytest.mark.parametrize("args,mc", (((4, 2, 2, 2, 1, 3), True), ((4, 2, 2, 2, 1, 5), False), ((8, 1, 1, 10, 4, 11), False)))
def test_the_expert_vote_networks(torch_cuda, oracle, args, mc):
    """The inputs that carry the cases (tests/test_ptable_cpu.py asserts that they do): chains of up to 10 moves, detours, cycles,
    ties; every max_depth of 0, 2 and 252; without the logits too."""
    torch, dev = torch_cuda, _dev(torch_cuda)
    S, T, Tt, K, n, seed = args
    blk, _, tgt = oracle.generate(S, T, Tt, K, n, seed=seed)
    mlp = xref.expert_vote_mlp(oracle, S, mc, blk, tgt, T)
    act, z, _ = xref.actions(oracle, S, mc, blk, tgt, T, mlp, True)
    table = tref.table(oracle, S, mc, blk, tgt, T)
    for max_depth in (0, 2, 252):
        dist = xref.walk(oracle, S, mc, blk, tgt, T, act, max_depth)
        want = dict(act=act, logits=z, dist=dist, score=xref.score(oracle, S, mc, blk, tgt, T, dist, act, table))
        assert _run_all(torch, dev, S, T, Tt, mc, blk, tgt, want, mlp=mlp, max_depth=max_depth, table=table) == [], max_depth
        del want["logits"]
        assert _run_all(torch, dev, S, T, Tt, mc, blk, tgt, want, mlp=mlp, max_depth=max_depth, table=table, with_logits=False) == [], max_depth
    assert ((dist >= 3) & (dist <= 252)).sum() >= 20 and (dist == 255).sum() >= 20


def _standing_env(torch, dev, S, T, mc, blk, tgt, valid, cells, **kw):
    """An environment of one board per valid placement, standing on it: (env, level of each, index of each)."""
    from tiler_slider_amd import VecTilerSliderEnv
    nb, ns = np.nonzero(valid)
    init = np.ascontiguousarray(cells[:, ns].astype(np.uint8))
    env = VecTilerSliderEnv.from_arrays(S, np.ascontiguousarray(blk[:, nb]), init, np.ascontiguousarray(tgt[:, nb]), multi_color=mc, device=dev,
                                        obs_dtype=None, **kw)
    env.reset()
    return env, nb, ns


@pytest.mark.parametrize("S,T,Tt,K,mc", [s for s in SHAPES if (s[0] * s[0]) ** s[1] <= 4096])
@pytest.mark.parametrize("H", (7, 64))
def test_gaussian_logits_are_bit_equal_to_policy_logits(torch_cuda, oracle, S, T, Tt, K, mc, H):
    """ts_policy_logits on a board standing on every valid placement, through the wrapper: torch.equal.  (The describe call reports
    one plan of the tile-plane weights for every table shape - staged; tests/test_ptable_cpu.py asserts it - so there is no second
    plan to cover.)  The values lie inside logits64's bound, and act is the rule applied to the kernel's own logits."""
    from tiler_slider_amd import MlpPolicy
    torch, dev = torch_cuda, _dev(torch_cuda)
    L = 5 if (S * S) ** T <= 625 else 2
    blk, tgt = _levels(oracle, S, T, Tt, K, L, seed=3 + S)
    tgt = _clamped(S, tgt)
    D = (1 + T + Tt if mc else 3) * S * S
    mlp = pref.random_mlp(np.random.default_rng(7 * S + H), D, H)
    policy = MlpPolicy(*(torch.from_numpy(a).to(dev) for a in mlp))
    valid, cells = xref.placements(S, blk, T)
    from tiler_slider_amd import VecTilerSliderEnv
    env = VecTilerSliderEnv.from_arrays(S, blk, np.zeros((T, L), np.uint8), tgt, multi_color=mc, device=dev, obs_dtype=None)
    pt = env.build_policy_table(policy, logits=True)
    standing, nb, ns = _standing_env(torch, dev, S, T, mc, blk, tgt, valid, cells)
    z_boards = standing.policy_logits(policy)
    z_table = pt.logits[torch.from_numpy(nb).to(dev), torch.from_numpy(ns).to(dev)]
    assert torch.equal(z_table.view(torch.int32), z_boards.view(torch.int32)), "the logits are not those of ts_policy_logits, bit for bit"
    _, z64, bound = xref.actions(oracle, S, mc, blk, tgt, T, mlp, False)
    got = pt.logits.cpu().numpy().astype(np.float64)
    assert (np.abs(got - z64) <= bound).all()
    z = pt.logits.cpu().numpy()
    rule = np.where(valid, pref.select(z.reshape(-1, 4), None, pref.GREEDY).reshape(valid.shape), 255)
    assert np.array_equal(pt.act.cpu().numpy(), rule)
    assert not z[~valid].any() and np.abs(z[valid]).max() > 0


@pytest.mark.parametrize("S,T,Tt,K,mc", SHAPES[:12])
def test_walk_over_random_bytes_and_over_the_expert(torch_cuda, oracle, S, T, Tt, K, mc):
    torch, dev = torch_cuda, _dev(torch_cuda)
    from tiler_slider_amd import VecTilerSliderEnv
    states = (S * S) ** T
    L = 3 if states >= 4096 else 65
    blk, tgt = _levels(oracle, S, T, Tt, K, L, seed=29 + S)
    rng = np.random.default_rng(S + 10 * T)
    act = _mixed_actions(oracle, rng, S, T, mc, blk, tgt)
    for max_depth in (252, 1):
        want = dict(dist=xref.walk(oracle, S, mc, blk, tgt, T, act, max_depth))
        assert _run_all(torch, dev, S, T, Tt, mc, blk, tgt, want, act_in=act, max_depth=max_depth) == [], max_depth
    # the expert's action table, from the kernel's own lookup on every placement: the walk is ts_table_build's output
    env = VecTilerSliderEnv.from_arrays(S, blk, np.zeros((T, L), np.uint8), tgt, multi_color=mc, device=dev, obs_dtype=None)
    table = env.build_table()
    expert, _ = xref.expert_actions(oracle, S, mc, blk, tgt, T, table.dist.cpu().numpy())
    d_expert = torch.from_numpy(expert).to(dev)
    for max_depth in (0, 2, 252):
        walked = env.walk_actions(d_expert, max_depth)
        assert torch.equal(walked.dist, env.build_table(max_depth).dist), max_depth
    score = env.score_policy(env.walk_actions(d_expert), table)
    assert torch.equal(score.solved, score.solvable) and torch.equal(score.optimal, score.solvable) and torch.equal(score.agree, score.solvable)
    assert not score.excess.any() and float(score.agreement) == (1.0 if int(score.solvable.sum()) else 0.0)


@pytest.mark.parametrize("S,T,Tt,K,mc", SHAPES[:12])
def test_score_over_tables_nobody_built(torch_cuda, oracle, S, T, Tt, K, mc):
    """Random bytes in all three tables, every array 5 bytes off a 16-byte boundary; and built tables at the same offset."""
    torch, dev = torch_cuda, _dev(torch_cuda)
    states = (S * S) ** T
    L = 3 if states >= 4096 else 65
    blk, tgt = _levels(oracle, S, T, Tt, K, L, seed=31 + S)
    rng = np.random.default_rng(S + 100 * T)
    from tiler_slider_amd import _ptable_cabi as xc
    dims = _dims(S, T, Tt, mc, L)
    st, keep = _state(torch, dev, blk, tgt)
    for built in (False, True):
        if built:
            act = _mixed_actions(oracle, rng, S, T, mc, blk, tgt)
            p, o = xref.walk(oracle, S, mc, blk, tgt, T, act), tref.table(oracle, S, mc, blk, tgt, T)
        else:
            act, p, o = (rng.integers(0, 256, (L, states)).astype(np.uint8) for _ in range(3))
            p[:, ::3], o[:, ::2] = rng.integers(0, 8, p[:, ::3].shape), rng.integers(0, 8, o[:, ::2].shape)
        want = xref.score(oracle, S, mc, blk, tgt, T, p, act, o)
        inputs = _Arena(dict(p=p, act=act, o=o), shift=5)
        ibuf = torch.from_numpy(inputs.build(dict(p=p, act=act, o=o))).to(dev)
        out = _Arena(dict(score=want), shift=4)
        obuf = torch.from_numpy(out.build(dict(score=want), complement=True)).to(dev)
        assert (inputs.ptr(ibuf, "p") % 16, out.ptr(obuf, "score") % 16) == (5, 4)
        rc = xc.lib().ts_ptable_score(C.byref(dims), C.byref(st), inputs.ptr(ibuf, "p"), inputs.ptr(ibuf, "act"), inputs.ptr(ibuf, "o"),
                                      out.ptr(obuf, "score"), _stream(torch, dev))
        assert rc == 0
        assert out.differing(obuf.cpu().numpy(), out.build(dict(score=want))) == [], built
        assert np.array_equal(ibuf.cpu().numpy(), inputs.build(dict(p=p, act=act, o=o)))
        if states > 1 and not built:
            assert want[:, 1].sum() > 0 and want[:, 2].sum() > 0
    del keep


# ---------------------------------------------------------------------------------------------------------------- the wrapper
@pytest.fixture(scope="module")
def two_levels(torch_cuda, oracle):
    """Two 4x4 levels (the issue's inputs of seeds 3 and 5 are single levels; these are two of one seed, multi colour), their
    expert-vote network, the yardstick's answer, and the environment of the levels."""
    from tiler_slider_amd import MlpPolicy, VecTilerSliderEnv
    torch, dev = torch_cuda, _dev(torch_cuda)
    S, T, mc = 4, 2, True
    blk, init, tgt = oracle.generate(S, T, T, 2, 2, seed=3)
    mlp = xref.expert_vote_mlp(oracle, S, mc, blk, tgt, T)
    act, z, _ = xref.actions(oracle, S, mc, blk, tgt, T, mlp, True)
    dist = xref.walk(oracle, S, mc, blk, tgt, T, act)
    env = VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=mc, device=dev, obs_dtype=None)
    policy = MlpPolicy(*(torch.from_numpy(a).to(dev) for a in mlp))
    return dict(S=S, T=T, mc=mc, blk=blk, tgt=tgt, mlp=mlp, act=act, z=z, dist=dist, env=env, policy=policy)


def test_build_policy_table_is_the_two_raw_calls(torch_cuda, oracle, two_levels):
    from tiler_slider_amd import DistanceTable, PolicyNet, PolicyTable
    torch, w = torch_cuda, two_levels
    env = w["env"]
    pt = env.build_policy_table(w["policy"], logits=True)
    assert isinstance(pt, PolicyTable) and isinstance(pt, DistanceTable) and pt.max_depth == 252
    assert np.array_equal(pt.act.cpu().numpy(), w["act"]) and np.array_equal(pt.dist.cpu().numpy(), w["dist"])
    assert np.array_equal(pt.logits.cpu().numpy(), w["z"])
    again = env.build_policy_table(w["policy"])
    assert again.logits is None and torch.equal(again.act, pt.act) and torch.equal(again.dist, pt.dist)          # the same bits on two runs
    assert torch.equal(env.walk_actions(pt.act).dist, pt.dist) and env.walk_actions(pt.act).act is pt.act
    cut = env.build_policy_table(w["policy"], max_depth=2)
    assert np.array_equal(cut.dist.cpu().numpy(), xref.walk(oracle, w["S"], w["mc"], w["blk"], w["tgt"], w["T"], w["act"], 2)) and not bool(cut.complete.all())
    # a PolicyNet through its .policy(): the parameters in the kernel layout, shared
    net = PolicyNet(w["policy"].features, w["policy"].hidden, env.device)
    with torch.no_grad():
        for p, a in zip((net.w1, net.b1, net.w2, net.b2), (w["policy"].w1, w["policy"].b1, w["policy"].w2, w["policy"].b2)):
            p.copy_(a)
    assert torch.equal(env.build_policy_table(net).dist, pt.dist)
    table = env.build_table()
    s1, s2 = env.score_policy(pt, table), env.score_policy(pt, table)
    want = xref.score(oracle, w["S"], w["mc"], w["blk"], w["tgt"], w["T"], w["dist"], w["act"], table.dist.cpu().numpy())
    assert np.array_equal(s1.columns.cpu().numpy(), want) and torch.equal(s1.columns, s2.columns)
    tot = want.sum(axis=0)
    assert s1.solved_share.dim() == 0 and s1.solved_share.device == env.device
    assert (float(s1.solved_share), float(s1.optimal_share), float(s1.agreement)) == (tot[2] / tot[1], tot[3] / tot[1], tot[4] / tot[1])
    assert torch.equal(s1.solved, s1.columns[:, 2]) and 0 < tot[3] < tot[2] < tot[1]


def test_lookup_and_place_at_distance_take_a_policy_table(torch_cuda, oracle, two_levels):
    torch, w = torch_cuda, two_levels
    env = w["env"]
    pt = env.build_policy_table(w["policy"])
    valid, cells = xref.placements(w["S"], w["blk"], w["T"])
    standing, nb, ns = _standing_env(torch, env.device, w["S"], w["T"], w["mc"], w["blk"], w["tgt"], valid, cells)
    moves, _ = standing.lookup(pt, rows=torch.from_numpy(nb.astype(np.int32)))
    assert np.array_equal(moves.cpu().numpy(), tref.to_moves(w["dist"][nb, ns]))
    rows = torch.from_numpy(nb.astype(np.int32)).to(env.device)
    info = standing.place_at_distance(pt, 3, 6, rows=rows, seed=1)
    want = ((w["dist"] >= 3) & (w["dist"] <= 6)).sum(axis=1)
    placed = info.placed.cpu().numpy()
    assert np.array_equal(info.count.cpu().numpy(), want[nb]) and np.array_equal(placed, want[nb] > 0) and want.max() >= 20
    d = info.dist.cpu().numpy()
    assert ((d[placed] >= 3) & (d[placed] <= 6)).all() and (d[~placed] == 255).all()
    assert np.array_equal(standing.lookup(pt, rows=rows)[0].cpu().numpy()[placed], d[placed].astype(np.int16))


def test_a_greedy_rollout_from_every_placement_wins_after_exactly_dist_steps(torch_cuda, oracle, two_levels):
    """Strict mode, no exploration: from every valid placement of the two levels the fused rollout first wins after exactly
    `dist` steps, and never where dist is 255."""
    torch, w = torch_cuda, two_levels
    dist = w["dist"]
    valid, cells = xref.placements(w["S"], w["blk"], w["T"])
    finite = dist[(dist >= 1) & (dist <= 252)]
    steps = int(finite.max()) + 1
    standing, nb, ns = _standing_env(torch, _dev(torch), w["S"], w["T"], w["mc"], w["blk"], w["tgt"], valid, cells, max_steps=1000)
    out = standing.rollout_policy(steps, w["policy"], select="greedy", epsilon=0.0, stats=("first_win", "wins"))
    d = dist[nb, ns].astype(np.int64)
    first = out.first_win.cpu().numpy()
    start_won = d == 0       # a board that stands on a won placement is not done: its first step un-wins it or not; it is left out
    assert np.array_equal(first[(d >= 1) & (d <= 252)], d[(d >= 1) & (d <= 252)])
    assert not first[d == 255].any() and (d == 255).sum() >= 20 and not out.wins.cpu().numpy()[d == 255].any()
    assert start_won.sum() == 2


def test_refusals_of_the_wrapper(torch_cuda, oracle, two_levels):
    from tiler_slider_amd import DistanceTable, VecTilerSliderEnv
    torch, w = torch_cuda, two_levels
    env = w["env"]
    pt, table = env.build_policy_table(w["policy"]), env.build_table()
    with pytest.raises(TypeError):
        env.build_policy_table("greedy")
    with pytest.raises(ValueError):
        env.build_policy_table(w["policy"], max_depth=253)
    with pytest.raises(ValueError):
        env.build_policy_table(w["policy"], max_bytes=100)
    with pytest.raises(TypeError):
        env.walk_actions(pt.act.int())
    with pytest.raises(ValueError):
        env.walk_actions(pt.act[:, :100])
    with pytest.raises(ValueError):
        env.walk_actions(pt.act, max_depth=-1)
    with pytest.raises(TypeError):
        env.score_policy(table, table)                # a DistanceTable has no actions
    with pytest.raises(TypeError):
        env.score_policy(pt, pt.dist)
    other = VecTilerSliderEnv.from_arrays(4, w["blk"], np.zeros((2, 2), np.uint8), w["tgt"], multi_color=False, device=env.device, obs_dtype=None)
    with pytest.raises(ValueError):
        other.score_policy(pt, table)                 # another shape
    with pytest.raises(ValueError):
        other.build_policy_table(w["policy"])         # the network reads other features
    big = VecTilerSliderEnv.from_arrays(5, *oracle.generate(5, 4, 4, 2, 2, seed=1), device=env.device, obs_dtype=None)
    with pytest.raises(ValueError):
        big.walk_actions(pt.act)
    assert isinstance(table, DistanceTable)


def test_a_call_on_a_stream_of_its_own_behind_a_step(torch_cuda, oracle, two_levels):
    torch, w = torch_cuda, two_levels
    env = w["env"]
    env.reset()
    side = torch.cuda.Stream(device=env.device)
    env.step(torch.zeros(env.num_envs, dtype=torch.uint8, device=env.device))
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        pt = env.build_policy_table(w["policy"], logits=True)
        score = env.score_policy(pt, env.build_table())
    side.synchronize()
    assert np.array_equal(pt.dist.cpu().numpy(), w["dist"]) and np.array_equal(pt.act.cpu().numpy(), w["act"])
    assert int(score.valid.sum()) == int((w["dist"] != 253).sum())


# ---------------------------------------------------------------------------------------------------------------- occupancy
# size -> (tiles, obstacles) of the occupancy cases, as tests/table_harness.py; 2x2 takes no obstacle here
_OCC = {1: (1, 0), 2: (2, 0), 3: (2, 1), 4: (2, 2), 5: (2, 3), 6: (2, 6), 7: (2, 8), 8: (2, 10)}
_BLOCK_OCC = {2: (4, 0), 3: (3, 1), 4: (2, 2), 5: (2, 3), 6: (2, 6), 7: (2, 8), 8: (2, 10)}   # index spaces of at least 256 placements
WAVES = 4096


def _occupancy_cases():
    cases = []
    for S in range(1, 9):
        cases.append((f"k_ptable_actions<{S}>", S, *_OCC[S]))
        cases.append((f"k_ptable_walk_wave<{S}>", S, 1, _OCC[S][1]))
        if S >= 2:
            cases.append((f"k_ptable_walk_block<{S}>", S, *_BLOCK_OCC[S]))
        cases.append((f"k_ptable_score<{S}>", S, 1, _OCC[S][1]))
    return cases


@pytest.mark.parametrize("name,S,T,K", _occupancy_cases(), ids=[c[0] for c in _occupancy_cases()])
def test_every_compiled_kernel_at_4096_waves(torch_cuda, oracle, name, S, T, K):
    from tiler_slider_amd import _ptable_cabi as xc
    torch, dev = torch_cuda, _dev(torch_cuda)
    states, mc = (S * S) ** T, S % 2 == 0
    pow2 = lambda v: 1 << (v - 1).bit_length()
    rng = np.random.default_rng(S)
    if "actions" in name:
        L = -(-WAVES * 64 // states)
    elif "block" in name:
        L = WAVES // 4
    else:
        L = WAVES * (64 // min(64, pow2(states)))
    blk, tgt = _levels(oracle, S, T, T, K, L, seed=41 + S)
    dims = _dims(S, T, T, mc, L)
    if "actions" in name:
        d = xc.describe_ptable_actions(dims, 7)
        mlp = pref.random_mlp(rng, (1 + 2 * T if mc else 3) * S * S, 7, "int")
        act, z, _ = xref.actions(oracle, S, mc, blk, tgt, T, mlp, True)
        bad = _run_all(torch, dev, S, T, T, mc, blk, tgt, dict(act=act, logits=z), mlp=mlp)
        waves = d["blocks"] * d["threads_per_block"] // 64
    else:
        act = _mixed_actions(oracle, rng, S, T, mc, blk, tgt)
        dist = xref.walk(oracle, S, mc, blk, tgt, T, act)
        if "walk" in name:
            d = xc.describe_ptable_walk(dims)
            bad = _run_all(torch, dev, S, T, T, mc, blk, tgt, dict(dist=dist), act_in=act)
        else:
            d = xc.describe_ptable_score(dims)
            table = tref.table(oracle, S, mc, blk, tgt, T)
            want = dict(dist=dist, score=xref.score(oracle, S, mc, blk, tgt, T, dist, act, table))
            bad = _run_all(torch, dev, S, T, T, mc, blk, tgt, want, act_in=act, table=table)
        waves = d["blocks"] * d["threads_per_block"] // 64
    assert d["name"] == name and waves >= WAVES, (d, waves)
    assert bad == []
