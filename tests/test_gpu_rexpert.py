"""ts_rexpert_rollout and ts_rexpert_labels on the GPU against the CPU yardstick (tests/rexpert_reference.py: the loop of
include/tiler_slider_rexpert.h over the oracle, with tests/rtable_reference.py's sorted keys for the expert move), against the
dense path where both apply, and against the loop of existing entry points the fused launch replaces.  Exact equality everywhere.
The raw C-ABI calls read a state and write outputs that lie between guard bytes the test owns; outputs are prefilled with the
bytewise complement of the yardstick's answer, so an element the kernel skips differs by construction."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 4, 5, 6, 8)
STATS = ("wins", "finished", "first_win", "win_moves", "reward_sum", "flags")
LOGS = ("act_log", "flags_log", "pos_log")
OUT_DTYPES = dict(wins=np.int32, finished=np.int32, first_win=np.int32, win_moves=np.int32, reward_sum=np.int32, flags=np.uint8, act_log=np.uint8,
                  flags_log=np.uint8, pos_log=np.uint8)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _oracle():
    from oracle import binding
    return binding


@functools.lru_cache(maxsize=None)
def _base(S, mc, mode):
    """(ref, blk, init, tgt, want) of the base case, computed once.  Do not write to it."""
    import rexpert_reference as rx
    return rx.base_case(_oracle(), S, mc, mode)


@functools.lru_cache(maxsize=None)
def _levels(S, mc):
    import reach_cases as cases
    import rtable_reference as rt
    blk, init, tgt = cases.levels(_oracle(), S, mc)
    return blk, init, tgt, rt.build(_oracle(), S, mc, blk, tgt, init, 252, cases.CAPACITY)


def _env(S, mc, blk, init, tgt, pos=None, **kw):
    import torch
    from tiler_slider_amd import VecTilerSliderEnv
    kw.setdefault("obs_dtype", None)
    env = VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=mc, **kw)
    env.reset()
    if pos is not None:
        env._pos.copy_(torch.from_numpy(np.ascontiguousarray(pos)).to(env._pos.device))
    return env


def _table(S, mc, blk, init, tgt, capacity=None, root="init", max_depth=252, pos=None):
    import reach_cases as cases
    return _env(S, mc, blk, init, tgt, pos=pos).build_reach_table(capacity=cases.CAPACITY if capacity is None else capacity, root=root, max_depth=max_depth)


class _State:
    """A ts_state whose six rows lie between guard bytes."""

    ROWS = ("pos", "init", "tgt", "blk", "step_count", "done")

    def __init__(self, torch, dev, S, mc, max_steps, blk, init, tgt, pos=None, step_count=None, done=None):
        from table_harness import guarded
        from tiler_slider_amd import _cabi
        n = blk.shape[1]
        self.torch, self.n, self.T = torch, n, init.shape[0]
        self.host = dict(pos=np.ascontiguousarray(init if pos is None else pos, np.uint8), init=np.ascontiguousarray(init, np.uint8),
                         tgt=np.ascontiguousarray(tgt, np.uint8), blk=np.ascontiguousarray(blk, np.uint32),
                         step_count=np.zeros(n, np.int32) if step_count is None else np.ascontiguousarray(step_count, np.int32),
                         done=np.zeros(n, np.uint8) if done is None else np.ascontiguousarray(done, np.uint8))
        self.bufs = {k: guarded(torch, dev, v) for k, v in self.host.items()}
        self.dims = _cabi.Dims(n, S, init.shape[0], tgt.shape[0], int(mc), max_steps, 0)
        from table_harness import GUARD
        self.state = _cabi.State(*(self.bufs[k].data_ptr() + GUARD for k in self.ROWS))

    def read(self):
        """The six rows after a call, every guard byte checked."""
        from table_harness import payload
        return {k: payload(self.bufs[k], v.dtype, v.shape) for k, v in self.host.items()}


def _raw_rollout(torch, st, rtab, steps, mode, want, ask=None, write_state=1, rows=None, threshold=0, seed=0, step_index=0, board_offset=0,
                 stream=None, describe=True):
    """ts_rexpert_rollout through the C-ABI on the guarded state `st`: {name: array} of the outputs asked for; an output not asked
    for is passed as NULL and must keep its fill."""
    from table_harness import GUARD, guarded, payload
    from tiler_slider_amd import _rexpert_cabi as ec
    ask = ec.OUT_FIELDS if ask is None else ask
    dev = rtab.table.device if rtab is not None else torch.device("cuda", 0)
    n, T = st.n, st.T
    shapes = {k: (n,) for k in STATS}
    shapes.update(act_log=(steps, n), flags_log=(steps, n), pos_log=(steps, T, n))
    fills = {k: (np.full(shapes[k], 77, OUT_DTYPES[k]) if want is None else ~np.asarray(want[k]).astype(OUT_DTYPES[k])) for k in ec.OUT_FIELDS}
    bufs = {k: guarded(torch, dev, fills[k]) for k in ec.OUT_FIELDS}
    r = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(dev)
    cfg = ec.RexpertCfg(steps, mode, write_state, 0, seed, step_index, board_offset, threshold,
                        None if rtab is None else rtab.table.data_ptr(), 2 if rtab is None else rtab.slots, None if rtab is None else rtab.count.data_ptr(),
                        0 if rtab is None else len(rtab), None if r is None else r.data_ptr())
    if describe and steps and n:
        d = ec.describe_rexpert_rollout(st.dims, cfg)
        assert (d["name"], d["blocks"], d["lds_bytes"]) == (f"k_rexpert_rollout<{st.dims.size}>", -(-n // 256), 0)
    out = ec.RolloutOut(*(bufs[k].data_ptr() + GUARD if k in ask else None for k in ec.OUT_FIELDS))
    s = torch.cuda.current_stream(dev) if stream is None else stream
    code = ec.lib().ts_rexpert_rollout(C.byref(st.dims), C.byref(st.state), C.byref(cfg), C.byref(out), s.cuda_stream)
    assert code == 0, code
    s.synchronize()
    got = {k: payload(bufs[k], OUT_DTYPES[k], shapes[k]) for k in ec.OUT_FIELDS}
    for k in ec.OUT_FIELDS:
        if k not in ask:
            np.testing.assert_array_equal(got[k], fills[k], err_msg=f"{k} was not asked for and was written")
    return {k: got[k] for k in ask}


def _raw_labels(torch, st, rtab, first, pos_log, steps, want=None, ask=(True, True, True), rows=None):
    """ts_rexpert_labels through the C-ABI: (moves, best, action) [K, N], each between guard bytes."""
    from table_harness import GUARD, guarded, payload
    from tiler_slider_amd import _rexpert_cabi as ec
    dev = rtab.table.device
    n = st.n
    dts = (np.int16, np.uint8, np.uint8)
    fills = [np.full((steps, n), 77, dt) if want is None else ~np.asarray(want[i]).astype(dt) for i, dt in enumerate(dts)]
    bufs = [guarded(torch, dev, f) for f in fills]
    f = guarded(torch, dev, np.ascontiguousarray(first, np.uint8))
    pl = None if pos_log is None else guarded(torch, dev, np.ascontiguousarray(pos_log, np.uint8))
    r = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(dev)
    tin = ec.RexpertLabelsIn(f.data_ptr() + GUARD, None if pl is None else pl.data_ptr() + GUARD, rtab.table.data_ptr(), rtab.count.data_ptr(),
                             None if r is None else r.data_ptr(), rtab.slots, len(rtab), steps, 0)
    tout = ec.LabelsOut(*(bufs[i].data_ptr() + GUARD if ask[i] else None for i in range(3)))
    what = sum(b for b, a in zip((1, 2, 4), ask) if a)
    d = ec.describe_rexpert_labels(st.dims, steps, what)
    assert (d["name"], d["blocks"], d["samples"]) == (f"k_rexpert_labels<{st.dims.size}>", -(-n // 256) * steps, steps * n)
    s = torch.cuda.current_stream(dev)
    code = ec.lib().ts_rexpert_labels(C.byref(st.dims), C.byref(st.state), C.byref(tin), C.byref(tout), s.cuda_stream)
    assert code == 0, code
    s.synchronize()
    got = [payload(b, dt, (steps, n)) for b, dt in zip(bufs, dts)]
    for i in range(3):
        if not ask[i]:
            np.testing.assert_array_equal(got[i], fills[i], err_msg="an output that was not asked for was written")
    return tuple(got)


def _same(got, want, ctx, names=None):
    import rexpert_reference as rx
    for k in (rx.OUTPUTS if names is None else names):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k}: {ctx}")


def _same_state(st, want, ctx):
    now = st.read()
    for k in ("pos", "step_count", "done"):
        np.testing.assert_array_equal(now[k], want[k].astype(now[k].dtype), err_msg=f"state {k}: {ctx}")
    for k in ("init", "tgt", "blk"):
        np.testing.assert_array_equal(now[k], st.host[k], err_msg=f"the level's {k} was written: {ctx}")


# ---------------------------------------------------------------------------------------------------- 1. all outputs and state
@pytest.mark.parametrize("mode", (1, 0), ids=("autoreset", "strict"))
@pytest.mark.parametrize("mc", (False, True))
@pytest.mark.parametrize("S", SIZES)
def test_all_outputs_and_state_of_the_base_case(torch_cuda, S, mc, mode):
    import rexpert_reference as rx
    torch = torch_cuda
    ref, blk, init, tgt, want = _base(S, mc, mode)
    print(S, mc, mode, rx.check_base(S, mode, want))      # the caps against a vacuous pass, on the yardstick, before any GPU call
    rtab = _table(S, mc, blk, init, tgt)
    np.testing.assert_array_equal(rtab.count.cpu().numpy(), ref.count)
    b = rx.BASE
    for write_state in (1, 0):
        st = _State(torch, rtab.table.device, S, mc, b["max_steps"], blk, init, tgt)
        got = _raw_rollout(torch, st, rtab, b["steps"], mode, want, write_state=write_state, threshold=rx.threshold_of(b["epsilon"]), seed=b["seed"])
        _same(got, want, (S, mc, mode, write_state))
        _same_state(st, want if write_state else st.host, (S, mc, mode, write_state))


# ---------------------------------------------------------------------------------------------------- 2. the shortest path
@pytest.mark.parametrize("mc", (False, True))
@pytest.mark.parametrize("S", SIZES)
def test_the_expert_wins_by_the_shortest_path(torch_cuda, S, mc):
    import rexpert_reference as rx
    import rtable_reference as rt
    torch = torch_cuda
    K, max_steps = 32, 64
    blk, init, tgt, ref = _levels(S, mc)
    near, never = (ref.root_moves >= 1) & (ref.root_moves <= K), ref.root_moves == rt.SOLVE_NONE
    assert near.sum() >= 11 and (S < 3 or never.sum() >= 10), (near.sum(), never.sum())
    want = rx.rollout(_oracle(), ref, S, mc, max_steps, blk, init, tgt, K, 0, threshold=0, seed=7)
    rtab = _table(S, mc, blk, init, tgt)
    st = _State(torch, rtab.table.device, S, mc, max_steps, blk, init, tgt)
    got = _raw_rollout(torch, st, rtab, K, 0, want, seed=7)
    _same(got, want, (S, mc))
    np.testing.assert_array_equal(got["first_win"][near], ref.root_moves[near])
    assert (got["wins"][never] == 0).all()
    best = rx.labels(_oracle(), ref, blk, tgt, init, got["pos_log"], K)[1]
    for n in np.flatnonzero(near):
        for k in range(ref.root_moves[n]):
            assert (best[k, n] >> got["act_log"][k, n]) & 1, (S, mc, n, k)


def test_a_deep_level_is_played_to_its_win(torch_cuda, oracle):
    """One level of tests/golden/deep_levels.npz, rooted (root="pos") on a placement at its deepest distance: without exploration
    the expert wins it in exactly that many steps."""
    import deep_cases
    torch = torch_cuda
    lv = next(iter(deep_cases.levels().values()))
    dist = deep_cases.exact(oracle, lv)
    far = deep_cases.deepest(dist)
    start = deep_cases.cells_of(lv, np.flatnonzero(dist == far)[:1])
    env = _env(lv.S, lv.mc, lv.blk, lv.init, lv.tgt, pos=start, max_steps=300)
    rtab = env.build_reach_table(capacity=1 << 14, root="pos")
    assert rtab.root_moves.tolist() == [far] and far >= 37
    out = env.rollout(far, "reach", table=rtab, epsilon=0.0, log=("flags",))
    assert out.first_win.tolist() == [far] and out.wins.tolist() == [1] and env.done.tolist() == [True] and env.is_won().tolist() == [True]
    assert int((out.flags_log[:-1] != 0).sum()) == 0   # every step before the last moved the board and did not win


# ---------------------------------------------------------------------------------------------------- 3. against the dense path
@pytest.mark.parametrize("S,T,K", ((4, 2, 2), (3, 4, 1)))
@pytest.mark.parametrize("mc", (False, True))
def test_equals_the_table_policy_where_play_stays_inside_R(torch_cuda, S, T, K, mc):
    """From a root that is neither won nor FULL play never leaves R, so the reach table answers what the dense table answers."""
    torch = torch_cuda
    blk, init, tgt = _oracle().generate_mt19937(S, T, T, K, np.arange(96, dtype=np.uint32))
    every = _env(S, mc, blk, init, tgt)
    rt_all = every.build_reach_table(capacity=4096)
    keep = ((rt_all.count > 0)).cpu().numpy()
    assert keep.sum() >= 48
    blk, init, tgt = (np.ascontiguousarray(a[:, keep]) for a in (blk, init, tgt))
    steps = 40
    outs = []
    for policy in ("reach", "table"):
        env = _env(S, mc, blk, init, tgt, auto_reset=True, max_steps=12)
        table = env.build_reach_table(capacity=4096) if policy == "reach" else env.build_table()
        out = env.rollout(steps, policy, table=table, epsilon=0.25, seed=11, log=("start", "act", "flags", "pos"))
        outs.append((out, env.positions.clone(), env.step_count.clone(), env.done.clone()))
    (a, *sa), (b, *sb) = outs
    for name in a.FIELDS + ("start_pos",):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for x, y in zip(sa, sb):
        assert torch.equal(x, y)
    # caps against a vacuous pass: boards win (3x3 with four tiles in multi colour rarely can) and are reset, and the expert played -
    # the actions are not the draw's
    rnd = np.stack([_oracle().fill_actions(blk.shape[1], seed=11, step_index=k) for k in range(steps)])
    assert int(a.wins.sum()) >= 1 and int((a.flags_log & 0x20).ne(0).sum()) >= 20 and int((a.act_log.cpu().numpy() != rnd).sum()) >= 50


# ---------------------------------------------------------------------------------------------------- 4. labels
@pytest.mark.parametrize("mc", (False, True))
@pytest.mark.parametrize("S", SIZES)
def test_labels_on_the_base_cases_logs(torch_cuda, S, mc):
    import rexpert_reference as rx
    torch = torch_cuda
    ref, blk, init, tgt, run = _base(S, mc, 1)
    K = rx.BASE["steps"]
    want = rx.labels(_oracle(), ref, blk, tgt, init, run["pos_log"], K)
    kinds = rx.kinds_of(want[0])
    assert S < 3 or kinds.min() >= 50, kinds
    rtab = _table(S, mc, blk, init, tgt)
    st = _State(torch, rtab.table.device, S, mc, 12, blk, init, tgt)
    for ask in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
        got = _raw_labels(torch, st, rtab, init, run["pos_log"], K, want, ask)
        for i, name in enumerate(("moves", "best", "action")):
            if ask[i]:
                np.testing.assert_array_equal(got[i], want[i], err_msg=f"{name}: {(S, mc, ask)}")
    one = _raw_labels(torch, st, rtab, init, None, 1, [w[:1] for w in want])       # steps == 1: pos_log NULL
    for g, w in zip(one, want):
        np.testing.assert_array_equal(g, w[:1])
    _same_state(st, st.host, (S, mc))
    # the Python path, on a Rollout of the same logs
    from tiler_slider_amd import Rollout
    env = _env(S, mc, blk, init, tgt)
    dev = env.device
    ro = Rollout(K, start_pos=torch.from_numpy(init).to(dev), pos_log=torch.from_numpy(run["pos_log"]).to(dev))
    for g, w in zip(env.trajectory_labels(ro, rtab), want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)


def _walked_5x5(n=256):
    import reach_cases as cases
    blk, init, tgt = _oracle().generate_mt19937(5, 4, 4, 3, np.arange(n, dtype=np.uint32))
    return blk, init, np.ascontiguousarray(cases.walked(_oracle(), 5, blk, init))


def test_labels_of_a_network_trajectory_are_the_lookups_board_by_board(torch_cuda):
    torch = torch_cuda
    from tiler_slider_amd import PolicyNet
    blk, init, tgt = _walked_5x5()
    env = _env(5, True, blk, init, tgt, auto_reset=True, max_steps=10)
    rtab = env.build_reach_table()
    net = PolicyNet(env.onehot_channels * 25, 16, env.device, generator=torch.Generator(device=env.device).manual_seed(3))
    K = 12
    out = env.rollout_policy(K, net.policy(), select="sample", seed=5, log=("start", "pos"))
    moves, best, action = env.trajectory_labels(out, rtab)
    twin = _env(5, True, blk, init, tgt)
    for k in range(K):
        twin._pos.copy_(out.start_pos if k == 0 else out.pos_log[k - 1])
        m, b = twin.lookup_bits(rtab)
        assert torch.equal(moves[k], m) and torch.equal(best[k], b) and torch.equal(action[k], twin.expert_actions_from(rtab)), k
    assert int((action != 255).sum()) >= 100


# ---------------------------------------------------------------------------------------------------- 5. edges of the probe and the key
def _check_rollout_and_labels(torch, S, mc, blk, init, tgt, ref, rtab, ctx, steps=12, max_steps=6, mode=1, rows=None, pos=None, seed=3, raw=None):
    """A rollout of `steps` steps with a quarter explored and the labels of its log, both against the yardstick; returns its answer.
    raw = (cells, targets): what the kernels read in place of init (and pos) and tgt - ids beyond the board, which the yardstick
    is handed clamped, as tests/test_gpu_rollout.py hands them to the oracle."""
    import rexpert_reference as rx
    want = rx.rollout(_oracle(), ref, S, mc, max_steps, blk, init, tgt, steps, mode, pos=pos, rows=rows, threshold=1 << 30, seed=seed)
    st = _State(torch, rtab.table.device, S, mc, max_steps, blk, init if raw is None else raw[0], tgt if raw is None else raw[1], pos=pos)
    got = _raw_rollout(torch, st, rtab, steps, mode, want, rows=rows, threshold=1 << 30, seed=seed)
    _same(got, want, ctx)
    _same_state(st, want, ctx)
    first = init if pos is None else pos
    lab = rx.labels(_oracle(), ref, blk, tgt, first, want["pos_log"], steps, rows)
    for g, w, name in zip(_raw_labels(torch, st, rtab, first if raw is None else raw[0], want["pos_log"], steps, lab, rows=rows), lab, ("moves", "best", "action")):
        np.testing.assert_array_equal(g, w, err_msg=f"{name}: {ctx}")
    return want, lab


# 2x2 boards of one tile whose play reaches 1, 1, 2, 3 and 3 placements that are not won, and one that is won as it stands
TINY = (([(1, 0), (1, 1)], [(0, 0)], [(0, 1)]), ([(1, 0), (1, 1)], [(0, 1)], [(0, 0)]), ([(1, 1)], [(0, 0)], [(1, 0)]), ([], [(0, 0)], [(1, 1)]),
        ([], [(1, 0)], [(0, 1)]), ([(1, 1)], [(0, 1)], [(0, 1)]))


@pytest.mark.parametrize("capacity", (1, 2, 3))
def test_tiny_tables_where_every_probe_wraps(torch_cuda, oracle, capacity):
    """Rows of 2, 4 and 8 slots, the rows that hold exactly `capacity` states among them: half full, so a probe that misses its home
    slot walks round the end of the row; levels above the capacity are FULL."""
    import rtable_reference as rt
    torch = torch_cuda
    S = 2
    blk, init, tgt = (np.ascontiguousarray(np.tile(a, (1, 11))) for a in oracle.pack_levels(S, TINY))
    for mc in (False, True):
        ref = rt.build(oracle, S, mc, blk, tgt, init, 252, capacity)
        assert sorted(ref.count[:6].tolist()) == sorted(c if c <= capacity else rt.SOLVE_FULL for c in (1, 1, 2, 3, 3, 0))
        rtab = _table(S, mc, blk, init, tgt, capacity=capacity)
        assert rtab.slots == (2, 4, 8)[capacity - 1]
        want, lab = _check_rollout_and_labels(torch, S, mc, blk, init, tgt, ref, rtab, (capacity, mc), steps=16, max_steps=5)
        assert (lab[0] >= 1).sum() >= 50 and ((lab[0] == rt.SOLVE_FULL).sum() >= 50 or capacity == 3)


def test_eight_tiles_and_keys_beyond_2_to_the_32(torch_cuda):
    import reach_cases as cases
    import rexpert_reference as rx
    torch = torch_cuda
    for mc in (False, True):
        blk, init, tgt, ref = _levels(8, mc)
        assert cases.SHAPES[8][:2] == (8, 38) and cases.check_rtable(8, ref)["long_keys"] >= 1000
        want, lab = _check_rollout_and_labels(torch, 8, mc, blk, init, tgt, ref, _table(8, mc, blk, init, tgt), (8, mc))
        assert rx.kinds_of(lab[0])[0] >= 100 and want["source"][0] >= 100


@pytest.mark.parametrize("S", (3, 5, 6))
def test_tables_rooted_on_the_cells_as_they_stand(torch_cuda, S):
    import reach_cases as cases
    import rtable_reference as rt
    torch = torch_cuda
    mc = S != 5
    blk, init, tgt, _ = _levels(S, mc)
    _, pos = cases.stepped(_oracle(), S, mc, blk, init, tgt)
    ref = rt.build(_oracle(), S, mc, blk, tgt, pos, 252, cases.CAPACITY)
    rtab = _table(S, mc, blk, init, tgt, root="pos", pos=pos)
    np.testing.assert_array_equal(rtab.count.cpu().numpy(), ref.count)
    # strict mode from the root the table was built on: no auto-reset takes a board back to cells the table may not hold
    _check_rollout_and_labels(torch, S, mc, blk, init, tgt, ref, rtab, S, mode=0, pos=pos)
    _check_rollout_and_labels(torch, S, mc, blk, init, tgt, ref, rtab, S, mode=1, pos=pos)


@pytest.mark.parametrize("depth", (0, 3))
def test_deep_entries_give_no_move(torch_cuda, depth):
    import reach_cases as cases
    import rtable_reference as rt
    torch = torch_cuda
    S, mc = 5, True
    blk, init, tgt, _ = _levels(S, mc)
    ref = rt.build(_oracle(), S, mc, blk, tgt, init, depth, cases.CAPACITY)
    assert (ref.entry == rt.DEEP).sum() >= 100
    want, lab = _check_rollout_and_labels(torch, S, mc, blk, init, tgt, ref, _table(S, mc, blk, init, tgt, max_depth=depth), depth)
    assert (lab[0] == rt.SOLVE_DEPTH).sum() >= 50 and ((lab[0] >= 1).sum() >= 10 or depth == 0) and (lab[0] > depth).sum() == 0


def test_rows_out_of_range_and_fewer_levels_than_boards(torch_cuda):
    import rtable_reference as rt
    torch = torch_cuda
    S, mc = 4, False
    blk, init, tgt, ref = _levels(S, mc)
    L = 40
    small = rt.build(_oracle(), S, mc, blk[:, :L], tgt[:, :L], init[:, :L], 252, 1024)
    rtab = _table(S, mc, *(np.ascontiguousarray(a[:, :L]) for a in (blk, init, tgt)))
    n = blk.shape[1]
    rows = np.arange(n, dtype=np.int32)
    rows[L:] = np.resize(np.array([-1, L, L + 5, 2**31 - 1, -2**31], np.int64), n - L).astype(np.int32)
    rows[L:L + 30:3] = np.arange(10)   # and some boards beyond the table's levels read a row of their own level's twin
    lv = np.where((rows >= 0) & (rows < L), rows, 0)
    twin = rows[L:L + 30:3]
    b, i, t = blk.copy(), init.copy(), tgt.copy()
    for a in (b, i, t):
        a[:, L:L + 30:3] = a[:, twin]
    want, lab = _check_rollout_and_labels(torch, S, mc, b, i, t, small, rtab, "rows", rows=rows)
    outside = (rows < 0) | (rows >= L)
    assert (lab[0][:, outside] == rt.SOLVE_NONE).all() and (lab[2][:, outside] == 255).all() and outside.sum() >= 60
    # no table at all: every board plays the draw
    st = _State(torch, rtab.table.device, S, mc, 6, blk, init, tgt)
    import rexpert_reference as rx
    none = rx.rollout(_oracle(), small, S, mc, 6, blk, init, tgt, 5, 1, rows=np.full(n, -1), threshold=0, seed=9)
    _same(_raw_rollout(torch, st, None, 5, 1, none, seed=9), none, "n_rows = 0")
    assert none["source"].tolist() == [0, 0, 5 * n]


def test_unequal_tile_and_target_counts_repeated_targets_and_cells_beyond_the_board(torch_cuda, oracle):
    import rtable_reference as rt
    torch = torch_cuda
    S, n = 4, 64
    blk, init, _ = oracle.generate_mt19937(S, 3, 3, 2, np.arange(n, dtype=np.uint32))
    cases = []
    tgt2 = np.ascontiguousarray(init[:2])                       # T = 3, Tt = 2: multi colour can never win, single colour neither
    cases.append(("T != Tt", init, tgt2))
    walked = __import__("reach_cases").walked(oracle, S, blk, init)
    rep = walked.copy()
    rep[2] = rep[1]                                             # a repeated target
    cases.append(("repeated", init, np.ascontiguousarray(np.concatenate([rep, rep[:1]]))))   # Tt = 4 > T, with a repeat
    far = walked.copy()
    far[0, ::2] = 200                                           # target ids beyond the board: they read as cell 15
    free = (((blk[0] >> 15) & 1) == 0) & ~(init[[0, 2]] == 15).any(axis=0)   # cell 15 holds no obstacle and no other tile
    assert free.sum() >= 16
    pos = init.copy()
    pos[1, free] = 255                                          # and cell ids beyond it, where cell 15 is a placement for tile 1
    cases.append(("beyond", pos, far))
    for name, raw_cells, raw_tgt in cases:
        cells, tgt = np.minimum(raw_cells, S * S - 1), np.minimum(raw_tgt, S * S - 1)
        for mc in (False, True):
            ref = rt.build(oracle, S, mc, blk, tgt, cells, 252, 4096)
            rtab = _env(S, mc, blk, cells, tgt).build_reach_table()
            np.testing.assert_array_equal(rtab.count.cpu().numpy(), ref.count)
            # no board is done on entry and every action is a move: the first step stores clamped cells, whatever the bytes were
            _check_rollout_and_labels(torch, S, mc, blk, cells, tgt, ref, rtab, (name, mc), raw=(raw_cells, raw_tgt))


def _home(key, slots):
    return (((int(key) * 0x9e3779b97f4a7c15) & ((1 << 64) - 1)) >> 32) >> (32 - (slots.bit_length() - 1))


def _host_rows(ref, slots):
    """uint64 [L, slots] by the format of include/tiler_slider_rtable.h alone: bit 63 | entry << 48 | key, in the first free slot from
    home(key), keys in DESCENDING order (no build lays them out so)."""
    L = len(ref.count)
    table = np.zeros((L, slots), np.uint64)
    for lv in range(L):
        if ref.count[lv] < 0:
            table[lv] = np.uint64(0x0123456789abcdef)   # a FULL row holds nothing a lookup may use
            continue
        for key, entry in zip(ref.keys(lv)[::-1], ref.entries(lv)[::-1]):
            s = _home(key, slots)
            while table[lv, s]:
                s = (s + 1) % slots
            table[lv, s] = np.uint64((1 << 63) | (int(entry) << 48) | int(key))
    return table


def test_rows_filled_on_the_host_and_rows_of_arbitrary_bytes(torch_cuda):
    import rtable_reference as rt
    from tiler_slider_amd import ReachTable
    torch = torch_cuda
    S, mc, capacity, slots = 5, True, 64, 128
    blk, init, tgt, _ = _levels(S, mc)
    ref = rt.build(_oracle(), S, mc, blk, tgt, init, 252, capacity)
    assert ((ref.count > 8)).sum() >= 10 and (ref.count == rt.SOLVE_FULL).sum() >= 10
    dev = torch.device("cuda", 0)
    wrap = lambda table, count: ReachTable(torch.from_numpy(table.view(np.int64)).to(dev), torch.from_numpy(count.astype(np.int32)).to(dev), None, None, capacity,
                                           S, init.shape[0], tgt.shape[0], mc, 252, "init")
    _check_rollout_and_labels(torch, S, mc, blk, init, tgt, ref, wrap(_host_rows(ref, slots), ref.count), "host rows")
    # rows of zeros and of 0xA5 bytes, count claiming they are built: the header defines the answer - the row does not hold the
    # placement, no move, the draw plays - and the launch ends
    import rexpert_reference as rx
    n = blk.shape[1]
    for byte in (0x00, 0xA5):
        junk = wrap(np.full((n, slots), byte * 0x0101010101010101, np.uint64), np.full(n, 5))
        want = rx.rollout(_oracle(), ref, S, mc, 6, blk, init, tgt, 4, 1, rows=np.full(n, -1), threshold=1 << 30, seed=2)
        st = _State(torch, dev, S, mc, 6, blk, init, tgt)
        got = _raw_rollout(torch, st, junk, 4, 1, want, threshold=1 << 30, seed=2)
        _same(got, want, hex(byte))
        moves, best, action = _raw_labels(torch, st, junk, init, want["pos_log"], 4)
        won = np.stack([_oracle().OracleBatch(S, mc, 2**30, blk, c, tgt).won() != 0 for c in [init] + list(want["pos_log"][:3])])
        np.testing.assert_array_equal(moves, np.where(won, 0, rt.SOLVE_ABSENT))
        assert (best == 0).all() and (action == 255).all()


def test_one_cell_and_boards_without_tiles(torch_cuda, oracle):
    import rtable_reference as rt
    torch = torch_cuda
    one = (np.zeros((1, 2), np.uint32), np.zeros((1, 2), np.uint8))
    cases = [(1, one[0], one[1], tgt) for tgt in (np.zeros((1, 2), np.uint8), np.zeros((0, 2), np.uint8))]
    for S, level in ((3, ([(1, 1)], [], [])), (3, ([(1, 1)], [], [(0, 0)])), (8, ([], [], []))):
        cases.append((S,) + tuple(oracle.pack_levels(S, [level])))
    for S, blk, init, tgt in cases:
        for mc in (False, True):
            ref = rt.build(oracle, S, mc, blk, tgt, init, 252, 1)
            rtab = _table(S, mc, blk, init, tgt, capacity=1)
            _check_rollout_and_labels(torch, S, mc, blk, init, tgt, ref, rtab, (S, mc, tgt.shape), steps=5, max_steps=3)


# ---------------------------------------------------------------------------------------------------- 6. stream and replay
def test_step_index_board_offset_and_replay(torch_cuda):
    import rexpert_reference as rx
    torch = torch_cuda
    S, mc = 5, False
    ref, blk, init, tgt, want = _base(S, mc, 1)
    b = rx.BASE
    K, n, thr = b["steps"], blk.shape[1], rx.threshold_of(b["epsilon"])
    rtab = _table(S, mc, blk, init, tgt)
    dev = rtab.table.device
    # two rollouts of K / 2 equal one of K
    st = _State(torch, dev, S, mc, b["max_steps"], blk, init, tgt)
    a1 = _raw_rollout(torch, st, rtab, K // 2, 1, None, threshold=thr, seed=b["seed"])
    a2 = _raw_rollout(torch, st, rtab, K // 2, 1, None, threshold=thr, seed=b["seed"], step_index=K // 2)
    for k in LOGS:
        np.testing.assert_array_equal(np.concatenate([a1[k], a2[k]]), want[k], err_msg=k)
    for k in ("wins", "finished", "win_moves", "reward_sum"):
        np.testing.assert_array_equal(a1[k] + a2[k], want[k], err_msg=k)
    np.testing.assert_array_equal(a2["flags"], want["flags"])
    _same_state(st, want, "two halves in time")
    # two halves of the batch with board_offset equal the whole
    h = n // 2 + 3
    for lo, hi in ((0, h), (h, n)):
        part = [np.ascontiguousarray(a[:, lo:hi]) for a in (blk, init, tgt)]
        st = _State(torch, dev, S, mc, b["max_steps"], *part)
        got = _raw_rollout(torch, st, rtab, K, 1, {k: want[k][..., lo:hi] for k in rx.OUTPUTS}, rows=np.arange(lo, hi), threshold=thr, seed=b["seed"], board_offset=lo)
        _same(got, {k: want[k][..., lo:hi] for k in rx.OUTPUTS}, (lo, hi))
    # two runs are bit-equal, unasked outputs keep their fill (checked inside), a side stream behind a step()
    env = _env(S, mc, blk, init, tgt, auto_reset=True, max_steps=b["max_steps"])
    env.step(torch.from_numpy(_oracle().fill_actions(n, seed=1, step_index=0)))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        o1 = env.rollout(K, "reach", table=rtab, epsilon=b["epsilon"], seed=b["seed"], log=("act", "flags", "pos"), advance=False)
    side.synchronize()
    o2 = env.rollout(K, "reach", table=rtab, epsilon=b["epsilon"], seed=b["seed"], log=("act", "flags", "pos"), advance=False)
    for name in o1.FIELDS:
        assert torch.equal(getattr(o1, name), getattr(o2, name)), name
    st = _State(torch, dev, S, mc, b["max_steps"], blk, init, tgt)
    some = _raw_rollout(torch, st, rtab, K, 1, want, ask=("first_win", "act_log"), write_state=0, threshold=thr, seed=b["seed"])
    _same(some, want, "two outputs", names=("first_win", "act_log"))
    _same_state(st, st.host, "write_state = 0")


# ---------------------------------------------------------------------------------------------------- 7. the Python path
def test_advance_leaves_the_environment_where_the_loop_leaves_a_twin(torch_cuda):
    torch = torch_cuda
    blk, init, tgt = _walked_5x5(192)
    K = 14
    for obs_dtype in ("float32", None):
        env = _env(5, True, blk, init, tgt, auto_reset=True, max_steps=8, obs_dtype=obs_dtype)
        twin = _env(5, True, blk, init, tgt, auto_reset=True, max_steps=8, obs_dtype=obs_dtype)
        rtab = env.build_reach_table()
        out = env.rollout(K, "reach", table=rtab, epsilon=0.0, seed=4, log=("start", "act", "flags"))
        assert torch.equal(out.start_pos, torch.from_numpy(init).to(env.device))
        for k in range(K):
            e = twin.expert_actions_from(rtab)
            rnd = torch.from_numpy(_oracle().fill_actions(192, seed=4, step_index=k)).to(env.device)
            act = torch.where(e == 255, rnd, e)
            obs, done, info = twin.step(act)
            assert torch.equal(out.act_log[k], act) and torch.equal(out.flags_log[k], info["flags"]), k
        assert torch.equal(env.positions, twin.positions) and torch.equal(env.step_count, twin.step_count) and torch.equal(env.done, twin.done)
        assert torch.equal(env._flags, twin._flags) and out.flags is env._flags
        if obs_dtype is not None:
            assert torch.equal(env._obs, obs) and torch.equal(env._obs, env.encode())
        assert int(out.wins.sum()) >= 20
        # advance=False leaves every byte
        before = (env.positions.clone(), env.step_count.clone(), env.done.clone(), env._flags.clone())
        env.rollout(K, "reach", table=rtab, epsilon=0.5, seed=5, advance=False)
        for x, y in zip(before, (env.positions, env.step_count, env.done, env._flags)):
            assert torch.equal(x, y)


def test_the_errors_of_the_python_path(torch_cuda):
    torch = torch_cuda
    blk, init, tgt = _oracle().generate_mt19937(4, 2, 2, 2, np.arange(8, dtype=np.uint32))
    env = _env(4, False, blk, init, tgt)
    dense, rtab = env.build_table(), env.build_reach_table()
    with pytest.raises(TypeError, match="DistanceTable"):
        env.rollout(3, "table", table=rtab)
    with pytest.raises(TypeError, match="DistanceTable"):
        env.place_at_distance(rtab)
    with pytest.raises(TypeError, match="ReachTable"):
        env.rollout(3, "reach", table=dense)
    with pytest.raises(TypeError, match="ReachTable"):
        env.rollout(3, "reach")
    with pytest.raises(ValueError):
        env.rollout(3, "expert")
    with pytest.raises(ValueError):
        env.rollout(-1, "reach", table=rtab)
    with pytest.raises(ValueError):
        env.rollout(3, "reach", table=rtab, epsilon=1.5)
    with pytest.raises(ValueError):
        env.rollout(3, "reach", table=rtab, log=("logits",))
    with pytest.raises(ValueError):
        env.rollout(3, "reach", table=rtab, rows=torch.zeros(3, dtype=torch.int32))
    other = _env(4, True, blk, init, tgt)
    with pytest.raises(ValueError, match="built for"):
        other.rollout(3, "reach", table=rtab)
    few = _env(4, False, blk[:, :4], init[:, :4], tgt[:, :4])
    with pytest.raises(ValueError, match="rows"):
        few.rollout(3, "reach", table=rtab)
    out = few.rollout(3, "reach", table=rtab, rows=[0, 1, 2, 3], log=("start", "pos"))
    with pytest.raises(ValueError, match="rows"):
        few.trajectory_labels(out, rtab)
    with pytest.raises(ValueError, match="built for"):
        other.trajectory_labels(other.rollout(2, "random", log=("start", "pos")), rtab)
    with pytest.raises(ValueError, match="start"):
        few.trajectory_labels(few.rollout(2, "random", log=("pos",)), rtab, rows=[0, 1, 2, 3])
    # a DistanceTable takes the path it took
    moves, best, action = few.trajectory_labels(out, dense, rows=[0, 1, 2, 3])
    m2, b2, a2 = few.trajectory_labels(out, rtab, rows=[0, 1, 2, 3])
    assert moves.shape == m2.shape == (3, 4) and torch.equal(a2[moves >= 0], action[moves >= 0])
    assert few.rollout(0, "reach", table=rtab, rows=[0, 1, 2, 3]).steps == 0


def test_one_imitation_step_end_to_end(torch_cuda):
    """Play the network, label with the reach table, cross-entropy through trajectory_loss(labels=), FusedAdam: the gradients are
    finite and 30 steps lower the loss on the same batch (what tests/test_gpu_loss.py asks of the dense path: below where it began)."""
    torch = torch_cuda
    from tiler_slider_amd import FusedAdam, PolicyNet
    blk, init, tgt = _walked_5x5()
    env = _env(5, True, blk, init, tgt, auto_reset=True, max_steps=16)
    rtab = env.build_reach_table()
    net = PolicyNet(env.onehot_channels * 25, 32, env.device, generator=torch.Generator(device=env.device).manual_seed(0))
    opt = FusedAdam(net.parameters(), lr=1e-2)
    out = env.rollout_policy(16, net.policy(), select="sample", seed=1, log=("start", "pos"))
    labels = env.trajectory_labels(out, rtab)[2]
    assert int((labels != 255).sum()) >= 500
    losses = []
    for it in range(31):
        info = env.trajectory_loss(env.trajectory_logits(net, out), out, labels=labels)
        losses.append(float(info.loss.detach()))
        if it < 30:
            info.loss.backward()
            assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
            opt.step(zero_grad=True)
    print("cross-entropy on the reach table's labels:", [round(x, 3) for x in losses])
    assert losses[-1] < losses[0]


# ---------------------------------------------------------------------------------------------------- 8. every kernel at occupancy
@functools.lru_cache(maxsize=None)
def _occupancy(S):
    """(mc, the boards, rows, the yardstick's rollout, its labels) of the occupancy case of size S, computed once for both kernels."""
    import rexpert_cases as cases
    import rexpert_reference as rx
    mc = S % 2 == 0
    blk, init, tgt, ref = _levels(S, mc)
    rows = (np.arange(cases.N_BOARDS) % blk.shape[1]).astype(np.int32)
    big = [np.ascontiguousarray(a[:, rows]) for a in (blk, init, tgt)]
    want = rx.rollout(_oracle(), ref, S, mc, cases.MAX_STEPS, *big, cases.STEPS, 1, rows=rows, threshold=rx.threshold_of(cases.EPSILON), seed=cases.SEED)
    lab = rx.labels(_oracle(), ref, big[0], big[2], big[1], want["pos_log"], cases.STEPS, rows)
    return mc, big, rows, want, lab


@pytest.mark.parametrize("name", sorted(__import__("rexpert_cases").CASES))
def test_every_kernel_at_occupancy(torch_cuda, name):
    """4,096 waves of boards that replicate the 128 levels through rows=; the yardstick plays the 128 distinct boards once per
    block of board offsets it needs: board n draws from (seed, board_offset + n), so a replica is a board of its own."""
    import rexpert_cases as cases
    import rexpert_reference as rx
    from tiler_slider_amd import _rexpert_cabi as ec
    torch = torch_cuda
    S = cases.CASES[name][0]
    mc, big, rows, want, lab = _occupancy(S)
    blk, init, tgt, ref = _levels(S, mc)
    L, K = blk.shape[1], cases.STEPS
    thr = rx.threshold_of(cases.EPSILON)
    rtab = _table(S, mc, blk, init, tgt)
    st = _State(torch, rtab.table.device, S, mc, cases.MAX_STEPS, *big)
    if "rollout" in name:
        cfg = ec.RexpertCfg(K, 1, 1, 0, 0, 0, 0, thr, None, rtab.slots, None, L, None)
        d = ec.describe_rexpert_rollout(st.dims, cfg)
        assert (d["name"], d["waves"]) == (name, cases.WAVES)
        got = _raw_rollout(torch, st, rtab, K, 1, want, rows=rows, threshold=thr, seed=cases.SEED)
        _same(got, want, name)
        _same_state(st, want, name)
    else:
        d = ec.describe_rexpert_labels(st.dims, K)
        assert d["name"] == name and d["waves"] >= cases.WAVES
        got = _raw_labels(torch, st, rtab, big[1], want["pos_log"], K, lab, rows=rows)
        for g, w, what in zip(got, lab, ("moves", "best", "action")):
            np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")
