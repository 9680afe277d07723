"""ts_mixed_rollout on the GPU against the CPU yardstick (tests/mixed_reference.py: the definition of include/tiler_slider_mixed.h
over the oracle, policy_reference's network, table_reference's and rtable_reference's lookups), against the calls it fuses -
trajectory_labels, rollout_policy, rollout("table") / rollout("reach") - and, through the raw C-ABI, into guarded memory.
Integer weights everywhere an exact answer is asked for: float32 is exact on them in any order."""
import ctypes as C
import functools

import numpy as np
import pytest

import mixed_reference as mx
import policy_reference as pref
import rollout_reference as rref

pytestmark = pytest.mark.gpu

STRICT, AUTORESET = 0, 1
ALL_LOGS = ("start", "act", "flags", "pos", "logits", "expert", "moves", "best", "who")
LOG_NAMES = ("act_log", "flags_log", "pos_log", "logits_log", "expert_log", "moves_log", "best_log", "who_log")
B = mx.BASE
BASE_CASES = [(mx.REACH, S) for S in mx.REACH_SIZES] + [(mx.DENSE, shape) for shape in mx.DENSE_SHAPES]
CASE_IDS = [f"reach{c[1]}" if c[0] == mx.REACH else "dense" + "x".join(map(str, c[1])) for c in BASE_CASES]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _env(S, mc, blk, init, tgt, max_steps=B["max_steps"], mode=STRICT, **kw):
    from tiler_slider_amd import VecTilerSliderEnv
    kw.setdefault("obs_dtype", None)
    env = VecTilerSliderEnv.from_arrays(S, blk, init, tgt, multi_color=mc, max_steps=max_steps, auto_reset=mode == AUTORESET, **kw)
    env.reset()
    return env


def _policy(torch, env, mlp):
    from tiler_slider_amd import MlpPolicy
    return MlpPolicy(*(torch.from_numpy(np.ascontiguousarray(a)).to(env.device) for a in mlp))


def _table(kind, S, mc, blk, init, tgt):
    """The table of the levels, built on the GPU: a ReachTable at reach_cases.CAPACITY rooted on the initial cells, or a DistanceTable."""
    import reach_cases as cases
    env = _env(S, mc, blk, init, tgt)
    return env.build_reach_table(capacity=cases.CAPACITY) if kind == mx.REACH else env.build_table()


def _size(case):
    return case[1] if case[0] == mx.REACH else case[1][0]


def _check(got, env, want, ctx, names=mx.OUTPUTS):
    for k in names:
        np.testing.assert_array_equal(getattr(got, k).cpu().numpy(), want[k], err_msg=f"{k}: {ctx}")
    if env is not None:
        np.testing.assert_array_equal(env.positions.cpu().numpy(), want["pos"], err_msg=f"pos: {ctx}")
        np.testing.assert_array_equal(env.step_count.cpu().numpy(), want["step_count"], err_msg=f"step_count: {ctx}")
        np.testing.assert_array_equal(env.done.cpu().numpy(), want["done"].astype(bool), err_msg=f"done: {ctx}")


# ---------------------------------------------------------------------------------------------------- 1. byte for byte
@pytest.mark.parametrize("mode", (STRICT, AUTORESET), ids=("strict", "autoreset"))
@pytest.mark.parametrize("mc", (False, True))
@pytest.mark.parametrize("case", BASE_CASES, ids=CASE_IDS)
def test_every_output_equals_the_yardstick_byte_for_byte(torch_cuda, oracle, case, mc, mode):
    torch = torch_cuda
    kind, shape = case
    S = _size(case)
    (blk, init, tgt), _, mlp, want = mx.base_case(oracle, kind, shape, mc, mode)
    print(case, mc, mode, mx.check_base(kind, S, mode, want))      # the floors against a vacuous pass, before any GPU call
    sel = "sample" if mx.MODES[mode][0] == pref.SAMPLE else "greedy"
    env = _env(S, mc, blk, init, tgt, mode=mode)
    table = _table(kind, S, mc, blk, init, tgt)
    got = env.rollout_policy(B["steps"], _policy(torch, env, mlp), select=sel, epsilon=B["epsilon"], seed=B["seed"], log=ALL_LOGS, expert=table,
                             beta=B["beta"])
    _check(got, env, want, (case, mc, mode))
    np.testing.assert_array_equal(got.start_pos.cpu().numpy(), init)
    assert got.moves_log.dtype == torch.int16 and got.who_log.dtype == torch.uint8 and tuple(got.logits_log.shape) == (B["steps"], blk.shape[1], 4)


# ---------------------------------------------------------------------------------------------------- 2. labels
@pytest.mark.parametrize("kind,shape", ((mx.DENSE, (4, 4, 2)), (mx.REACH, 5)), ids=("dense", "reach"))
def test_the_three_label_logs_are_trajectory_labels_of_the_same_rollout(torch_cuda, oracle, kind, shape):
    """517 boards replicate the 128 levels through rows=; a board draws from (seed, n), so a replica is a board of its own."""
    torch = torch_cuda
    S = _size((kind, shape))
    for mc, mode in ((False, AUTORESET), (True, STRICT)):
        (blk, init, tgt), _, mlp, _ = mx.base_case(oracle, kind, shape, mc, mode)
        table = _table(kind, S, mc, blk, init, tgt)
        rows = (np.arange(517) * 5 % blk.shape[1]).astype(np.int32)
        env = _env(S, mc, *(np.ascontiguousarray(a[:, rows]) for a in (blk, init, tgt)), mode=mode)
        r = torch.from_numpy(rows).to(env.device)
        out = env.rollout_policy(B["steps"], _policy(torch, env, mlp), select="greedy", epsilon=B["epsilon"], seed=B["seed"],
                                 log=("start", "pos", "expert", "moves", "best"), expert=table, beta=B["beta"], rows=r)
        moves, best, action = env.trajectory_labels(out, table, rows=r)
        assert torch.equal(out.moves_log, moves) and torch.equal(out.best_log, best) and torch.equal(out.expert_log, action), (kind, mc, mode)
        assert int((action != 255).sum()) >= 500 and int((action == 255).sum()) >= 500 and len(torch.unique(moves)) >= 5


# ---------------------------------------------------------------------------------------------------- 3. beta = 0
@pytest.mark.parametrize("kind,shape", ((mx.DENSE, (4, 2, 2)), (mx.DENSE, (6, 3, 4)), (mx.REACH, 3), (mx.REACH, 8)))
def test_beta_zero_is_rollout_policy(torch_cuda, oracle, kind, shape):
    torch = torch_cuda
    S = _size((kind, shape))
    policy_logs = ("start", "act", "flags", "pos", "logits")
    for mc, mode in ((False, AUTORESET), (True, STRICT)):
        (blk, init, tgt), _, mlp, _ = mx.base_case(oracle, kind, shape, mc, mode)
        sel = "sample" if mx.MODES[mode][0] == pref.SAMPLE else "greedy"
        table = _table(kind, S, mc, blk, init, tgt)
        a, b, c = (_env(S, mc, blk, init, tgt, mode=mode) for _ in range(3))
        kw = dict(select=sel, epsilon=B["epsilon"], seed=B["seed"])
        plain = a.rollout_policy(B["steps"], _policy(torch, a, mlp), log=policy_logs, **kw)
        mixed = b.rollout_policy(B["steps"], _policy(torch, b, mlp), log=policy_logs + ("who",), expert=table, beta=0.0, **kw)
        labelled = c.rollout_policy(B["steps"], _policy(torch, c, mlp), log=ALL_LOGS, expert=table, beta=0.0, **kw)   # the table is read: the play is the same
        for other, env in ((mixed, b), (labelled, c)):
            for name in plain.FIELDS + ("logits_log", "start_pos"):
                assert torch.equal(getattr(plain, name), getattr(other, name)), (name, kind, mc, mode)
            for name in ("_pos", "_step_count", "_done", "_flags"):
                assert torch.equal(getattr(a, name), getattr(env, name)), (name, kind, mc, mode)
            assert int((other.who_log == 1).sum()) == 0 and int((other.who_log == 2).sum()) >= 300
        assert mixed.expert_log is None and int((labelled.expert_log != 255).sum()) >= 50
        # the raw call with no table at all: NULL pointers, n_rows of a table that is never read
        want = {k: getattr(plain, k).cpu().numpy() for k in pref.OUTPUTS}
        want.update(pos=a.positions.cpu().numpy(), step_count=a.step_count.cpu().numpy(), done=a.done.cpu().numpy().astype(np.uint8))
        want["who_log"] = mixed.who_log.cpu().numpy()
        st = _State(torch, a.device, S, mc, B["max_steps"], blk, init, tgt)
        ask = tuple(pref.OUTPUTS) + ("who_log",)
        got = _raw(torch, st, mlp, kind, None, B["steps"], mode, mx.MODES[mode][0], want, ask=ask, threshold=rref.threshold_of(B["epsilon"]), beta=0,
                   seed=B["seed"], n_rows=blk.shape[1])
        for k in ask:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k}: NULL table {(kind, mc, mode)}")
        _same_state(st, want, "NULL table")


# ---------------------------------------------------------------------------------------------------- 4. beta = 1
@pytest.mark.parametrize("kind,shape", ((mx.DENSE, (4, 2, 2)), (mx.DENSE, (4, 4, 2)), (mx.REACH, 4), (mx.REACH, 6)))
def test_beta_one_plays_the_table_rollouts_where_the_expert_always_has_a_move(torch_cuda, oracle, kind, shape):
    torch = torch_cuda
    S = _size((kind, shape))
    for mc in (False, True):
        (blk, init, tgt), _, mlp, _ = mx.base_case(oracle, kind, shape, mc, STRICT)
        table = _table(kind, S, mc, blk, init, tgt)
        a, b = _env(S, mc, blk, init, tgt), _env(S, mc, blk, init, tgt)
        K = B["steps"]
        mixed = a.rollout_policy(K, _policy(torch, a, mlp), select="greedy", epsilon=0.0, seed=B["seed"], log=("act", "flags", "pos", "expert", "who"),
                                 expert=table, beta=1.0)
        expert = b.rollout(K, "reach" if kind == mx.REACH else "table", table=table, epsilon=0.0, seed=B["seed"], log=("act", "flags", "pos"))
        flags, x = mixed.flags_log.cpu().numpy(), mixed.expert_log.cpu().numpy()
        done_on_entry = (flags & rref.FLAG_STEPPED_DONE) != 0
        first_done = np.where(done_on_entry.any(axis=0), done_on_entry.argmax(axis=0), K)
        before = np.arange(K)[:, None] < first_done[None, :]
        boards = np.flatnonzero(((x != 255) | ~before).all(axis=0) & (first_done > 0))
        assert boards.size >= 10, (kind, mc, boards.size)
        idx = torch.from_numpy(boards).to(a.device)
        assert torch.equal(mixed.pos_log[:, :, idx], expert.pos_log[:, :, idx]) and torch.equal(mixed.flags_log[:, idx], expert.flags_log[:, idx]), (kind, mc)
        assert (mixed.who_log.cpu().numpy()[before & (x != 255)] == 1).all() and int((mixed.who_log == 2).sum()) == 0
        assert int(mixed.wins[idx].sum()) >= 5


# ---------------------------------------------------------------------------------------------------- 5. Gaussian weights
SLACK, CAP = 2.0 ** -16, 1e-3


@pytest.mark.parametrize("select", ("greedy", "sample"))
@pytest.mark.parametrize("kind,shape,mc,H", ((mx.DENSE, (4, 4, 2), True, 64), (mx.REACH, 5, False, 16), (mx.REACH, 8, True, 29)))
def test_gaussian_weights_teacher_forced(torch_cuda, oracle, kind, shape, mc, H, select):
    """Every logged logit within the bound of the float64 logits of the board before its step; the yardstick, forced to select on
    the kernel's own logged logits, gives every log and the state byte for byte (SAMPLE: the boards that never come within 2**-16
    of a boundary of the float64 CDF, which leaves out at most 1 board-step in 1,000)."""
    torch = torch_cuda
    S = _size((kind, shape))
    sel = pref.GREEDY if select == "greedy" else pref.SAMPLE
    (blk, init, tgt), table, _, _ = mx.base_case(oracle, kind, shape, mc, AUTORESET)
    n, K = blk.shape[1], B["steps"]
    mlp = pref.random_mlp(np.random.default_rng(50 + H), mx.features(S, init.shape[0], tgt.shape[0], mc), H)
    env = _env(S, mc, blk, init, tgt, mode=AUTORESET)
    got = env.rollout_policy(K, _policy(torch, env, mlp), select=select, epsilon=B["epsilon"], seed=B["seed"], log=ALL_LOGS,
                             expert=_table(kind, S, mc, blk, init, tgt), beta=B["beta"])
    logits_log, pos_log = got.logits_log.cpu().numpy(), got.pos_log.cpu().numpy()
    b = oracle.OracleBatch(S, mc, B["max_steps"], blk, init, tgt)
    b.reset()
    near = np.zeros(n, bool)
    worst, left_out = 0.0, 0
    for k in range(K):
        b.pos[...] = init if k == 0 else pos_log[k - 1]
        z, bound = pref.board_logits(b, mlp)
        err = np.abs(logits_log[k].astype(np.float64) - z)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (k, float((err / bound).max()))
        if sel == pref.SAMPLE:
            close = pref.sample_margin(logits_log[k], rref.draws(n, B["seed"], k)) < SLACK
            left_out += int(close.sum())
            near |= close
    print(f"{kind} {shape} H={H} {select}: worst logit error / bound {worst:.3f}, left out near a CDF boundary {left_out / (n * K):.2e}")
    assert left_out <= CAP * n * K
    want = mx.rollout(oracle, kind, table, S, mc, B["max_steps"], blk, init, tgt, mlp, K, sel, AUTORESET, threshold=rref.threshold_of(B["epsilon"]),
                      beta=rref.threshold_of(B["beta"]), seed=B["seed"], exact32=False, force_logits=logits_log)
    keep = ~near
    for name in mx.OUTPUTS:
        if name != "logits_log":
            np.testing.assert_array_equal(getattr(got, name).cpu().numpy()[..., keep], want[name][..., keep], err_msg=name)
    np.testing.assert_array_equal(env.positions.cpu().numpy()[:, keep], want["pos"][:, keep])
    assert want["who"].min() >= 15 and len(np.unique(want["act_log"])) == 4


# ---------------------------------------------------------------------------------------------------- 6. advance
def test_advance_false_leaves_the_environment_untouched_and_true_equals_a_twin_stepped(torch_cuda, oracle):
    torch = torch_cuda
    for kind, shape, mc in ((mx.DENSE, (4, 2, 2), False), (mx.REACH, 5, True)):
        S = _size((kind, shape))
        (blk, init, tgt), _, mlp, _ = mx.base_case(oracle, kind, shape, mc, AUTORESET)
        table = _table(kind, S, mc, blk, init, tgt)
        for obs_dtype in ("float32", None):
            env, twin = (_env(S, mc, blk, init, tgt, mode=AUTORESET, obs_dtype=obs_dtype) for _ in range(2))
            policy = _policy(torch, env, mlp)
            before = (env.positions.clone(), env.step_count.clone(), env.done.clone(), env._flags.clone())
            free = env.rollout_policy(B["steps"], policy, select="greedy", epsilon=B["epsilon"], seed=B["seed"], log=("act", "flags"), expert=table,
                                      beta=B["beta"], advance=False)
            for x, y in zip(before, (env.positions, env.step_count, env.done, env._flags)):
                assert torch.equal(x, y)
            out = env.rollout_policy(B["steps"], policy, select="greedy", epsilon=B["epsilon"], seed=B["seed"], log=("act", "flags", "who"), expert=table,
                                     beta=B["beta"])
            assert torch.equal(out.act_log, free.act_log) and torch.equal(out.flags_log, free.flags_log) and torch.equal(out.wins, free.wins)
            for k in range(B["steps"]):
                obs, _, info = twin.step(out.act_log[k])
                assert torch.equal(out.flags_log[k], info["flags"]), k
            assert torch.equal(env.positions, twin.positions) and torch.equal(env.step_count, twin.step_count) and torch.equal(env.done, twin.done)
            assert torch.equal(env._flags, twin._flags) and out.flags is env._flags
            if obs_dtype is not None:
                assert torch.equal(env._obs, obs) and torch.equal(env._obs, env.encode())
            assert int((out.who_log == 1).sum()) >= 15


def test_the_errors_of_the_python_path(torch_cuda, oracle):
    torch = torch_cuda
    blk, init, tgt = oracle.generate_mt19937(4, 2, 2, 2, np.arange(8, dtype=np.uint32))
    env = _env(4, False, blk, init, tgt)
    mlp = mx.base_mlp(4, 2, 2, False, "int")
    policy = _policy(torch, env, mlp)
    dense, rtab = env.build_table(), env.build_reach_table()
    for table in (dense, rtab):
        assert env.rollout_policy(0, policy, expert=table).steps == 0
        for bad in (dict(beta=-0.1), dict(beta=1.5), dict(epsilon=2.0), dict(select="best"), dict(log=("values",)), dict(rows=torch.zeros(3, dtype=torch.int32))):
            with pytest.raises(ValueError):
                env.rollout_policy(3, policy, expert=table, **bad)
        with pytest.raises(TypeError):
            env.rollout_policy(3, object(), expert=table)
        other = _env(4, True, blk, init, tgt)
        with pytest.raises(ValueError, match="built for"):
            other.rollout_policy(3, _policy(torch, other, mx.base_mlp(4, 2, 2, True, "int")), expert=table)
        few = _env(4, False, blk[:, :4], init[:, :4], tgt[:, :4])
        with pytest.raises(ValueError, match="rows"):
            few.rollout_policy(3, policy, expert=table)
        out = few.rollout_policy(3, policy, expert=table, rows=[0, 1, 2, 3], log="expert")
        assert tuple(out.expert_log.shape) == (3, 4) and out.moves_log is None and out.who_log is None
    with pytest.raises(TypeError, match="DistanceTable"):
        env.rollout_policy(3, policy, expert="table")
    for name in ("expert", "moves", "best", "who"):
        with pytest.raises(ValueError):
            env.rollout_policy(3, policy, log=(name,))
    with pytest.raises(ValueError, match="expert"):
        env.rollout_policy(3, policy, beta=0.5)
    with pytest.raises(ValueError, match="expert"):
        env.rollout_policy(3, policy, rows=[0] * 8)
    plain = env.rollout_policy(3, policy, log=("act",), advance=False)
    assert plain.expert_log is None and plain.who_log is None and plain.act_log is not None


# ---------------------------------------------------------------------------------------------------- 7. raw calls, guarded memory
class _State:
    """A ts_state whose six rows lie between guard bytes."""

    ROWS = ("pos", "init", "tgt", "blk", "step_count", "done")

    def __init__(self, torch, dev, S, mc, max_steps, blk, init, tgt):
        from table_harness import GUARD, guarded
        from tiler_slider_amd import _cabi
        n = blk.shape[1]
        self.n, self.T = n, init.shape[0]
        self.host = dict(pos=np.ascontiguousarray(init, np.uint8), init=np.ascontiguousarray(init, np.uint8), tgt=np.ascontiguousarray(tgt, np.uint8),
                         blk=np.ascontiguousarray(blk, np.uint32), step_count=np.zeros(n, np.int32), done=np.zeros(n, np.uint8))
        self.bufs = {k: guarded(torch, dev, v) for k, v in self.host.items()}
        self.dims = _cabi.Dims(n, S, init.shape[0], tgt.shape[0], int(mc), max_steps, 0)
        self.state = _cabi.State(*(self.bufs[k].data_ptr() + GUARD for k in self.ROWS))

    def read(self):
        from table_harness import payload
        return {k: payload(self.bufs[k], v.dtype, v.shape) for k, v in self.host.items()}


def _same_state(st, want, ctx):
    now = st.read()
    for k in ("pos", "step_count", "done"):
        np.testing.assert_array_equal(now[k], np.asarray(want[k]).astype(now[k].dtype), err_msg=f"state {k}: {ctx}")
    for k in ("init", "tgt", "blk"):
        np.testing.assert_array_equal(now[k], st.host[k], err_msg=f"the level's {k} was written: {ctx}")


def _raw(torch, st, mlp, kind, table, steps, mode, select, want, ask=None, rows=None, threshold=0, beta=0, seed=0, n_rows=None, expect_name=True):
    """ts_mixed_rollout through the C-ABI on the guarded state `st`: {name: array} of the outputs asked for, each between guard
    bytes and prefilled with the bytewise complement of `want` (77s where it has none); an output not asked for is passed as NULL
    and must keep its fill.  table: a DistanceTable, a ReachTable, or None (NULL pointers)."""
    from table_harness import GUARD, guarded, payload
    from tiler_slider_amd import _mixed_cabi as mc_
    ask = mc_.OUT_FIELDS if ask is None else ask
    dev = st.bufs["pos"].device
    n, T = st.n, st.T
    shapes = {k: (n,) for k in mx.STATS}
    shapes.update({k: (steps, n) for k in LOG_NAMES}, pos_log=(steps, T, n), logits_log=(steps, n, 4))
    fills = {}
    for k in mc_.OUT_FIELDS:
        dt = mx.OUT_DTYPES[k]
        if want is None or k not in want:
            fills[k] = np.full(shapes[k], 77, dt)
        else:
            fills[k] = (~np.ascontiguousarray(want[k]).astype(dt).view(np.uint8)).view(dt).reshape(shapes[k])
    bufs = {k: guarded(torch, dev, fills[k]) for k in mc_.OUT_FIELDS}
    w1, b1, w2, b2 = mlp
    params = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (w1.T, b1, w2.T, b2)]
    net = mc_.Mlp(*(t.data_ptr() for t in params), w1.shape[0], 0)
    r = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(dev)
    cfg = mc_.MixedCfg(steps, mode, select, 1, seed, 0, 0, threshold, beta, kind, 0)
    cfg.slots = 2
    if table is not None:
        if kind == mx.REACH:
            cfg.table, cfg.slots, cfg.count, cfg.n_rows = table.table.data_ptr(), table.slots, table.count.data_ptr(), len(table)
        else:
            cfg.dense, cfg.n_rows = table.dist.data_ptr(), table.dist.shape[0]
    if n_rows is not None:
        cfg.n_rows = n_rows
    cfg.rows = None if r is None else r.data_ptr()
    if expect_name:
        d = mc_.describe_mixed_rollout(st.dims, w1.shape[0], cfg)
        assert d["name"] == f"k_mixed_rollout<{st.dims.size}, {select}, {kind}>" and d["blocks"] == -(-n // d["threads_per_block"])
    out = mc_.MixedOut(*(bufs[k].data_ptr() + GUARD if k in ask else None for k in mc_.OUT_FIELDS))
    s = torch.cuda.current_stream(dev)
    code = mc_.lib().ts_mixed_rollout(C.byref(st.dims), C.byref(st.state), C.byref(net), C.byref(cfg), C.byref(out), s.cuda_stream)
    assert code == 0, code
    s.synchronize()
    got = {k: payload(bufs[k], mx.OUT_DTYPES[k], shapes[k]) for k in mc_.OUT_FIELDS}
    for k in mc_.OUT_FIELDS:
        if k not in ask:
            np.testing.assert_array_equal(got[k].view(np.uint8), fills[k].view(np.uint8), err_msg=f"{k} was not asked for and was written")
    return {k: got[k] for k in ask}


@pytest.mark.parametrize("kind,shape,mc,mode", ((mx.DENSE, (4, 4, 2), False, STRICT), (mx.DENSE, (7, 2, 6), True, AUTORESET),
                                                (mx.REACH, 5, True, STRICT), (mx.REACH, 8, False, AUTORESET)))
def test_raw_calls_into_guarded_memory(torch_cuda, oracle, kind, shape, mc, mode):
    """165 boards (two full waves and a ragged third) replicate the 128 levels through rows=, some of them outside the table; every
    one of the fourteen outputs lies between guard bytes and is prefilled with the complement of the yardstick's answer."""
    torch = torch_cuda
    S = _size((kind, shape))
    (blk, init, tgt), ref, mlp, _ = mx.base_case(oracle, kind, shape, mc, mode)
    L, n = blk.shape[1], 165
    level = (np.arange(n) * 7 % L).astype(np.int32)
    rows = level.copy()
    rows[5::23] = np.resize(np.array([-1, L, 2**31 - 1, -2**31], np.int64), rows[5::23].size).astype(np.int32)
    big = [np.ascontiguousarray(a[:, level]) for a in (blk, init, tgt)]
    sel = mx.MODES[mode][0]
    kw = dict(threshold=rref.threshold_of(B["epsilon"]), beta=rref.threshold_of(B["beta"]), seed=B["seed"])
    want = mx.rollout(oracle, kind, ref, S, mc, B["max_steps"], *big, mlp, B["steps"], sel, mode, rows=rows, **kw)
    outside = (rows < 0) | (rows >= L)
    assert outside.sum() >= 5 and (want["expert_log"][:, outside] == 255).all() and want["who"][mx.WHO_EXPERT] >= 15
    table = _table(kind, S, mc, blk, init, tgt)
    st = _State(torch, torch.device("cuda", 0), S, mc, B["max_steps"], *big)
    got = _raw(torch, st, mlp, kind, table, B["steps"], mode, sel, want, rows=rows, **kw)
    for k in mx.OUTPUTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k}: {(kind, shape, mc, mode)}")
    _same_state(st, want, (kind, shape, mc, mode))
    # two outputs alone: the others are passed as NULL and keep their fill (checked inside)
    st = _State(torch, torch.device("cuda", 0), S, mc, B["max_steps"], *big)
    some = _raw(torch, st, mlp, kind, table, B["steps"], mode, sel, want, ask=("moves_log", "who_log"), rows=rows, **kw)
    np.testing.assert_array_equal(some["moves_log"], want["moves_log"])
    np.testing.assert_array_equal(some["who_log"], want["who_log"])


def test_reach_rows_of_arbitrary_bytes_end_the_call_and_give_no_move(torch_cuda, oracle):
    """Rows of 0xA5 bytes and rows of random bytes whose key bits are no placement of the shape, count claiming they are built: every
    probe walks its whole row, the launch ends, no board has an expert move - moves is 0 on a won board and TS_RTABLE_ABSENT
    elsewhere -, the network and the draw play what they play without a table, and nothing outside the buffers is written."""
    from tiler_slider_amd import ReachTable
    torch = torch_cuda
    S, mc, slots = 5, True, 128
    (blk, init, tgt), _, mlp, _ = mx.base_case(oracle, mx.REACH, S, mc, AUTORESET)
    n = 165
    level = (np.arange(n) * 7 % blk.shape[1]).astype(np.int32)
    big = [np.ascontiguousarray(a[:, level]) for a in (blk, init, tgt)]
    dev = torch.device("cuda", 0)
    kw = dict(threshold=rref.threshold_of(B["epsilon"]), seed=B["seed"])
    want = mx.rollout(oracle, mx.REACH, None, S, mc, B["max_steps"], *big, mlp, B["steps"], pref.GREEDY, AUTORESET, **kw)
    cells = [init[:, level]] + list(want["pos_log"][:-1])
    won = np.stack([oracle.OracleBatch(S, mc, 2**30, big[0], np.ascontiguousarray(c), big[2]).won() != 0 for c in cells])
    assert won.sum() >= 5
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 2**63, (n, slots), dtype=np.int64).view(np.uint64) | np.uint64(1 << 47)   # key bits 2^47 and up: no placement of 5x5 / 6
    for junk in (np.full((n, slots), 0xA5A5A5A5A5A5A5A5, np.uint64), noise):
        assert ((junk & np.uint64((1 << 48) - 1)) >= np.uint64((S * S) ** init.shape[0])).all() and (junk != 0).all()
        table = ReachTable(torch.from_numpy(junk.view(np.int64)).to(dev), torch.full((n,), 5, dtype=torch.int32, device=dev), None, None, 64, S, init.shape[0],
                           tgt.shape[0], mc, 252, "init")
        st = _State(torch, dev, S, mc, B["max_steps"], *big)
        got = _raw(torch, st, mlp, mx.REACH, table, B["steps"], AUTORESET, pref.GREEDY, want, beta=rref.threshold_of(B["beta"]), **kw)
        for k in pref.OUTPUTS + ("who_log",):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        _same_state(st, want, "junk rows")
        np.testing.assert_array_equal(got["moves_log"], np.where(won, 0, -4).astype(np.int16))
        assert (got["expert_log"] == 255).all() and (got["best_log"] == 0).all()


# ---------------------------------------------------------------------------------------------------- 8. every kernel at occupancy
@functools.lru_cache(maxsize=None)
def _occupancy_levels(orc, S, kind):
    """(mc, levels, the yardstick's table) of the occupancy case of size S: multi colour up to 4x4, single colour above (the planes
    of 262,141 boards stay small); dense: the base case's two-tile shape of that size, 1x1 with its one tile."""
    mc = S <= 4
    if kind == mx.REACH:
        return (mc,) + mx.reach_levels(orc, S, mc)
    if S == 1:
        import table_reference as tref
        n = B["levels"]
        blk, init, tgt = np.zeros((1, n), np.uint32), np.zeros((1, n), np.uint8), np.zeros((1, n), np.uint8)
        return mc, blk, init, tgt, tref.table(orc, 1, mc, blk, tgt, 1)
    shape = next(s for s in mx.DENSE_SHAPES if s[0] == S)
    return (mc,) + mx.dense_levels(orc, *shape, mc)


@pytest.mark.parametrize("name", sorted(mx.OCCUPANCY_CASES))
def test_every_compiled_mixed_kernel_at_occupancy(torch_cuda, oracle, name):
    """4,096 waves - 262,141 boards, the last wave ragged - that replicate the 128 levels through rows=, four steps."""
    from tiler_slider_amd import _mixed_cabi as mc_
    torch = torch_cuda
    S, sel, kind = mx.OCCUPANCY_CASES[name]
    mc, blk, init, tgt, ref = _occupancy_levels(oracle, S, kind)
    mode = AUTORESET if sel == pref.GREEDY else STRICT
    mlp = mx.base_mlp(S, init.shape[0], tgt.shape[0], mc, "int" if sel == pref.GREEDY else "int128")
    rows = (np.arange(mx.OCC_BOARDS) % blk.shape[1]).astype(np.int32)
    big = [np.ascontiguousarray(a[:, rows]) for a in (blk, init, tgt)]
    kw = dict(threshold=rref.threshold_of(B["epsilon"]), beta=rref.threshold_of(B["beta"]), seed=0x0CCE)
    want = mx.rollout(oracle, kind, ref, S, mc, 3, *big, mlp, mx.OCC_STEPS, sel, mode, rows=rows, **kw)
    assert S < 3 or (want["who"].min() >= 1000 and want["n_wins"] >= 100), (name, want["who"], want["n_wins"])
    table = _table(kind, S, mc, blk, init, tgt)
    st = _State(torch, torch.device("cuda", 0), S, mc, 3, *big)
    d = mc_.describe_mixed_rollout(st.dims, B["hidden"], mc_.MixedCfg(mx.OCC_STEPS, mode, sel, 1, 0, 0, 0, 0, 1, kind, 0, None, None, 2, None, 0, None))
    assert d["name"] == name and d["blocks"] * d["threads_per_block"] // 64 == mx.OCC_WAVES
    got = _raw(torch, st, mlp, kind, table, mx.OCC_STEPS, mode, sel, want, rows=rows, **kw)
    for k in mx.OUTPUTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k}: {name}")
    _same_state(st, want, name)


# ---------------------------------------------------------------------------------------------------- 9. streams
def test_a_mixed_rollout_on_a_stream_of_its_own_ordered_after_a_step(torch_cuda, oracle):
    """2**16 boards on a reach table, one extra stream, no host synchronisation until the end: the rollout is enqueued while the
    step still runs.  A launch that ignored its `stream` argument would play from cells the step has not written yet."""
    torch = torch_cuda
    kind, S, mc, n, K = mx.REACH, 5, True, 1 << 16, 12
    blk, init, tgt, ref = mx.reach_levels(oracle, S, mc)
    rows = (np.arange(n) % blk.shape[1]).astype(np.int32)
    big = [np.ascontiguousarray(a[:, rows]) for a in (blk, init, tgt)]
    mlp = mx.base_mlp(S, init.shape[0], tgt.shape[0], mc, "int")
    act = oracle.fill_actions(n, seed=0x57EA, step_index=0)
    twin = oracle.OracleBatch(S, mc, B["max_steps"], *big)
    twin.reset()
    twin.step(act, mode=AUTORESET, obs=False)
    kw = dict(rows=rows, threshold=rref.threshold_of(B["epsilon"]), beta=rref.threshold_of(B["beta"]), seed=8)
    want = mx.rollout(oracle, kind, ref, S, mc, B["max_steps"], *big, mlp, K, pref.GREEDY, AUTORESET, pos=twin.pos, step_count=twin.step_count,
                      done=twin.done, **kw)
    from_start = mx.rollout(oracle, kind, ref, S, mc, B["max_steps"], *big, mlp, K, pref.GREEDY, AUTORESET, **kw)
    assert (want["pos"] != from_start["pos"]).any(axis=0).sum() >= 1000      # the step matters
    table = _table(kind, S, mc, blk, init, tgt)
    env = _env(S, mc, *big, mode=AUTORESET)
    policy = _policy(torch, env, mlp)
    actions, r = torch.from_numpy(act).to(env.device), torch.from_numpy(rows).to(env.device)
    side = torch.cuda.Stream(device=env.device)
    assert side.cuda_stream != torch.cuda.current_stream(env.device).cuda_stream
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        env.step(actions)
        got = env.rollout_policy(K, policy, select="greedy", epsilon=B["epsilon"], seed=8, log=ALL_LOGS, expert=table, beta=B["beta"], rows=r)
    side.synchronize()
    _check(got, env, want, "stream")
