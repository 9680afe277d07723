"""The in-place step on the GPU (lib/libtiler_slider_update.so, include/tiler_slider_update.h): ts_step_update against ts_step and
the CPU oracle, byte for byte - no tolerances anywhere in this file.

Levels come from the oracle's twin of ts_generate with bench.py's LEVEL_SEED, actions from ts_fill_actions with its ACTION_SEED
(a few bytes above 3 patched in).  The oracle's trajectory of a case is computed once and shared by the float32 and the uint8
run."""
import ctypes as C

import numpy as np
import pytest

import table_harness as th
import update_cases as cases
from update_cases import ACTION_SEED, AUTORESET, LEVEL_SEED, SUCCESS, TIMEOUT, VOID

pytestmark = pytest.mark.gpu

STEPS = 24

# name: (S, T, Tt, obstacles, multi colour, max_steps, boards); ragged batches: 322 = 5 waves + 2 boards, 331 = 5 waves + 11
CASES = {
    "4x4_2_2": (4, 2, 2, 2, True, 6, 322),
    "3x3_1_0": (3, 1, 1, 0, True, 4, 331),
    "5x5_3_3_mc": (5, 3, 3, 3, True, 6, 322),
    "5x5_3_3_sc": (5, 3, 3, 3, False, 6, 331),
    "8x8_8_10": (8, 8, 8, 10, True, 9, 331),
    "1x1_1": (1, 1, 1, 0, False, 5, 322),
    "4x4_T3_Tt1": (4, 3, 1, 2, False, 6, 331),
    "4x4_dup_target": (4, 2, 2, 2, False, 6, 322),
}
# the cases whose run has to contain moves, autoresets and wins (autoreset mode).  The CPU oracle gives for these exact levels
# and the unpatched action stream over 24 steps: 4x4 / 2 / 2 (322 boards) 67 % moved, 978 autoresets, 22 wins; 3x3 / 1 / 0
# (331 boards) 64 % moved, 1,564 autoresets, 430 wins.  (5x5 / 3 / 3 and 8x8 / 8 / 10 show no win in 24 steps.)
HONEST = ("4x4_2_2", "3x3_1_0")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _levels(oracle, name):
    S, T, Tt, K, mc, max_steps, N = CASES[name]
    if S == 1:  # one cell: the tile stands on it, and so does the target - nothing to draw
        return np.zeros((1, N), np.uint32), np.zeros((T, N), np.uint8), np.zeros((Tt, N), np.uint8)
    blk, init, tgt = oracle.generate(S, T, Tt, K, N, seed=LEVEL_SEED)
    if name == "4x4_dup_target":
        tgt[1, ::2] = tgt[0, ::2]  # every other board: both targets on one cell
    return blk, init, tgt


def _actions(oracle, N, k):
    """Step k's actions of ts_fill_actions' stream (the oracle's twin; test_generated_actions pins the two to each other) with a
    few bytes above 3 patched in."""
    act = oracle.fill_actions(N, seed=ACTION_SEED, step_index=k)
    act[(7 * k + 3) % N] = 4 + k
    act[(11 * k + 100) % N] = 255
    return act


_TRAJECTORIES = {}


def _trajectory(oracle, name, mode):
    """The oracle's 24 steps of a case, once: per step the actions and everything a step writes."""
    key = (name, mode)
    if key not in _TRAJECTORIES:
        S, T, Tt, K, mc, max_steps, N = CASES[name]
        blk, init, tgt = _levels(oracle, name)
        ref = oracle.OracleBatch(S, mc, max_steps, blk, init, tgt)
        ref.reset()
        steps = []
        for k in range(STEPS):
            act = _actions(oracle, N, k)
            want = ref.step(act, mode=mode, reward=True)
            steps.append(dict(act=act, obs=want["obs"], flags=want["flags"], reward=want["reward"], pos=ref.pos.copy(),
                              step_count=ref.step_count.copy(), done=ref.done.copy()))
        _TRAJECTORIES[key] = steps
    return _TRAJECTORIES[key]


class _Raw:
    """One copy of a batch's state and outputs as device tensors, stepped through the C-ABI directly."""

    def __init__(self, torch, S, T, Tt, mc, max_steps, blk, init, tgt, u8, guard=0):
        from tiler_slider_amd import _cabi
        dev = torch.device("cuda", 0)
        self.torch, self.S, self.u8, self.N = torch, S, u8, blk.shape[1]
        self.blk = torch.from_numpy(blk.view(np.int32)).to(dev)
        self.init, self.tgt = torch.from_numpy(init).to(dev), torch.from_numpy(tgt).to(dev)
        self.pos = self.init.clone()
        self.step_count = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self.done = torch.zeros(self.N, dtype=torch.uint8, device=dev)
        self.flags = torch.full((self.N,), 0xEE, dtype=torch.uint8, device=dev)
        self.reward = torch.full((self.N,), 12345, dtype=torch.int32, device=dev)
        dtype = torch.uint8 if u8 else torch.float32
        self.guard = guard  # elements of sentinel on either side of the observation
        self.whole = torch.full((2 * guard + self.N * S * S * 3,), 99, dtype=dtype, device=dev)
        self.obs = self.whole[guard:guard + self.N * S * S * 3].view(self.N, S, S, 3)
        self.shown = torch.full_like(self.pos, 0xDD)
        self.dims = _cabi.Dims(self.N, S, T, Tt, int(mc), max_steps, 0)
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.bind()

    def bind(self):
        """The C structs of the tensors as they are now (again after a tensor was replaced: tensors held between guard bytes,
        an observation at an odd address)."""
        from tiler_slider_amd import _cabi
        self.state = _cabi.State(self.pos.data_ptr(), self.init.data_ptr(), self.tgt.data_ptr() if self.dims.n_targets else None,
                                 self.blk.data_ptr(), self.step_count.data_ptr(), self.done.data_ptr(), None)
        self.out = _cabi.StepOut(self.flags.data_ptr(), None if self.u8 else self.obs.data_ptr(), self.reward.data_ptr(), None, None,
                                 self.obs.data_ptr() if self.u8 else None, None)

    def encode(self, into=None):
        """ts_encode / ts_encode_u8 of the current cells into the observation (or `into`)."""
        from tiler_slider_amd import _cabi
        L = _cabi.lib()
        fn = L.ts_encode_u8 if self.u8 else L.ts_encode
        dst = self.obs if into is None else into
        assert fn(C.byref(self.dims), C.byref(self.state), dst.data_ptr(), self.stream) == 0
        return dst

    def show(self):
        """The contract of ts_step_update on entry: a full write, then shown = pos."""
        self.encode()
        self.shown.copy_(self.pos)

    def step(self, act, mode):
        from tiler_slider_amd import _cabi
        assert _cabi.lib().ts_step(C.byref(self.dims), C.byref(self.state), act.data_ptr(), mode, C.byref(self.out), self.stream) == 0

    def step_update(self, act, mode):
        from tiler_slider_amd import _update_cabi
        rc = _update_cabi.lib().ts_step_update(C.byref(self.dims), C.byref(self.state), act.data_ptr(), mode, C.byref(self.out),
                                               self.shown.data_ptr(), self.stream)
        assert rc == 0, rc

    def fields(self):
        return dict(pos=self.pos, step_count=self.step_count, done=self.done, flags=self.flags, reward=self.reward, obs=self.obs)


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_update_equals_ts_step_and_the_oracle(torch_cuda, oracle, name):
    """Two copies of the state, one stepped by ts_step and one by ts_step_update, both modes, float32 and uint8: after every
    one of 24 steps pos, step_count, done, flags, reward and the observation are equal to each other and to the oracle's, and
    shown == pos.  A run's verdicts are collected and reported together, first failures first."""
    torch = torch_cuda
    S, T, Tt, K, mc, max_steps, N = CASES[name]
    blk, init, tgt = _levels(oracle, name)
    names = ("pos", "step_count", "done", "flags", "reward", "obs")
    for mode in (oracle.MODE_STRICT, oracle.MODE_AUTORESET):
        traj = _trajectory(oracle, name, mode)
        want = [{f: torch.from_numpy(step[f]).cuda() for f in names + ("act",)} for step in traj]
        for u8 in (False, True):
            a = _Raw(torch, S, T, Tt, mc, max_steps, blk, init, tgt, u8)
            b = _Raw(torch, S, T, Tt, mc, max_steps, blk, init, tgt, u8)
            b.show()
            ok = np.zeros((STEPS, 2 * len(names) + 1), bool)
            flags = np.stack([step["flags"] for step in traj])
            moved, resets, wins = int(((flags & (VOID | 0x02)) == 0).sum()), int(((flags & 0x20) != 0).sum()), int(((flags & 0x04) != 0).sum())
            for k in range(STEPS):
                a.step(want[k]["act"], mode)
                b.step_update(want[k]["act"], mode)
                fa, fb = a.fields(), b.fields()
                for i, f in enumerate(names):
                    ok[k, 2 * i] = torch.equal(fa[f], fb[f])
                    w = want[k][f]
                    ok[k, 2 * i + 1] = torch.equal(fb[f], w.to(fb[f].dtype)) if f != "obs" else bool((fb[f].to(torch.float32) == w).all())
                ok[k, -1] = torch.equal(b.shown, b.pos)
            bad = np.argwhere(~ok).tolist()
            labels = [f"{f} vs {ref}" for f in names for ref in ("ts_step", "oracle")] + ["shown == pos"]
            assert not bad, (name, mode, "uint8" if u8 else "float32", [(k, labels[j]) for k, j in bad[:6]])
            print(f"{name} mode {mode} {'uint8' if u8 else 'float32'}: {moved / (STEPS * N):.2f} of the board-steps moved a tile, "
                  f"{resets} autoresets, {wins} wins")
            if mode == oracle.MODE_AUTORESET and name in HONEST:
                assert moved >= 0.25 * STEPS * N and resets >= 1 and wins >= 1, (name, moved, resets, wins)


def test_the_update_writes_only_the_cells_that_change(torch_cuda, oracle):
    """Sentinels in channels 0 and 2 and in guard elements on either side of the buffer survive the steps - so it was the
    in-place kernel that ran, and it wrote channel 1 alone - while channel 1 equals the full encoding after every step; a board
    whose tiles stand still has no byte of its channel 1 rewritten either (a sentinel in a cell no tile touches stays)."""
    torch = torch_cuda
    for name, u8 in (("4x4_2_2", False), ("5x5_3_3_sc", True), ("8x8_8_10", False)):
        S, T, Tt, K, mc, max_steps, N = CASES[name]
        blk, init, tgt = _levels(oracle, name)
        b = _Raw(torch, S, T, Tt, mc, max_steps, blk, init, tgt, u8, guard=4096)
        b.show()
        b.obs[..., 0] = 77
        b.obs[..., 2] = 55
        full = torch.empty_like(b.obs)
        for k in range(8):
            act = torch.from_numpy(_actions(oracle, N, k)).cuda()
            b.step_update(act, oracle.MODE_AUTORESET)
            b.encode(into=full)
            assert torch.equal(b.obs[..., 1], full[..., 1]), (name, k, "channel 1")
            assert bool((b.obs[..., 0] == 77).all()) and bool((b.obs[..., 2] == 55).all()), (name, k, "channels 0 and 2")
            assert bool((b.whole[:4096] == 99).all()) and bool((b.whole[-4096:] == 99).all()), (name, k, "guards")
        # a step that moves nothing (every action byte is bad) stores nothing: a sentinel on an empty cell of channel 1 stays
        empty = (full[..., 1] == 0).flatten(1).to(torch.uint8).argmax(dim=1)  # an empty cell of every board
        flat = b.obs.view(N, S * S, 3)
        flat[torch.arange(N, device="cuda"), empty, 1] = 33
        b.step_update(torch.full((N,), 9, dtype=torch.uint8, device="cuda"), oracle.MODE_STRICT)
        assert bool((flat[torch.arange(N, device="cuda"), empty, 1] == 33).all()), (name, "a standing board was rewritten")
        assert bool(((b.flags == 0x40) | (b.flags == 0x10)).all()) and bool((b.flags == 0x40).any())  # BAD_ACTION, or done: STEPPED_DONE


def test_state_edited_behind_the_kernels_back(torch_cuda, oracle):
    """pos is overwritten between two steps - with other legal cells, with ids >= S*S, with two tiles on one cell - and shown is
    left alone: the next step's observation is ts_encode of the new state, and everything equals ts_step from the same cells."""
    torch = torch_cuda
    for name, u8 in (("4x4_2_2", False), ("5x5_3_3_mc", True), ("5x5_3_3_sc", False), ("8x8_8_10", False)):
        S, T, Tt, K, mc, max_steps, N = CASES[name]
        blk, init, tgt = _levels(oracle, name)
        a = _Raw(torch, S, T, Tt, mc, max_steps, blk, init, tgt, u8)
        b = _Raw(torch, S, T, Tt, mc, max_steps, blk, init, tgt, u8)
        donor = _Raw(torch, S, T, Tt, mc, max_steps, blk, init, tgt, u8)  # legal cells of the same levels, a few steps on
        b.show()
        full = torch.empty_like(b.obs)
        for k in range(9):
            act = torch.from_numpy(_actions(oracle, N, 40 + k)).cuda()
            donor.step(torch.from_numpy(_actions(oracle, N, 80 + k)).cuda(), oracle.MODE_AUTORESET)
            edit = donor.pos.clone()
            if k % 3 == 1:
                edit[0, ::3] = 200           # ids >= S*S: clamped like everywhere else
                edit[T - 1, 1::5] = S * S
            elif k % 3 == 2 and T > 1:
                edit[1, ::2] = edit[0, ::2]  # two tiles on one cell: the higher index is drawn
                edit[T - 1, 1::4] = edit[0, 1::4]
            a.pos.copy_(edit)
            b.pos.copy_(edit)                # shown still holds the cells of the step before
            for mode in (oracle.MODE_AUTORESET, oracle.MODE_STRICT):
                a.step(act, mode)
                b.step_update(act, mode)
                b.encode(into=full)
                assert torch.equal(b.obs, full), (name, k, mode, "observation vs ts_encode of the new state")
                for f, t in a.fields().items():
                    assert torch.equal(t, b.fields()[f]), (name, k, mode, f)
                assert torch.equal(b.shown, b.pos), (name, k, mode, "shown")


def test_step_update_at_occupancy(torch_cuda, oracle):
    """262,144 4x4 boards - 4,096 waves, 16 per CU - 8 steps against ts_step."""
    torch = torch_cuda
    N = 262_144
    blk, init, tgt = oracle.generate(4, 2, 2, 2, N, seed=LEVEL_SEED)
    a = _Raw(torch, 4, 2, 2, True, 5, blk, init, tgt, False)
    b = _Raw(torch, 4, 2, 2, True, 5, blk, init, tgt, False)
    b.show()
    for k in range(8):
        act = torch.from_numpy(oracle.fill_actions(N, seed=ACTION_SEED, step_index=k)).cuda()
        a.step(act, oracle.MODE_AUTORESET)
        b.step_update(act, oracle.MODE_AUTORESET)
        for f, t in a.fields().items():
            assert torch.equal(t, b.fields()[f]), (k, f)
        assert torch.equal(b.shown, b.pos), k
    assert int(((a.flags & 0x20) != 0).sum()) > 0 or int(a.done.sum()) > 0


def test_environment_steps_in_place_by_default(torch_cuda, oracle):
    """The default environment of bench.py's cfg1 - 1,048,576 4x4 boards, 2 tiles, 2 obstacles, bench's seeds - reports the
    in-place kernel through describe_launch and equals an obs_update="full" twin over 50 steps with a reset() in the middle and
    cells edited from outside; smaller batches, batches whose observation does not fit the cache threshold, and environments
    with two observation buffers, with one-hot planes, with the legality mask or in host-mapped memory report the full-write
    path."""
    torch = torch_cuda
    from tiler_slider_amd import VecTilerSliderEnv, _cabi
    N = 1 << 20
    kw = dict(multi_color=True, max_steps=7, auto_reset=True)
    outs = _cabi.OUT_OBS | _cabi.OUT_FLAGS
    env = VecTilerSliderEnv.random(N, size=4, num_tiles=2, num_obstacles=2, seed=LEVEL_SEED, **kw)
    full = VecTilerSliderEnv.from_arrays(4, env._blk, env._init, env._tgt, obs_update="full", **kw)
    assert env.obs_update == "auto" and env._in_place and not full._in_place
    d = _cabi.describe_launch(env._dims, _cabi.OP_STEP, outs)
    assert d["name"] == "k_step_update<4, 2, false>" and d["kernel"] == 6 and d["blocks"] == N // 256
    assert _cabi.describe_launch(full._dims, _cabi.OP_STEP, outs)["name"] == "k_multi<4, 2, false, 2>"
    acts = []
    for k in range(16):
        a = torch.empty(N, dtype=torch.uint8, device="cuda")
        _cabi.check(_cabi.lib().ts_fill_actions(N, ACTION_SEED, 0, k, a.data_ptr(), torch.cuda.current_stream().cuda_stream), "ts_fill_actions")
        a[(7 * k + 3)::9973] = 4 + k  # a few bad action bytes
        acts.append(a)
    assert torch.equal(env.reset(), full.reset())
    for k in range(50):
        if k == 25:
            assert torch.equal(env.reset(), full.reset())
        if k == 33:  # env.positions is the live tensor: a caller moves tiles by hand
            edit = env.positions.roll(1, dims=0).clone()
            env.positions.copy_(edit)
            full.positions.copy_(edit)
        obs, done, info = env.step(acts[k & 15])
        fobs, fdone, finfo = full.step(acts[k & 15])
        assert torch.equal(obs, fobs), (k, "obs")
        assert torch.equal(done, fdone) and torch.equal(info["flags"], finfo["flags"]) and torch.equal(env.positions, full.positions), k
        assert torch.equal(env.step_count, full.step_count), k
    assert obs.data_ptr() == env._obs.data_ptr()  # the environment's own buffer, every time
    assert int(((info["flags"] & 0x20) != 0).sum()) > 0 and torch.equal(env._shown, env.positions)
    del env, full, obs, fobs
    # who keeps the full-write path: small batches first
    blk, init, tgt = oracle.generate(4, 2, 2, 2, 4099, seed=LEVEL_SEED)
    small = VecTilerSliderEnv.from_arrays(4, blk, init, tgt, **kw)
    assert not small._in_place and _cabi.describe_launch(small._dims, _cabi.OP_STEP, outs)["name"].startswith("k_small<")
    few = [np.ascontiguousarray(x[:, :64]) for x in (blk, init, tgt)]
    for extra in (dict(obs_buffers=2), dict(with_onehot=True), dict(with_valid_moves=True), dict(host_mapped=True), dict(obs_dtype=None)):
        other = VecTilerSliderEnv.from_arrays(4, *few, **kw, **extra)
        assert not other._in_place and other._shown is None, extra
        with pytest.raises(ValueError):
            VecTilerSliderEnv.from_arrays(4, *few, obs_update="inplace", **kw, **extra)
    with pytest.raises(ValueError):
        VecTilerSliderEnv.from_arrays(9, *oracle.generate(9, 2, 2, 2, 64, seed=1), obs_update="inplace", **kw)
    with pytest.raises(ValueError):
        VecTilerSliderEnv.from_arrays(4, blk, init, tgt, obs_update="sometimes", **kw)
    # the domain of "auto" (the rows of profiles/update_ab.log): inside the cache threshold the full-write kernels switch their
    # forms by from 786,432 boards on; beyond it where a board has at least 170 bytes of observation per tile
    pays, L = VecTilerSliderEnv.in_place_pays, _cabi.lib()
    assert pays(192 << 20, 1 << 20, 2) and pays(144 << 20, 3 << 18, 2) and pays(48 << 20, 1 << 20, 8)
    assert not pays(96 << 20, 1 << 19, 2) and not pays(48 << 20, 1 << 18, 2) and not pays(12 << 20, 65536, 2) and not pays(0, 0, 2)
    assert not pays(768 << 20, 4 << 20, 2) and not pays(3072 << 20, 16 << 20, 2) and not pays(300 << 20, 1 << 20, 2)
    assert pays(384 << 20, 1 << 19, 4) and not pays(384 << 20, 1 << 19, 5) and not pays(288 << 20, 393216, 4)
    before = L.ts_tuning(_cabi.TUNE_NT_THRESHOLD_BYTES, (192 << 20) - 1)
    try:
        assert not pays(192 << 20, 1 << 20, 2)
        L.ts_tuning(_cabi.TUNE_NT_THRESHOLD_BYTES, 0)
        assert not pays(48 << 20, 1 << 20, 2) and not pays(201326592, 262144, 4)  # 8x8, forced beyond the cache, 262,144 boards
    finally:
        L.ts_tuning(_cabi.TUNE_NT_THRESHOLD_BYTES, before)


def test_forced_in_place_environment_and_captured_graphs(torch_cuda, oracle):
    """obs_update="inplace" on a small ragged batch, float32 and uint8 with reward, against a full-write twin: a captured graph of
    four steps, replayed twice, equals eager steps; an environment that was never reset makes its full write before it
    captures, so an eager step before the first replay is right too; a rollout that advances the boards leaves an observation the next step can update."""
    torch = torch_cuda
    from tiler_slider_amd import VecTilerSliderEnv, _cabi
    N = 4099
    blk, init, tgt = oracle.generate(4, 2, 2, 2, N, seed=LEVEL_SEED)
    acts = [torch.from_numpy(_actions(oracle, N, k)).cuda() for k in range(8)]
    for dtype in ("float32", "uint8"):
        kw = dict(multi_color=True, max_steps=7, auto_reset=True, obs_dtype=dtype, with_reward=dtype == "uint8")
        env = VecTilerSliderEnv.from_arrays(4, blk, init, tgt, obs_update="inplace", **kw)
        full = VecTilerSliderEnv.from_arrays(4, blk, init, tgt, obs_update="full", **kw)
        outputs = (_cabi.OUT_OBS if dtype == "float32" else _cabi.OUT_OBS_U8 | _cabi.OUT_REWARD)
        assert _cabi.describe_launch(env._dims, _cabi.OP_STEP, outputs)["name"] == f"k_step_update<4, 2, {'false' if dtype == 'float32' else 'true'}>"
        assert torch.equal(env.reset(), full.reset())
        graph = env.capture_steps(acts[:4])
        for rep in range(2):
            graph.replay()
            for k in range(4):
                full.step_async(acts[k])
            torch.cuda.synchronize()
            assert torch.equal(env._obs, full._obs) and torch.equal(env._flags, full._flags) and torch.equal(env.positions, full.positions), (dtype, rep)
            assert torch.equal(env._shown, env.positions)
        env.rollout(3, "random", seed=5)
        full.rollout(3, "random", seed=5)
        for k in range(4, 8):
            obs, _, _ = env.step(acts[k])
            fobs, _, _ = full.step(acts[k])
            assert torch.equal(obs, fobs) and torch.equal(env.positions, full.positions), (dtype, k, "after a rollout")
        fresh = VecTilerSliderEnv.from_arrays(4, blk, init, tgt, obs_update="inplace", **kw)
        twin = VecTilerSliderEnv.from_arrays(4, blk, init, tgt, obs_update="full", **kw)
        graph = fresh.capture_steps(acts[:2])
        fresh.step_async(acts[2]), twin.step_async(acts[2])  # eager, before the first replay
        graph.replay()
        twin.step_async(acts[0]), twin.step_async(acts[1])
        torch.cuda.synchronize()
        assert torch.equal(fresh._obs, twin._obs) and torch.equal(fresh.positions, twin.positions), dtype


# ---- every compiled kernel (tests/update_cases.py: one entry per kernel of the code object) ----
_FIELDS = ("pos", "step_count", "done", "flags", "reward", "obs")
_LABELS = [f"{f} vs {ref}" for f in _FIELDS for ref in ("ts_step", "oracle")] + ["shown == pos"]


def _oracle_run(oracle, S, mc, max_steps, lv, mode, steps, obs=True):
    """`steps` steps of the oracle on the levels `lv` under _actions' stream (unpatched below 63 boards, where the two bad
    bytes a step would be most of the batch): per step the actions and everything a step writes."""
    ref = oracle.OracleBatch(S, mc, max_steps, *lv)
    ref.reset()
    out = []
    for k in range(steps):
        act = _actions(oracle, ref.n, k) if ref.n >= 63 else oracle.fill_actions(ref.n, seed=ACTION_SEED, step_index=k)
        want = ref.step(act, mode=mode, reward=True, obs=obs)
        row = dict(act=act, flags=want["flags"], reward=want["reward"], pos=ref.pos.copy(), step_count=ref.step_count.copy(), done=ref.done.copy())
        if obs:
            row["obs"] = want["obs"]
        out.append(row)
    return out


def _upload(torch, run):
    return [{f: torch.from_numpy(v).cuda() for f, v in row.items()} for row in run]


def _compare_run(torch, a, b, want, mode):
    """Steps `a` through ts_step and `b` through ts_step_update over the oracle's run `want` (device tensors).  After every step
    the six fields of b against a's and against the oracle's (where the run holds them), and shown == pos; the verdicts stay on
    the device until the run is over.  Returns the failures as (step, what), first step first."""
    rows = []
    yes = torch.ones((), dtype=torch.bool, device="cuda")
    for w in want:
        a.step(w["act"], mode)
        b.step_update(w["act"], mode)
        fa, fb = a.fields(), b.fields()
        row = []
        for f in _FIELDS:
            row.append((fa[f] == fb[f]).all())
            row.append((fb[f] == w[f]).all() if f in w else yes)
        row.append((b.shown == b.pos).all())
        rows.append(torch.stack(row))
    ok = torch.stack(rows).cpu().numpy()
    return [(k, _LABELS[j]) for k, j in np.argwhere(~ok).tolist()]


def _launches(raw, name):
    """The kernel ts_step_update launches for this copy's dims and outputs is the case's."""
    from tiler_slider_amd import _cabi, _update_cabi
    outputs = (_cabi.OUT_OBS_U8 if raw.u8 else _cabi.OUT_OBS) | _cabi.OUT_REWARD
    return _update_cabi.describe_step_update(raw.dims, outputs)["name"] == name


_CASE_RUNS = {}  # of the shape run last, as _OCC_RUN below


def _case_run(oracle, name, mc, mode):
    """Levels and the oracle's 24 steps of a case's shape in a ragged batch of 331, once for both observation types."""
    key = (cases.shape_key(name), mc, mode)
    if key not in _CASE_RUNS:
        if any(k[0] != key[0] for k in _CASE_RUNS):
            _CASE_RUNS.clear()
        lv = cases.levels(oracle, name, 331, mc)
        _CASE_RUNS[key] = (lv, _oracle_run(oracle, cases.CASES[name][0], mc, 6, lv, mode, STEPS))
    return _CASE_RUNS[key]


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_every_update_kernel_in_a_ragged_batch(torch_cuda, oracle, name):
    """One case per kernel of the code object (tests/update_cases.py; tests/test_update_cpu.py pins the table to it): 331
    boards - five waves and eleven lanes - both colour modes, both step modes, 24 steps with max_steps 6 and a few bad action
    bytes.  After every step pos, step_count, done, flags, reward and the observation equal ts_step's and the oracle's, and
    shown == pos.  The oracle's flags of the autoreset runs keep the table's floors: tiles move, boards win, time out and are
    reset."""
    torch = torch_cuda
    S, T, Tt, K = cases.CASES[name]
    u8 = cases.is_u8(name)
    failures = []
    for mc in (True, False):
        for mode in (oracle.MODE_STRICT, oracle.MODE_AUTORESET):
            lv, run = _case_run(oracle, name, mc, mode)
            a = _Raw(torch, S, T, Tt, mc, 6, *lv, u8)
            b = _Raw(torch, S, T, Tt, mc, 6, *lv, u8)
            assert _launches(b, name) and (Tt > 0 or b.state.tgt is None)
            b.show()
            bad = _compare_run(torch, a, b, _upload(torch, run), mode)
            failures += [("multi" if mc else "single", "autoreset" if mode else "strict") + x for x in bad[:6]]
            flags = np.stack([row["flags"] for row in run])
            print(f"{name} {'multi' if mc else 'single'} colour, mode {mode}: moved {cases.stats(flags)[0]:.2f}, wins / autoresets / timeouts {cases.stats(flags)[1:]}")
            if mode == oracle.MODE_AUTORESET:
                cases.assert_floors(name, mc, flags)
    assert not failures, (name, failures)


OCC_BOARDS, OCC_STEPS = 262_144, 8
_OCC_RUN = {}  # the shape run last: a kernel's two observation types follow each other in sorted(CASES)


def _occupancy_run(oracle, name):
    key = cases.shape_key(name)
    if key not in _OCC_RUN:
        _OCC_RUN.clear()
        S = key[0]
        lv = cases.levels(oracle, name, OCC_BOARDS, S % 2 == 0)
        _OCC_RUN[key] = (lv, _oracle_run(oracle, S, S % 2 == 0, 5, lv, oracle.MODE_AUTORESET, OCC_STEPS, obs=False))
    return _OCC_RUN[key]


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_every_update_kernel_at_occupancy(torch_cuda, oracle, name):
    """The same table at 262,144 distinct boards - 4,096 waves, 16 per CU: multi colour on even sizes, single colour on odd
    ones, autoreset mode, max_steps 5, 8 steps.  After every step all six fields equal a ts_step twin's and shown == pos; pos,
    step_count, done, flags and reward equal the oracle's; after the last step the observation is ts_encode of the final state.
    By the oracle's flags the run holds autoresets, and wins exactly where the counts allow them."""
    torch = torch_cuda
    S, T, Tt, K = cases.CASES[name]
    u8, mc = cases.is_u8(name), S % 2 == 0
    lv, run = _occupancy_run(oracle, name)
    a = _Raw(torch, S, T, Tt, mc, 5, *lv, u8)
    b = _Raw(torch, S, T, Tt, mc, 5, *lv, u8)
    assert _launches(b, name) and b.N == OCC_BOARDS
    b.show()
    bad = _compare_run(torch, a, b, _upload(torch, run), oracle.MODE_AUTORESET)
    assert not bad, (name, bad[:8])
    full = torch.empty_like(b.obs)
    b.encode(into=full)
    assert torch.equal(b.obs, full), (name, "the observation against ts_encode of the final state")
    moved, wins, resets, timeouts = cases.stats(np.stack([row["flags"] for row in run]))
    print(f"{name}: moved {moved:.2f}, {wins} wins, {resets} autoresets, {timeouts} timeouts")
    assert resets >= OCC_BOARDS and (timeouts > 0 or not cases.can_move(name)), (name, resets, timeouts)  # step 5 times out, step 6 resets
    expected = cases.wins_expected(name, mc)
    assert expected is None or (wins >= 1000 if expected else wins == 0), (name, wins)
    assert (moved >= 0.2) if cases.can_move(name) else moved == 0, (name, moved)


def _between_guards(torch, raw):
    """Every buffer of `raw` that ts_step_update reads or writes moves into an allocation of its own between table_harness's
    guard bytes.  Returns {field: (guarded buffer, the payload's bytes as they are now)}."""
    held = {}
    for f in ("pos", "shown", "step_count", "done", "flags", "reward", "obs", "init", "tgt", "blk"):
        t = getattr(raw, f)
        if t.numel() == 0:
            continue
        before = t.cpu().numpy()
        g = th.guarded(torch, t.device, before)
        setattr(raw, f, g[th.GUARD:g.numel() - th.GUARD].view(t.dtype).view(t.shape))
        held[f] = (g, before)
    raw.whole = held["obs"][0]
    raw.bind()
    return held


def _edge_batches(torch, oracle):
    """N = 1 (63 lanes play a copy of the only board and must write nothing), one lane either side of a wave, one lane either
    side of a block (257: the second block's last three waves leave at the wave-uniform return), on a 32-bit and on a partly
    filled 64-bit mask: against ts_step and the oracle, every buffer of the in-place copy between guard bytes.  The guard is
    256 bytes: a stray observation store of the first lane past the batch lands in it at 4x4 (a board is 192 bytes of float32)
    and at 7x7 in uint8 (147 bytes), not at 7x7 in float32 (588 bytes) - there the state buffers' guards are what bites."""
    for stem in ("k_step_update<4, 2, ", "k_step_update<7, 8, "):
        for N in (1, 63, 64, 65, 255, 256, 257):
            for mc in (True, False):
                lv = cases.levels(oracle, stem + "false>", N, mc)
                S, T, Tt, K = cases.CASES[stem + "false>"]
                for mode in (oracle.MODE_AUTORESET, oracle.MODE_STRICT):
                    run = _oracle_run(oracle, S, mc, 6, lv, mode, 12)
                    for u8 in (False, True):
                        what = (stem, N, mc, mode, u8)
                        a = _Raw(torch, S, T, Tt, mc, 6, *lv, u8)
                        b = _Raw(torch, S, T, Tt, mc, 6, *lv, u8)
                        assert _launches(b, stem + ("true>" if u8 else "false>"))
                        b.show()
                        held = _between_guards(torch, b)
                        want = _upload(torch, run)
                        acts = [th.guarded(torch, b.pos.device, row["act"]) for row in run]
                        for w, g in zip(want, acts):
                            w["act"] = g[th.GUARD:th.GUARD + N]
                        bad = _compare_run(torch, a, b, want, mode)
                        assert not bad, (what, bad[:8])
                        for f, (g, before) in held.items():
                            try:
                                now = th.payload(g, before.dtype, before.shape)  # asserts the guard bytes
                            except AssertionError as e:
                                raise AssertionError((what, f, str(e))) from None
                            if f in ("init", "tgt", "blk"):
                                assert np.array_equal(now, before), (what, f, "an input was written")
                            else:
                                assert np.array_equal(now, getattr(a, "pos" if f == "shown" else f).cpu().numpy()), (what, f)
                        for row, g in zip(run, acts):
                            try:
                                assert np.array_equal(th.payload(g, np.uint8, (N,)), row["act"]), "actions were written"
                            except AssertionError as e:
                                raise AssertionError((what, "actions", str(e))) from None


def _edge_odd_address(torch, oracle):
    """The header asks no alignment of a uint8 observation: the in-place copy's starts 1 and 3 bytes into its allocation (the
    ts_step twin and ts_encode_u8 keep aligned ones).  Contents equal the twin's after every step; no byte outside the view
    changes."""
    N = 331
    for name in ("k_step_update<5, 8, true>", "k_step_update<6, 8, true>"):
        S, T, Tt, K = cases.CASES[name]
        mc = S % 2 == 0
        lv = cases.levels(oracle, name, N, mc)
        want = _upload(torch, _oracle_run(oracle, S, mc, 6, lv, oracle.MODE_AUTORESET, 8))
        for off in (1, 3):
            a = _Raw(torch, S, T, Tt, mc, 6, *lv, True)
            b = _Raw(torch, S, T, Tt, mc, 6, *lv, True)
            n = b.obs.numel()
            b.whole = torch.full((n + 8,), 99, dtype=torch.uint8, device="cuda")
            b.obs = b.whole[off:off + n].view(N, S, S, 3)
            b.bind()
            assert b.obs.data_ptr() % 4 == off and a.obs.data_ptr() % 4 == 0 and _launches(b, name)
            b.obs.copy_(a.encode())  # the contract on entry: the full encoding, written by other means
            b.shown.copy_(b.pos)
            bad = _compare_run(torch, a, b, want, oracle.MODE_AUTORESET)
            assert not bad, (name, off, bad[:8])
            full = torch.empty_like(a.obs)
            b.encode(into=full)
            assert torch.equal(b.obs, full), (name, off, "ts_encode_u8 of the final state")
            assert bool((b.whole[:off] == 99).all()) and bool((b.whole[off + n:] == 99).all()), (name, off, "bytes around the view")


def _edge_max_steps_1(torch, oracle):
    """max_steps = 1: every played step times out, in autoreset mode every other step is the reset.  On the one-cell board the
    same step carries IS_WON | SUCCESS | TIMEOUT; 6x6 with two tiles."""
    N = 331
    for stem in ("k_step_update<1, 2, ", "k_step_update<6, 2, "):
        S, T, Tt, K = cases.CASES[stem + "false>"]
        for mc in (True, False):
            lv = cases.levels(oracle, stem + "false>", N, mc)
            for mode in (oracle.MODE_AUTORESET, oracle.MODE_STRICT):
                run = _oracle_run(oracle, S, mc, 1, lv, mode, 8)
                flags = np.stack([row["flags"] for row in run])
                played = (flags & VOID) == 0
                assert ((flags[played] & TIMEOUT) != 0).all() and played[0].sum() >= N - 2
                if mode == oracle.MODE_AUTORESET:
                    assert int(((flags & AUTORESET) != 0).sum()) >= 4 * (N - 8) and int(played.sum()) >= 4 * (N - 8)
                if S == 1:
                    won_in_time = cases.IS_WON | SUCCESS | TIMEOUT
                    assert ((flags[played] & won_in_time) == won_in_time).all()
                for u8 in (False, True):
                    a = _Raw(torch, S, T, Tt, mc, 1, *lv, u8)
                    b = _Raw(torch, S, T, Tt, mc, 1, *lv, u8)
                    assert _launches(b, stem + ("true>" if u8 else "false>"))
                    b.show()
                    bad = _compare_run(torch, a, b, _upload(torch, run), mode)
                    assert not bad, (stem, mc, mode, u8, bad[:8])


@pytest.mark.parametrize("edge", ("batches", "odd_address", "max_steps_1"))
def test_edges_of_the_launch_and_the_buffers(torch_cuda, oracle, edge):
    """Small and boundary batches with every buffer between guard bytes; a uint8 observation at an odd address; max_steps 1."""
    {"batches": _edge_batches, "odd_address": _edge_odd_address, "max_steps_1": _edge_max_steps_1}[edge](torch_cuda, oracle)


def test_forced_in_place_environment_on_a_64_bit_mask(torch_cuda, oracle):
    """obs_update="inplace" on 7x7 boards (49 of the mask's 64 bits) with 3 tiles and 5 obstacles, 4,099 boards of the case
    table's winnable construction, float32 single colour and uint8 multi colour with reward, against an obs_update="full" twin:
    reset(), a captured graph of four steps replayed twice, rollout(3, "random"), four eager steps - observation, flags,
    positions and step_count equal throughout, boards win on the way, and at the end _shown == positions."""
    torch = torch_cuda
    from tiler_slider_amd import VecTilerSliderEnv, _cabi
    N = 4099
    acts = [torch.from_numpy(_actions(oracle, N, k)).cuda() for k in range(8)]
    for dtype, mc in (("float32", False), ("uint8", True)):
        blk, init, tgt = cases.make_levels(oracle, 7, 3, 3, 5, N, mc)
        kw = dict(multi_color=mc, max_steps=7, auto_reset=True, obs_dtype=dtype, with_reward=dtype == "uint8")
        env = VecTilerSliderEnv.from_arrays(7, blk, init, tgt, obs_update="inplace", **kw)
        full = VecTilerSliderEnv.from_arrays(7, blk, init, tgt, obs_update="full", **kw)
        outputs = (_cabi.OUT_OBS if dtype == "float32" else _cabi.OUT_OBS_U8 | _cabi.OUT_REWARD)
        assert env._in_place and not full._in_place
        assert _cabi.describe_launch(env._dims, _cabi.OP_STEP, outputs)["name"] == f"k_step_update<7, 8, {'false' if dtype == 'float32' else 'true'}>"

        def same(what):
            assert torch.equal(env._obs, full._obs), (dtype, what, "obs")
            assert torch.equal(env._flags, full._flags), (dtype, what, "flags")
            assert torch.equal(env.positions, full.positions) and torch.equal(env.step_count, full.step_count), (dtype, what, "state")
            if dtype == "uint8":
                assert torch.equal(env._reward, full._reward), (dtype, what, "reward")

        assert torch.equal(env.reset(), full.reset())
        wins = 0
        graph = env.capture_steps(acts[:4])
        for rep in range(2):
            graph.replay()
            for k in range(4):
                full.step_async(acts[k])
                wins += int(((full._flags & SUCCESS) != 0).sum())
            torch.cuda.synchronize()
            same(("replay", rep))
            assert torch.equal(env._shown, env.positions)
        env.rollout(3, "random", seed=5)
        full.rollout(3, "random", seed=5)
        same("rollout")  # the rollout re-encodes the observation, rebinds the flags and re-synchronises _shown
        assert torch.equal(env._shown, env.positions), (dtype, "rollout", "shown")
        for k in range(4, 8):
            obs, done, info = env.step(acts[k])
            fobs, fdone, finfo = full.step(acts[k])
            assert torch.equal(obs, fobs) and torch.equal(done, fdone) and torch.equal(info["flags"], finfo["flags"]), (dtype, k)
            same(("eager", k))
            wins += int(((finfo["flags"] & SUCCESS) != 0).sum())
        assert wins >= 100, (dtype, wins)  # half the boards win one step in four
        assert torch.equal(env._shown, env.positions)
