"""The in-place step on the GPU (lib/libtiler_slider_update.so, include/tiler_slider_update.h): ts_step_update against ts_step and
the CPU oracle, byte for byte - no tolerances anywhere in this file.

Levels come from the oracle's twin of ts_generate with bench.py's LEVEL_SEED, actions from ts_fill_actions with its ACTION_SEED
(a few bytes above 3 patched in).  The oracle's trajectory of a case is computed once and shared by the float32 and the uint8
run."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVEL_SEED = 0x715311DE
ACTION_SEED = 0xAC710005
STEPS = 24
VOID = 0x10 | 0x20 | 0x40  # STEPPED_DONE | AUTORESET | BAD_ACTION: no transition was played

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
        self.state = _cabi.State(self.pos.data_ptr(), self.init.data_ptr(), self.tgt.data_ptr() if Tt else None, self.blk.data_ptr(),
                                 self.step_count.data_ptr(), self.done.data_ptr(), None)
        self.out = _cabi.StepOut(self.flags.data_ptr(), None if u8 else self.obs.data_ptr(), self.reward.data_ptr(), None, None,
                                 self.obs.data_ptr() if u8 else None, None)
        self.stream = torch.cuda.current_stream(dev).cuda_stream

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
