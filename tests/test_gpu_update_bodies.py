"""The two bodies of the in-place step's kernels on the GPU (csrc/ts_update.hip): boards that take the straight-line body and
boards that take the general body of the same kernels, and waves that do and do not load their initial cells - against ts_step
and the CPU oracle, byte for byte, every buffer of the in-place copy between guard bytes."""
import numpy as np
import pytest

import table_harness as th
import test_gpu_update as base
import update_cases as cases

pytestmark = pytest.mark.gpu

STEPS = 24
BATCHES = (1, 63, 64, 65, 257)  # a lone board, one lane either side of a wave, a second block of one board

# name: (S, T, Tt, obstacles, kernel stem, takes the straight-line body)
SHAPES = {
    "4x4_full": (4, 2, 2, 2, "k_step_update<4, 2, ", True),
    "4x4_T1_Tt2": (4, 1, 2, 2, "k_step_update<4, 2, ", False),
    "4x4_T2_Tt1": (4, 2, 1, 2, "k_step_update<4, 2, ", False),
    "4x4_T2_Tt0": (4, 2, 0, 2, "k_step_update<4, 2, ", False),
    "4x4_T8_Tt8": (4, 8, 8, 0, "k_step_update<4, 8, ", False),  # a full eight-tile kernel: it has the general body alone
    "4x4_T3_Tt3": (4, 3, 3, 2, "k_step_update<4, 8, ", False),
    "8x8_full": (8, 2, 2, 6, "k_step_update<8, 2, ", True),     # 64-bit masks
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch


def _drop_reward(raw):
    """The same copy without the reward output: ts_step and ts_step_update get a NULL pointer, the tensor keeps its sentinel."""
    from tiler_slider_amd import _cabi
    raw.out = _cabi.StepOut(raw.flags.data_ptr(), None if raw.u8 else raw.obs.data_ptr(), None, None, None,
                            raw.obs.data_ptr() if raw.u8 else None, None)


def _guards_hold(held, a, what):
    for f, (g, before) in held.items():
        try:
            now = th.payload(g, before.dtype, before.shape)  # asserts the guard bytes
        except AssertionError as e:
            raise AssertionError((what, f, str(e))) from None
        if f in ("init", "tgt", "blk"):
            assert np.array_equal(now, before), (what, f, "an input was written")
        else:
            assert np.array_equal(now, getattr(a, "pos" if f == "shown" else f).cpu().numpy()), (what, f)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_both_bodies_against_ts_step_and_the_oracle(torch_cuda, oracle, name):
    """Per shape: 1, 63, 64, 65 and 257 boards, both colour modes, strict and autoreset mode, float32 and uint8, 24 steps with
    max_steps 6 and a few bad action bytes.  After every step pos, step_count, done, flags, reward and the observation equal
    ts_step's and the oracle's and shown == pos; at the end no guard byte around any buffer has changed.  At 65 and 257 boards
    the runs are repeated without the reward output, whose tensor then keeps its sentinel."""
    torch = torch_cuda
    from tiler_slider_amd import _cabi, _update_cabi
    S, T, Tt, K, stem, full = SHAPES[name]
    for N in BATCHES:
        for mc in (True, False):
            lv = cases.make_levels(oracle, S, T, Tt, K, N, mc)
            for mode in (oracle.MODE_STRICT, oracle.MODE_AUTORESET):
                run = base._oracle_run(oracle, S, mc, 6, lv, mode, STEPS)
                for u8 in (False, True):
                    for reward in ((True, False) if N in (65, 257) else (True,)):
                        what = (name, N, mc, mode, u8, reward)
                        a = base._Raw(torch, S, T, Tt, mc, 6, *lv, u8)
                        b = base._Raw(torch, S, T, Tt, mc, 6, *lv, u8)
                        assert base._launches(b, stem + ("true>" if u8 else "false>")) and _update_cabi.full_body(b.dims) == full
                        b.show()
                        held = base._between_guards(torch, b)
                        want = base._upload(torch, run)
                        if not reward:
                            _drop_reward(a), _drop_reward(b)
                            for w in want:
                                w["reward"] = torch.full_like(w["reward"], 12345)
                        bad = base._compare_run(torch, a, b, want, mode)
                        assert not bad, (what, bad[:8])
                        _guards_hold(held, a, what)


def _reset_waves_run(torch, oracle, lone, mode, u8):
    """128 boards, two waves, max_steps 40 (no episode ends by itself in ten steps, and these levels see no win); step counters
    preset so that a step times out exactly the chosen boards: step 0 the one board `lone` of wave 0, step 5 all of wave 1 and
    none of wave 0.  pos is edited from outside between steps; every step is compared with ts_step and the oracle."""
    S, T, Tt, K, N, M = 4, 2, 2, 2, 128, 40
    lv = oracle.generate(S, T, Tt, K, N, seed=cases.LEVEL_SEED)
    ref = oracle.OracleBatch(S, True, M, *lv)
    ref.reset()
    a = base._Raw(torch, S, T, Tt, True, M, *lv, u8)
    b = base._Raw(torch, S, T, Tt, True, M, *lv, u8)
    b.show()
    held = base._between_guards(torch, b)
    what = (lone, mode, u8)

    def preset(boards):
        count = np.zeros(N, np.int32)
        count[boards] = M - 1
        ref.step_count[:] = count
        for raw in (a, b):
            raw.step_count.copy_(torch.from_numpy(count).cuda())

    def edit(k):
        """the cells of every third board rotate among its tiles: legal cells, tiles apart, shown left alone"""
        rolled = np.roll(ref.pos, 1, axis=0)
        ref.pos[:, k % 3::3] = rolled[:, k % 3::3]
        for raw in (a, b):
            raw.pos.copy_(torch.from_numpy(ref.pos).cuda())

    dones = []
    for k in range(10):
        if k == 0:
            preset([lone])
        if k == 5:
            preset(list(range(64, 128)))
        if k in (2, 3, 7):
            edit(k)
        act = oracle.fill_actions(N, seed=cases.ACTION_SEED, step_index=k)
        want = ref.step(act, mode=mode, reward=True)
        dones.append(ref.done.copy())
        dev = torch.from_numpy(act).cuda()
        a.step(dev, mode)
        b.step_update(dev, mode)
        for f, t in b.fields().items():
            assert torch.equal(t, a.fields()[f]), (what, k, f, "ts_step")
            w = ref.pos if f == "pos" else ref.step_count if f == "step_count" else ref.done if f == "done" else want[f]
            assert np.array_equal(t.cpu().numpy().astype(w.dtype), w), (what, k, f, "oracle")
        assert torch.equal(b.shown, b.pos), (what, k)
    _guards_hold(held, a, what)
    return dones


@pytest.mark.parametrize("lone", (0, 63))
def test_initial_cells_are_loaded_only_where_a_wave_resets(torch_cuda, oracle, lone):
    """The waves of the batch as the kernel meets them: after step 0 wave 0 holds exactly one done board (lane 0 in one run,
    lane 63 in the other) and wave 1 none - step 1 loads the initial cells in wave 0 alone; after step 5 wave 0 holds no done
    board and wave 1 holds 64 - step 6 loads them in wave 1 alone.  Strict and autoreset mode, float32 and uint8."""
    torch = torch_cuda
    for mode in (oracle.MODE_AUTORESET, oracle.MODE_STRICT):
        for u8 in (False, True):
            dones = _reset_waves_run(torch, oracle, lone, mode, u8)
            assert dones[0][lone] == 1 and dones[0].sum() == 1, "the oracle's run is not the one the test describes"
            assert dones[5][64:].sum() == 64 and dones[5][:64].sum() == (0 if mode == oracle.MODE_AUTORESET else 1)
            if mode == oracle.MODE_AUTORESET:
                assert dones[1].sum() == 0 and dones[6].sum() == 0  # each reset on the step after
