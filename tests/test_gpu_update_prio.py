"""The in-place step around its priority schedule (csrc/ts_update.hip: kLoadsFirst; profiles/update_requests.md, section 7) on
the GPU.  A wave's priority cannot change a value; what can go wrong is the code around the two `asm` statements - the loads,
the lazy initial cells of a resetting wave, the lanes past the batch - being scheduled differently.  So: raw calls into guarded
memory, exact against a ts_step twin and the CPU oracle field by field, shown == pos and no changed guard byte, on both bodies
of both observation types, an eight-tile kernel and the other written-through kernel, at a partial wave, a partial second wave
and a second block, in strict and in auto-reset mode with episodes of three steps, so that resetting waves load their initial
cells inside the raised region.  The helpers and the oracle's runs are those of tests/test_gpu_update.py and
tests/test_gpu_update_writeback.py."""
import pytest

from test_gpu_update import _Raw, _between_guards, _compare_run, _launches, _upload, torch_cuda  # noqa: F401 (fixture)
from test_gpu_update_quad import _check_guards
from test_gpu_update_writeback import MAX_STEPS, STEPS, _run

pytestmark = pytest.mark.gpu

assert (STEPS, MAX_STEPS) == (8, 3)
BATCHES = (1, 65, 257)
# id: (S, T, Tt, obstacles, uint8, kernel)
SHAPES = {
    "4x4_2_2_f32": (4, 2, 2, 2, False, "k_step_update<4, 2, false>"),  # the straight-line body
    "4x4_2_2_u8": (4, 2, 2, 2, True, "k_step_update<4, 2, true>"),
    "4x4_2_1_f32": (4, 2, 1, 2, False, "k_step_update<4, 2, false>"),  # the general body
    "4x4_3_3_f32": (4, 3, 3, 2, False, "k_step_update<4, 8, false>"),  # an eight-tile kernel
    "8x8_2_2_u8": (8, 2, 2, 6, True, "k_step_update<8, 2, true>"),     # the other kernel that writes through
}


@pytest.mark.parametrize("mode_name", ("strict", "autoreset"))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_field_is_exact_around_the_raised_region(torch_cuda, oracle, shape, mode_name):
    """1, 65 and 257 boards, eight steps with max_steps 3, multi colour.  After every step pos, step_count, done, flags, reward
    and the observation equal the ts_step twin's and the oracle's and shown == pos; after the last step no guard byte has
    changed and no input was written."""
    torch = torch_cuda
    S, T, Tt, K, u8, kernel = SHAPES[shape]
    mode = oracle.MODE_AUTORESET if mode_name == "autoreset" else oracle.MODE_STRICT
    for N in BATCHES:
        lv, run, _ = _run(oracle, S, T, Tt, K, N, mode)
        a = _Raw(torch, S, T, Tt, True, MAX_STEPS, *lv, u8)
        b = _Raw(torch, S, T, Tt, True, MAX_STEPS, *lv, u8)
        assert _launches(b, kernel), (shape, N)
        b.show()
        held = _between_guards(torch, b)
        assert all(f in run[0] for f in ("obs", "pos", "step_count", "done", "flags", "reward")), sorted(run[0])
        bad = _compare_run(torch, a, b, _upload(torch, run), mode)  # the six fields against both, and shown == pos, step by step
        assert not bad, (shape, N, mode_name, bad[:8])
        _check_guards(a, held, (shape, N, mode_name))
