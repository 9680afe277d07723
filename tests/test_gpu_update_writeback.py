"""The in-place step's stores after the write-back study (csrc/ts_update.hip; profiles/update_requests.md, section 6) on the GPU:
raw calls into guarded memory, exact against a ts_step twin and the CPU oracle field by field, shown == pos, and sentinels where
the kernel must not write - channels 0 and 2 of every cell and a channel-1 cell no tile comes near.  The study shipped a flavour
and no block-dependent rule - <4, 2, false> and <8, 2, true> write the observation through the L2, every block alike - so the
sizes are those at which a store's flavour or its issuing lane could matter: one board, either side of a wave, either side of
a block.  The helpers are those of tests/test_gpu_update.py."""
import numpy as np
import pytest

import update_cases as cases
from test_gpu_update import _Raw, _between_guards, _launches, _oracle_run, torch_cuda  # noqa: F401 (fixture)
from test_gpu_update_quad import _check_guards

pytestmark = pytest.mark.gpu

STEPS = 8
MAX_STEPS = 3
BATCHES = (1, 63, 64, 65, 255, 256, 257)
# id: (S, T, Tt, obstacles, uint8, kernel)
SHAPES = {
    "4x4_2_2_f32": (4, 2, 2, 2, False, "k_step_update<4, 2, false>"),  # two targets: the straight-line body
    "4x4_2_2_u8": (4, 2, 2, 2, True, "k_step_update<4, 2, true>"),
    "4x4_2_1_f32": (4, 2, 1, 2, False, "k_step_update<4, 2, false>"),  # one target: the general body
    "4x4_2_1_u8": (4, 2, 1, 2, True, "k_step_update<4, 2, true>"),
    "4x4_3_3_f32": (4, 3, 3, 2, False, "k_step_update<4, 8, false>"),  # an eight-tile kernel: per-lane stores
    "8x8_2_2_u8": (8, 2, 2, 6, True, "k_step_update<8, 2, true>"),     # the other kernel that writes through
}
CH0, CH2, CH1 = 77, 55, 33  # the sentinels

_RUNS = {}  # (S, T, Tt, K, N, mode) -> (levels, the oracle's run, a cell of every board no tile stands on in it): both types share it


def _run(oracle, S, T, Tt, K, N, mode):
    key = (S, T, Tt, K, N, mode)
    if key not in _RUNS:
        lv = cases.make_levels(oracle, S, T, Tt, K, N, True)
        run = _oracle_run(oracle, S, True, MAX_STEPS, lv, mode, STEPS)
        drawn = np.zeros((N, S * S), bool)  # cells a tile stands on at any time of the run: the start, then every step
        drawn[np.arange(N)[None, :], lv[1]] = True
        for row in run:
            drawn |= row["obs"][..., 1].reshape(N, S * S) != 0
        assert not drawn.all(axis=1).any(), "a board without an untouched cell"
        _RUNS[key] = (lv, run, np.argmin(drawn, axis=1))
    return _RUNS[key]


@pytest.mark.parametrize("mode_name", ("strict", "autoreset"))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_stores_over_the_boundary_batches(torch_cuda, oracle, shape, mode_name):
    """1, 63 / 64 / 65 and 255 / 256 / 257 boards, eight steps with max_steps 3, multi colour.  After every step pos, step_count,
    done, flags and reward equal the ts_step twin's and the oracle's, channel 1 equals both outside the sentinel cell, shown ==
    pos, and every sentinel stands; after the last step no guard byte has changed and no input was written."""
    torch = torch_cuda
    S, T, Tt, K, u8, kernel = SHAPES[shape]
    mode = oracle.MODE_AUTORESET if mode_name == "autoreset" else oracle.MODE_STRICT
    for N in BATCHES:
        lv, run, spare = _run(oracle, S, T, Tt, K, N, mode)
        a = _Raw(torch, S, T, Tt, True, MAX_STEPS, *lv, u8)
        b = _Raw(torch, S, T, Tt, True, MAX_STEPS, *lv, u8)
        assert _launches(b, kernel), (shape, N)
        b.show()
        held = _between_guards(torch, b)
        b.obs[..., 0] = CH0
        b.obs[..., 2] = CH2
        boards = torch.arange(N, device="cuda")
        spare_t = torch.from_numpy(spare).cuda()
        flat = b.obs.view(N, S * S, 3)
        flat[boards, spare_t, 1] = CH1
        elsewhere = torch.ones((N, S * S), dtype=torch.bool, device="cuda")
        elsewhere[boards, spare_t] = False
        rows = []
        for row in run:
            w = {f: torch.from_numpy(v).cuda() for f, v in row.items()}
            a.step(w["act"], mode)
            b.step_update(w["act"], mode)
            fa, fb = a.fields(), b.fields()
            ok = []
            for f in ("pos", "step_count", "done", "flags", "reward"):
                ok += [(fa[f] == fb[f]).all(), (fb[f] == w[f]).all()]
            mine = flat[..., 1]
            ok += [(mine == fa["obs"].view(N, S * S, 3)[..., 1])[elsewhere].all(),
                   (mine.to(torch.float32) == w["obs"].view(N, S * S, 3)[..., 1])[elsewhere].all(),
                   (b.shown == b.pos).all(), (flat[..., 0] == CH0).all(), (flat[..., 2] == CH2).all(), (flat[boards, spare_t, 1] == CH1).all()]
            rows.append(torch.stack(ok))
        labels = [f"{f} vs {ref}" for f in ("pos", "step_count", "done", "flags", "reward") for ref in ("ts_step", "oracle")] + [
            "channel 1 vs ts_step", "channel 1 vs oracle", "shown == pos", "channel 0", "channel 2", "the untouched channel-1 cell"]
        bad = [(k, labels[j]) for k, j in np.argwhere(~torch.stack(rows).cpu().numpy()).tolist()]
        assert not bad, (shape, N, mode_name, bad[:8])
        # the twin's observation carries no sentinel: give b's back what the sentinels replaced before the guards' comparison
        b.obs[..., 0] = a.obs[..., 0]
        b.obs[..., 2] = a.obs[..., 2]
        flat[boards, spare_t, 1] = 0
        _check_guards(a, held, (shape, N, mode_name))
