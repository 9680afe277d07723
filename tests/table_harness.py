"""Shared pieces of the distance-table tests (test infrastructure, no test of its own): buffers between guard bytes for raw
C-ABI calls, the save / set / restore of the ts_table_tuning knobs, and the table of occupancy cases - one per kernel of the
table library - that tests/test_gpu_table.py runs and tests/test_table_cpu.py pins to the code object.  Imports neither torch
nor the libraries at import time."""
import numpy as np

GUARD, GUARD_BYTE = 256, 0xA5


def guarded(torch, device, fill):
    """uint8 device buffer: GUARD guard bytes, the bytes of `fill` (a numpy array), GUARD guard bytes."""
    raw = np.ascontiguousarray(fill).reshape(-1).view(np.uint8)
    buf = torch.full((2 * GUARD + raw.size,), GUARD_BYTE, dtype=torch.uint8, device=device)
    if raw.size:
        buf[GUARD:GUARD + raw.size] = torch.from_numpy(raw.copy()).to(device)
    return buf


def payload(buf, dtype, shape):
    """After the call: every guard byte as it was; the payload as a numpy array (the copy to the host waits for the stream)."""
    host = buf.cpu().numpy()
    assert (host[:GUARD] == GUARD_BYTE).all() and (host[len(host) - GUARD:] == GUARD_BYTE).all(), "a guard byte was overwritten"
    return host[GUARD:len(host) - GUARD].view(dtype).reshape(shape)


class knobs:
    """Sets ts_table_tuning knobs by the names of tiler_slider_amd._table_cabi and restores all three."""

    def __init__(self, values):
        from tiler_slider_amd import _table_cabi as tc
        self.tc, self.L, self.values = tc, tc.lib(), values
        self.keys = (tc.TUNE_WAVE_MAX_STATES, tc.TUNE_STATES_PER_LANE, tc.TUNE_BLOCK_BELOW_BOARDS)

    def __enter__(self):
        self.saved = tuple(self.L.ts_table_tuning(k, -1) for k in self.keys)
        for name, v in self.values.items():
            self.L.ts_table_tuning(getattr(self.tc, name), v)
        return self

    def __exit__(self, *exc):
        for k, v in zip(self.keys, self.saved):
            self.L.ts_table_tuning(k, v)


# kernel name -> (S, T, obstacles, the ts_table_tuning knobs that force its form); tests/test_table_cpu.py pins the names to the
# code object.  Two tiles from 4x4 up keep the tables modest: 4,349 boards of 8x8 are 17 MiB.
# size -> (tiles, obstacles); 2x2 takes two tiles and an obstacle, so its targets cannot be drawn beside the tiles (test_gpu_table._occupancy_levels)
_OCC_SHAPES = {1: (1, 0), 2: (2, 1), 3: (2, 1), 4: (2, 2), 5: (2, 3), 6: (2, 6), 7: (2, 8), 8: (2, 10)}
_WAVE_KNOBS = {"TUNE_BLOCK_BELOW_BOARDS": 0, "TUNE_WAVE_MAX_STATES": 65536}   # else the small-batch rule takes the block form
_BLOCK_KNOBS = {"TUNE_WAVE_MAX_STATES": 0}
OCCUPANCY_CASES = {}
for _S, (_T, _K) in _OCC_SHAPES.items():
    OCCUPANCY_CASES[f"k_table_wave<{_S}>"] = (_S, _T, _K, _WAVE_KNOBS)
    if _S >= 2:
        OCCUPANCY_CASES[f"k_table_block<{_S}>"] = (_S, _T, _K, _BLOCK_KNOBS)
    OCCUPANCY_CASES[f"k_table_lookup<{_S}>"] = (_S, _T, _K, {})
# the same k_table_wave<4> with eight lanes per board: eight boards per wave, and idle groups in the ragged last block
SUB_WAVE_CASE = (4, 2, 2, {**_WAVE_KNOBS, "TUNE_STATES_PER_LANE": 32})
SUB_WAVE = "k_table_wave<4>, eight boards per wave"
