"""The occupancy cases of the reach-table experts (test infrastructure, no test of its own): one case per kernel of the rexpert
library, on the shapes and levels of tests/reach_cases.py.  tests/test_gpu_rexpert.py runs the cases; tests/test_rexpert_cpu.py
pins their names to the code object.  Imports neither torch nor the libraries at import time."""
import reach_cases

WAVES = 4096
N_BOARDS = WAVES * 64 - 3      # 262,141 boards, one per lane: the last wave is ragged; they replicate the 128 levels through rows=
STEPS, EPSILON, MAX_STEPS, SEED = 6, 0.25, 4, 0x0CCE

# kernel name -> (S, tiles, obstacles).  The labels run over the same STEPS * N_BOARDS samples, a sample per lane.
CASES = {f"k_rexpert_{what}<{S}>": (S, T, K) for S, (T, K, _) in reach_cases.SHAPES.items() for what in ("rollout", "labels")}
