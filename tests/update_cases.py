"""The table of in-place step cases (test infrastructure, no test of its own): one per kernel of the update library, the
levels each one runs on and what the CPU oracle makes of them.  tests/test_update_cpu.py pins the names to the code object
and holds the oracle's trajectories to the floors below; tests/test_gpu_update.py launches every entry in a ragged batch and
at 4,096 waves.  Imports neither torch nor the libraries at import time."""
import numpy as np

LEVEL_SEED = 0x715311DE   # bench.py's
ACTION_SEED = 0xAC710005
VOID = 0x10 | 0x20 | 0x40  # STEPPED_DONE | AUTORESET | BAD_ACTION: no transition was played
IS_WON, INVALID_MOVE, SUCCESS, TIMEOUT, AUTORESET = 0x01, 0x02, 0x04, 0x08, 0x20

# (S, TMAX) -> (T, Tt, obstacles): the smallest shapes that reach each kernel and between them every relation of the counts.
#   <1, 8>  Tt > C: every target clamps to cell 0          <2, 8>  MT = C < TMAX and a full board: nothing can move
#   <3, 2>  no targets, st->tgt is NULL                    <3, 8>  TMAX = 8 chosen by Tt alone, Tt > T
#   <5, 2>  T > Tt                                         <7, 2>  Tt > T
#   S = 6, 7: 64-bit masks that are only partly filled (36 and 49 cells)
#
# What the oracle gives for levels(...) of 331 boards under ACTION_SEED's unpatched stream, 24 steps, max_steps 6, autoreset mode
# (stats(); multi colour / single colour): share of board-steps that moved a tile, wins, autoresets, timeouts
#   <1, 2>  0.00 / 0.00   3972 / 3972   3972 / 3972   0 / 0          <1, 8>  0.00 / 0.00   0 / 3972      993 / 3972    993 / 0
#   <2, 2>  0.25 / 0.24   703 / 1131    1342 / 1557   734 / 566      <2, 8>  0.00 / 0.00   180 / 3972    1128 / 3972   948 / 0
#   <3, 2>  0.39 / 0.39   0 / 0         993 / 993     993 / 993      <3, 8>  0.49 / 0.49   0 / 0         993 / 993     993 / 993
#   <4, 2>  0.54 / 0.54   303 / 311     1173 / 1174   912 / 907      <4, 8>  0.56 / 0.56   263 / 267     1156 / 1159   932 / 931
#   <5, 2>  0.56 / 0.56   0 / 0         993 / 993     993 / 993      <5, 8>  0.59 / 0.59   254 / 259     1152 / 1154   936 / 934
#   <6, 2>  0.58 / 0.58   261 / 261     1158 / 1158   934 / 934      <6, 8>  0.63 / 0.63   247 / 247     1157 / 1157   948 / 948
#   <7, 2>  0.52 / 0.52   0 / 0         993 / 993     993 / 993      <7, 8>  0.65 / 0.65   248 / 248     1159 / 1159   948 / 948
#   <8, 2>  0.59 / 0.59   276 / 279     1169 / 1170   932 / 930      <8, 8>  0.66 / 0.66   248 / 248     1159 / 1159   948 / 948
# assert_floors() holds every such run to: moved >= 0.2 and timeouts >= 500 where a tile can move (S >= 2, T < S*S), moved == 0
# elsewhere; wins >= 100 where T == Tt and a tile can move, wins == 0 where T != Tt (but <1, 8> in single colour, where the one
# cell is every target); autoresets >= 900.
_SHAPES = {
    (1, 2): (1, 1, 0), (1, 8): (1, 3, 0),
    (2, 2): (2, 2, 0), (2, 8): (4, 4, 0),
    (3, 2): (1, 0, 2), (3, 8): (2, 3, 1),
    (4, 2): (2, 2, 2), (4, 8): (3, 3, 2),
    (5, 2): (2, 1, 3), (5, 8): (3, 3, 3),
    (6, 2): (2, 2, 4), (6, 8): (5, 5, 4),
    (7, 2): (1, 2, 5), (7, 8): (8, 8, 5),
    (8, 2): (2, 2, 6), (8, 8): (8, 8, 10),
}
# kernel name -> (S, T, Tt, obstacles); both observation types of a shape run the same levels
CASES = {f"k_step_update<{S}, {tmax}, {u8}>": (S, T, Tt, K) for (S, tmax), (T, Tt, K) in _SHAPES.items() for u8 in ("false", "true")}


def is_u8(name):
    return name.endswith(", true>")


def shape_key(name):
    """What the two observation types of a shape share: their levels and the oracle's trajectory."""
    return CASES[name]


def make_levels(oracle, S, T, Tt, K, N, mc=True):
    """(blk, init, tgt) of N boards.  ts_generate's twin with LEVEL_SEED where it can draw T + Tt + K distinct cells; all zeros on
    the one-cell board; on a 2x2 board of four tiles a permutation of the cells for the tiles and another for the targets.
    Then every even board whose tiles move under action (b // 2) % 4 takes the cells they reach as its targets (equal counts
    only): random play wins those about one step in four, and again after each autoreset."""
    C = S * S
    if S == 1:
        blk, init, tgt = np.zeros((1, N), np.uint32), np.zeros((T, N), np.uint8), np.zeros((Tt, N), np.uint8)
    elif T + Tt + K <= C:
        blk, init, tgt = oracle.generate(S, T, Tt, K, N, seed=LEVEL_SEED)
    else:
        assert (S, T, Tt, K) == (2, 4, 4, 0), (S, T, Tt, K)
        rng = np.random.default_rng(LEVEL_SEED)
        blk = np.zeros((1, N), np.uint32)
        init = np.ascontiguousarray(rng.permuted(np.tile(np.arange(4, dtype=np.uint8), (N, 1)), axis=1).T)
        tgt = np.ascontiguousarray(rng.permuted(np.tile(np.arange(4, dtype=np.uint8), (N, 1)), axis=1).T)
    if T == Tt and S > 1:
        ref = oracle.OracleBatch(S, mc, 1 << 20, blk, init, tgt)
        ref.reset()
        flags = ref.step(((np.arange(N) // 2) % 4).astype(np.uint8), mode=oracle.MODE_STRICT, obs=False)["flags"]
        take = ((flags & (VOID | INVALID_MOVE)) == 0) & (np.arange(N) % 2 == 0)
        tgt = tgt.copy()
        tgt[:, take] = ref.pos[:, take]
    return blk, init, tgt


def levels(oracle, name, N, mc=True):
    return make_levels(oracle, *CASES[name], N, mc)


def stats(flags):
    """Of the oracle's flags [steps][N]: share of board-steps that moved a tile, wins, autoresets, timeouts."""
    flags = np.asarray(flags)
    moved = int(((flags & (VOID | INVALID_MOVE)) == 0).sum())
    return (moved / flags.size, int(((flags & SUCCESS) != 0).sum()), int(((flags & AUTORESET) != 0).sum()),
            int(((flags & TIMEOUT) != 0).sum()))


def can_move(name):
    S, T, Tt, K = CASES[name]
    return S >= 2 and T < S * S


def wins_expected(name, mc):
    """True: the run has to contain wins; False: it cannot contain one; None: no claim (the full 2x2 board, where single colour
    wins every step and multi colour wins where the two permutations agree)."""
    S, T, Tt, K = CASES[name]
    if S == 1:
        return T == Tt or not mc  # one cell: the tile stands on every target - unless the counts differ in multi colour
    if T != Tt:
        return False
    return True if T < S * S else None


def assert_floors(name, mc, flags):
    """The floors of a 331-board, 24-step, max_steps 6 autoreset run - on the ORACLE's flags, never on a kernel's."""
    moved, wins, resets, timeouts = stats(flags)
    what = (name, mc, moved, wins, resets, timeouts)
    if can_move(name):
        assert moved >= 0.2 and timeouts >= 500, what
    else:
        assert moved == 0, what
    expected = wins_expected(name, mc)
    if expected is True and can_move(name):
        assert wins >= 100, what
    elif expected is False:
        assert wins == 0, what
    assert resets >= 900, what
    return moved, wins, resets, timeouts
