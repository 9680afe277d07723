"""The occupancy cases of the hashed solver and the reachable distance tables (test infrastructure, no test of its own): one case
per kernel of the reach and rtable libraries, the levels each case is run on, and the conditions the yardsticks' answers must meet
before a GPU test may rely on them.  tests/test_gpu_reach_occupancy.py runs the cases; tests/test_reach_cpu.py and
tests/test_rtable_cpu.py pin their names to the code objects and check the conditions on the CPU.  Imports neither torch nor the
libraries at import time.

Every size that has room for them takes more than four tiles - the upper half of the key, hi = idx / (S * S) ** 4, is then a real
division for S = 3, 5, 6, 7 - and on 6x6, 7x7 and 8x8 the keys pass 2^32."""
import numpy as np

# size -> (tiles, obstacles, seed offset of the draw).  8x8 takes 38 obstacles: with 30 the walk of the odd-numbered levels leaves
# only two roots where they stood (won), and the conditions below ask for three
SHAPES = {1: (1, 0, 0), 2: (3, 0, 0), 3: (5, 1, 0), 4: (5, 2, 1000), 5: (6, 12, 1000), 6: (7, 18, 1000), 7: (6, 24, 1000), 8: (8, 38, 1000)}
DISTINCT = 128          # levels of a case
CAPACITY = 1024         # states a level may hold: some levels of every case from 3x3 up are FULL
GRID = 1024             # blocks of a launch of k_reach and k_rtable_build, whatever the batch (kMaxInFlight)
N_BUILD = GRID + 61     # boards of a build or a search: a full grid and a ragged second pass through 61 of the slices
LOOKUP_WAVES = 4096
N_LOOKUP = LOOKUP_WAVES * 64 - 3   # boards of a lookup, one per lane
WALK, WALK_SEED = 10, 0x3A1C
LONG_KEY = 1 << 32

REACH_CASES = {f"k_reach<{S}>": (S, T, K) for S, (T, K, _) in SHAPES.items()}
RTABLE_CASES = {f"k_rtable_{what}<{S}>": (S, T, K) for S, (T, K, _) in SHAPES.items() for what in ("build", "lookup")}


def walked(orc, S, blk, init, moves=WALK, seed=WALK_SEED):
    """Where `moves` moves of ts_fill_actions' stream leave the tiles of every level (as test_gpu_reach._walked walks them)."""
    n = init.shape[1]
    b = orc.OracleBatch(S, True, 2**30, blk, init, init)
    b.reset()
    for k in range(moves):
        b.step(orc.fill_actions(n, seed=seed, step_index=k), obs=False)
    return b.pos.copy()


def levels(orc, S, mc, n=DISTINCT):
    """(blk, init, tgt) of the case of size S.  Odd-numbered levels take their targets where WALK moves leave the tiles - they
    can be won, at spread distances -, even-numbered levels take targets drawn on their own and can mostly not be won."""
    T, K, offset = SHAPES[S]
    if S == 1:   # one cell: the tile sits on its target (won), or there is no target to sit on (single colour: never won)
        return np.zeros((1, n), np.uint32), np.zeros((1, n), np.uint8), np.zeros((1 if mc else 0, n), np.uint8)
    if 2 * T + K > S * S:   # no room for tiles, targets and obstacles side by side: the targets are drawn on their own
        blk, init, _ = orc.generate(S, T, 0, K, n, seed=0x50F7 + offset)
        _, _, tgt = orc.generate(S, 0, T, 0, n, seed=0x50F8 + offset)
    else:
        blk, init, tgt = orc.generate_mt19937(S, T, T, K, np.arange(offset, offset + n, dtype=np.uint32))
    tgt = tgt.copy()
    tgt[:, 1::2] = walked(orc, S, blk, init)[:, 1::2]
    return blk, init, np.ascontiguousarray(tgt)


def stepped(orc, S, mc, blk, init, tgt, seed=0x0CC5):
    """(actions, pos): one move of ts_fill_actions' stream per level and the cells it leaves - the root of a build on st->pos."""
    act = orc.fill_actions(init.shape[1], seed=seed, step_index=0)
    twin = orc.OracleBatch(S, mc, 2**30, blk, init, tgt)
    twin.reset()
    twin.step(act, obs=False)
    return act, twin.pos.copy()


def rtable_summary(ref):
    """What a Reference covers, from the yardstick alone."""
    finite = (ref.entry >= 1) & (ref.entry <= 252)
    return dict(built_100=int((ref.count >= 100).sum()), full=int((ref.count == -3).sum()), won=int((ref.root_moves == 0).sum()),
                root_moves=sorted(set(ref.root_moves[ref.root_moves >= 1].tolist())), finite=int(finite.sum()), none=int((ref.entry == 255).sum()),
                largest=int(ref.count.max()), deepest=int(ref.deepest.max()), long_keys=int((ref.idx >= LONG_KEY).sum()))


def check_rtable(S, ref):
    """The conditions that keep a test of the case from passing on degenerate input; returns rtable_summary(ref)."""
    s = rtable_summary(ref)
    if S <= 2:   # reachable sets of 1 to 12 states
        return s
    assert s["built_100"] >= 8 and s["full"] >= 3 and s["won"] >= 3 and len(s["root_moves"]) >= 3 and s["finite"] >= 1 and s["none"] >= 1, (S, s)
    assert S < 6 or s["long_keys"] >= 1000, (S, s)
    return s


def reach_summary(want):
    moves = want[0]
    return dict(solved=int((moves >= 1).sum()), won=int((moves == 0).sum()), none=int((moves == -1).sum()), depth=int((moves == -2).sum()),
                full=int((moves == -3).sum()), deepest=int(moves.max()), most_states=int(want[2].max()))


def check_reach(S, want):
    s = reach_summary(want)
    if S >= 3:
        assert s["solved"] >= 3 and s["none"] >= 3 and s["full"] >= 3, (S, s)
    return s
