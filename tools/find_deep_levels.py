"""Search for DEEP levels - levels whose farthest winnable placement lies more than 35 moves from the win - and write them to
tests/golden/deep_levels.npz (CPU only; never runs a kernel).

A seeded hill-climb over the CPU yardstick: tests/table_reference.exact over oracle/.  A level is a set of obstacles and a list
of targets; one move of the search moves, adds or removes one obstacle or moves one target, a batch of such moves is evaluated in
one call of the yardstick, and the best is kept if the deepest finite distance of the level does not fall (ties: the level with
more placements at distance >= 36).  Every search starts from one 8x8 layout of 13 obstacles found by an earlier throw-away
search, cut to the board size it runs on, so the first evaluation of the 8x8 levels already tells whether that layout reproduces.

The fixture holds levels only, a few hundred bytes: per level the size, tile count, target count, colour mode, the obstacle
words `blk` (uint32 [L, 2], the device layout, zero padded), the targets `tgt` (uint8 [L, 3], padded with 255), `init` (uint8
[L, 4], the lowest-index placement at the deepest distance, padded with 255), the recorded deepest distance and the seed.
tests/deep_cases.py loads it; tests/test_deep_cpu.py holds it to the yardstick.

    python tools/find_deep_levels.py                      # the committed fixture: about two minutes of one core
    python tools/find_deep_levels.py --seconds 600        # a longer climb per searched level

The climb is deterministic for a seed and a number of STEPS (--steps), not for a number of seconds; the committed fixture was
made with the default --steps and --seed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

START_OBSTACLES = (2, 13, 16, 22, 25, 28, 31, 33, 37, 46, 56, 59, 62)     # cells row * 8 + col of an 8x8 board
START_TARGETS = (24, 4)
DEEP_FROM = 36                                                            # the first distance the shallow suite never reaches

# name, size, tiles, targets, multi colour, steps of the climb (0: the start layout as it is)
LEVELS = (("8x8 two tiles multi colour", 8, 2, 2, True, 0),
          ("8x8 two tiles single colour", 8, 2, 2, False, 0),
          ("8x8 two tiles three targets one repeated single colour", 8, 2, 3, False, 0),
          ("5x5 two tiles multi colour", 5, 2, 2, True, 3000),
          ("5x5 three tiles multi colour", 5, 3, 3, True, 300))


def pack(S, obstacles, targets):
    """(blk uint32 [W, 1], tgt uint8 [Tt, 1]) of one level in the device layout."""
    blk = np.zeros(((S * S + 31) // 32, 1), np.uint32)
    for c in obstacles:
        blk[c >> 5, 0] |= np.uint32(1 << (c & 31))
    return blk, np.array(targets, np.uint8).reshape(-1, 1)


def start_layout(S, Tt, mc):
    """The 8x8 start layout cut to an SxS board: the obstacles and targets whose row and column lie on it; a target that falls off,
    and in multi colour a third target, goes to the first free cell; in single colour a third target repeats the first."""
    on = lambda c: c // 8 < S and c % 8 < S
    obstacles = sorted((c // 8) * S + c % 8 for c in START_OBSTACLES if on(c))
    targets = []
    for k in range(Tt):
        c = START_TARGETS[k] if k < len(START_TARGETS) else None
        if c is None and not mc:
            targets.append(targets[0])
        elif c is not None and on(c):
            targets.append((c // 8) * S + c % 8)
        else:
            targets.append(next(f for f in range(S * S) if f not in obstacles and f not in targets))
    return obstacles, targets


def evaluate(orc, tref, S, T, mc, candidates):
    """[(deepest finite distance or -1, placements at distance >= DEEP_FROM)] of (obstacles, targets) candidates, one yardstick call."""
    packed = [pack(S, o, t) for o, t in candidates]
    blk, tgt = np.concatenate([p[0] for p in packed], axis=1), np.concatenate([p[1] for p in packed], axis=1)
    dist = tref.exact(orc, S, mc, blk, tgt, T)
    finite = (dist >= 0) & (dist < tref.UNREACHABLE)
    deepest = np.where(finite, dist, -1).max(axis=1)
    return [(int(d), int(n)) for d, n in zip(deepest, (finite & (dist >= DEEP_FROM)).sum(axis=1))]


def mutate(rng, S, T, Tt, mc, obstacles, targets):
    """One move of the search; None where the draw gives no level (a target on an obstacle, too few free cells, ...)."""
    C = S * S
    obstacles, targets = list(obstacles), list(targets)
    free = [c for c in range(C) if c not in obstacles]
    kind = rng.integers(4)
    if kind == 0 and obstacles:                                        # move an obstacle
        obstacles[rng.integers(len(obstacles))] = free[rng.integers(len(free))]
    elif kind == 1 and len(free) > T + 2:                              # add one
        obstacles.append(free[rng.integers(len(free))])
    elif kind == 2 and obstacles:                                      # remove one
        del obstacles[rng.integers(len(obstacles))]
    else:                                                              # move a target (a repeated one moves with its twin)
        k = rng.integers(Tt)
        new = free[rng.integers(len(free))]
        targets = [new if t == targets[k] else t for t in targets]
    if set(targets) & set(obstacles) or (mc and len(set(targets)) != len(targets)) or C - len(obstacles) < T:
        return None
    return sorted(set(obstacles)), targets


def climb(orc, tref, rng, S, T, Tt, mc, steps, batch, seconds, log):
    level = start_layout(S, Tt, mc)
    best = evaluate(orc, tref, S, T, mc, [level])[0]
    log(f"  start: deepest {best[0]}, {best[1]} placements at distance >= {DEEP_FROM}")
    t0 = time.time()
    for step in range(steps):
        if seconds is not None and time.time() - t0 > seconds:
            break
        cands = [c for c in (mutate(rng, S, T, Tt, mc, *level) for _ in range(batch)) if c is not None]
        if not cands:
            continue
        scores = evaluate(orc, tref, S, T, mc, cands)
        k = max(range(len(cands)), key=lambda i: scores[i])
        if scores[k][0] >= best[0]:                                     # sideways moves are taken: they leave plateaus
            if scores[k] > best:
                log(f"  step {step}: deepest {scores[k][0]}, {scores[k][1]} at distance >= {DEEP_FROM}, {len(cands[k][0])} obstacles")
            level, best = cands[k], scores[k]
    return level, best


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=float, default=1.0, help="multiplies the steps of every searched level")
    ap.add_argument("--batch", type=int, default=16, help="moves evaluated per step")
    ap.add_argument("--seconds", type=float, default=None, help="stop each climb after this long (not reproducible)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "deep_levels.npz"))
    args = ap.parse_args()
    import table_reference as tref
    from oracle import binding as orc
    orc.lib().tso_set_num_threads(1)
    log = lambda s: print(s, flush=True)
    L = len(LEVELS)
    out = {"name": np.array([l[0] for l in LEVELS]), "size": np.zeros(L, np.int32), "tiles": np.zeros(L, np.int32),
           "targets": np.zeros(L, np.int32), "multi_color": np.zeros(L, np.uint8), "blk": np.zeros((L, 2), np.uint32),
           "tgt": np.full((L, 3), 255, np.uint8), "init": np.full((L, 4), 255, np.uint8), "deepest": np.zeros(L, np.int32),
           "seed": np.full(L, args.seed, np.int64)}
    t0 = time.time()
    for i, (name, S, T, Tt, mc, steps) in enumerate(LEVELS):
        log(f"{name}:")
        rng = np.random.default_rng([args.seed, i])
        (obstacles, targets), (deepest, n_deep) = climb(orc, tref, rng, S, T, Tt, mc, int(steps * args.steps), args.batch, args.seconds, log)
        blk, tgt = pack(S, obstacles, targets)
        dist = tref.exact(orc, S, mc, blk, tgt, T)[0]
        finite = (dist >= 0) & (dist < tref.UNREACHABLE)
        assert deepest == dist[finite].max() > DEEP_FROM - 1, (name, deepest)
        far = int(np.flatnonzero(finite & (dist == deepest))[0])
        out["size"][i], out["tiles"][i], out["targets"][i], out["multi_color"][i], out["deepest"][i] = S, T, Tt, mc, deepest
        out["blk"][i, :blk.shape[0]], out["tgt"][i, :Tt] = blk[:, 0], tgt[:, 0]
        out["init"][i, :T] = [(far // (S * S) ** t) % (S * S) for t in range(T)]
        log(f"  kept: deepest {deepest}, {n_deep} placements at distance >= {DEEP_FROM}, obstacles {obstacles}, targets {targets}  [{time.time() - t0:.0f} s]")
    np.savez(args.out, **out)
    log(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
