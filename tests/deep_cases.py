"""The deep levels and their chain policies (test infrastructure, no test of its own): tests/golden/deep_levels.npz - levels whose
farthest winnable placement lies 37 to 106 moves from the win, found by tools/find_deep_levels.py -, each level's yardstick
distances (table_reference.exact, computed once per process), and a tabular policy with LONG chains on a level.

The chain policy: a depth-first tree grown backwards from the won placements over the predecessor edges (s -> succ_a(s), one
OracleBatch.step per move through ptable_reference.successors), the predecessors of a node taken in a seeded shuffled order; every
node's action is the move to its parent, every placement off the tree - and every won one - has 255.  Depth-first trees are
deep: the chains of such a policy are the tree's depths, far beyond the level's distances.  Imports neither torch nor the
libraries; tests/test_deep_cpu.py holds the fixture and the policies to the yardstick's numbers."""
import os
from collections import namedtuple

import numpy as np

import ptable_reference as xref
import table_reference as tref

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deep_levels.npz")
DEEP_FROM = 36                      # the first distance no level of the shallow suite holds

Level = namedtuple("Level", "name S T Tt mc blk tgt init deepest seed")     # blk [W, 1], tgt [Tt, 1], init [T, 1]: one board each

# name of the level in the fixture: 4,096 states in both colour modes, n_tiles != n_targets with a repeated target, 625 and 15,625 states
MULTI, SINGLE, REPEATED, SMALL, LARGE = ("8x8 two tiles multi colour", "8x8 two tiles single colour",
                                         "8x8 two tiles three targets one repeated single colour", "5x5 two tiles multi colour",
                                         "5x5 three tiles multi colour")
# level -> seed of its chain policy (chain_policy); test_deep_cpu.py asserts what each gives
CHAIN_SEED = {MULTI: 0, SMALL: 1, LARGE: 0}

_levels, _exact, _chains = None, {}, {}


def levels():
    """{name: Level} of the fixture."""
    global _levels
    if _levels is None:
        with np.load(FIXTURE) as z:
            g = {k: z[k] for k in z.files}
        _levels = {}
        for i, name in enumerate(g["name"].tolist()):
            S, T, Tt = int(g["size"][i]), int(g["tiles"][i]), int(g["targets"][i])
            W = (S * S + 31) // 32
            _levels[name] = Level(name, S, T, Tt, bool(g["multi_color"][i]), np.ascontiguousarray(g["blk"][i, :W].reshape(W, 1)),
                                  np.ascontiguousarray(g["tgt"][i, :Tt].reshape(Tt, 1)), np.ascontiguousarray(g["init"][i, :T].reshape(T, 1)),
                                  int(g["deepest"][i]), int(g["seed"][i]))
    return _levels


def exact(orc, lv):
    """int32 [states]: table_reference.exact of the level, computed once.  Do not write to it."""
    if lv.name not in _exact:
        _exact[lv.name] = tref.exact(orc, lv.S, lv.mc, lv.blk, lv.tgt, lv.T)[0]
        _exact[lv.name].setflags(write=False)
    return _exact[lv.name]


def deepest(dist):
    """The largest finite distance of exact()'s answer."""
    return int(dist[(dist >= 0) & (dist < tref.UNREACHABLE)].max())


def cells_of(lv, idx):
    """uint8 [T, len(idx)]: the cells of placements given by index."""
    C = lv.S * lv.S
    idx = np.asarray(idx, np.int64)
    return np.stack([(idx // C ** t) % C for t in range(lv.T)]).astype(np.uint8)


def tiled(lv, n):
    """(blk, tgt) of n copies of the level."""
    return np.ascontiguousarray(np.repeat(lv.blk, n, axis=1)), np.ascontiguousarray(np.repeat(lv.tgt, n, axis=1))


def _board(lv, name, free, targets):
    """A level of lv's shape whose free cells are `free` (None: lv's own obstacles)."""
    C, W = lv.S * lv.S, lv.blk.shape[0]
    blk = lv.blk.copy() if free is None else np.zeros((W, 1), np.uint32)
    for c in (() if free is None else set(range(C)) - set(free)):
        blk[c >> 5, 0] |= np.uint32(1 << (c & 31))
    tgt = np.array(targets, np.uint8).reshape(lv.Tt, 1)
    init = lv.init.copy() if free is None else np.array(sorted(free)[:lv.T], np.uint8).reshape(lv.T, 1)
    return Level(name, lv.S, lv.T, lv.Tt, lv.mc, blk, tgt, init, -1, -1)


def companions(lv):
    """Three 8x8 two-tile multi-colour levels that stop long before the deep one, for the boards that share a wave with it:
    `shallow` - a room of five cells, every distance at most 3; `never won` - the deep level's obstacles with both targets on
    one cell (two tiles never share a cell); `won or stuck` - two free cells: the won placement, and the swapped one from which
    nothing moves.  tests/test_deep_cpu.py asserts these properties on the yardstick's answer."""
    assert (lv.S, lv.T, lv.Tt, lv.mc) == (8, 2, 2, True)
    return {"shallow": _board(lv, "shallow", (0, 1, 2, 8, 9), (0, 1)),
            "never won": _board(lv, "never won", None, (int(lv.tgt[0, 0]), int(lv.tgt[0, 0]))),
            "won or stuck": _board(lv, "won or stuck", (0, 1), (0, 1))}


def chain_policy(orc, lv, seed=None):
    """(act uint8 [states], chain int32 [states]): the backward depth-first tree described above and, from
    ptable_reference.walk_exact - not from the tree -, the number of moves the policy takes from every placement
    (table_reference.UNREACHABLE off the tree, INVALID_PLACEMENT on invalid placements).  Computed once per (level, seed)."""
    seed = CHAIN_SEED[lv.name] if seed is None else seed
    if (lv.name, seed) in _chains:
        return _chains[lv.name, seed]
    dist = exact(orc, lv)
    states = dist.size
    succ = np.stack([xref.successors(orc, lv.S, lv.mc, lv.blk, lv.tgt, lv.T, np.full((1, states), a, np.uint8))[0] for a in range(4)])
    valid, won = dist != tref.INVALID_PLACEMENT, dist == 0
    pred = [[] for _ in range(states)]                                   # pred[p]: (s, a) with succ_a(s) = p, s valid, not won, s != p
    for a in range(4):
        for s in np.flatnonzero(valid & ~won & (succ[a] != np.arange(states))):
            pred[succ[a][s]].append((int(s), a))
    rng = np.random.default_rng(seed)
    act = np.full(states, xref.NO_ACTION, np.uint8)
    seen = won.copy()
    for root in np.flatnonzero(won):
        stack = [iter([pred[root][i] for i in rng.permutation(len(pred[root]))])]
        while stack:
            nxt = next(stack[-1], None)
            if nxt is None:
                stack.pop()
            elif not seen[nxt[0]]:
                s, a = nxt
                seen[s], act[s] = True, a
                stack.append(iter([pred[s][i] for i in rng.permutation(len(pred[s]))]))
    chain = xref.walk_exact(orc, lv.S, lv.mc, lv.blk, lv.tgt, lv.T, act[None, :])[0]
    act.setflags(write=False)
    chain.setflags(write=False)
    _chains[lv.name, seed] = (act, chain)
    return act, chain


def longest(chain):
    return int(chain[(chain >= 0) & (chain < tref.UNREACHABLE)].max())
