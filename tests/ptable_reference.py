"""CPU yardstick of the policy tables (test infrastructure, no test of its own): the definitions of
include/tiler_slider_ptable.h restated on NumPy and the CPU oracle.  It shares nothing with tiler_slider_amd/csrc/ts_ptable.hip:
the valid placements are enumerated as table_reference.exact enumerates them, the network's input is
`OracleBatch.encode_onehot()`, the logits are policy_reference's (logits_exact32 for integer weights, logits64 with its bound
otherwise), the action is policy_reference.select(..., GREEDY), the successor is ONE `OracleBatch.step`, the distance is relaxed
    dist[i] = 1 + dist[succ(i)]
until nothing changes, and the stopping rule is table_reference.cut as it is.  Imports neither torch nor the libraries.

    placements(S, blk, T)         (valid bool [N, states], cells int64 [T, states])
    actions(...)                  (act uint8 [N, states], logits [N, states, 4], bound or None)
    successors(...)               int64 [N, states]: succ(i) of the header, i itself where it is not defined
    walk(...)                     uint8 [N, states]: the policy table of an action table of ANY bytes
    score(...)                    int32 [N, 8]
    expert_actions(...)           uint8 [N, states], best bits uint8 [N, states]: ts_table_lookup on every placement
    expert_vote_mlp(...)          an integer network that follows the expert often enough to solve, and not always"""
import numpy as np

import policy_reference as pref
import table_reference as tref

NO_ACTION = 255


def placements(S, blk, T):
    blk = np.ascontiguousarray(blk, np.uint32)
    N, C = blk.shape[1], S * S
    states = C ** T
    idx = np.arange(states, dtype=np.int64)
    cells = np.stack([(idx // C ** t) % C for t in range(T)]) if T else np.zeros((0, states), np.int64)
    valid = np.ones((N, states), bool)
    for i in range(T):
        for j in range(i):
            valid &= (cells[i] != cells[j])[None, :]
    c = np.arange(C)
    blocked = ((blk[c // 32, :] >> (c % 32).astype(np.uint32)[:, None]) & 1).T != 0     # [N, C]
    for t in range(T):
        valid &= ~blocked[:, cells[t]]
    return valid, cells


def _batch(orc, S, mc, blk, tgt, valid, cells):
    """One oracle board per valid placement, standing on it: (batch, level of each, index of each)."""
    nb, ns = np.nonzero(valid)
    pos = np.ascontiguousarray(cells[:, ns].astype(orc.cell_dtype(S)))
    b = orc.OracleBatch(S, mc, 2 ** 30, np.ascontiguousarray(np.asarray(blk, np.uint32)[:, nb]), pos, np.ascontiguousarray(np.asarray(tgt)[:, nb]))
    return b, nb, ns


def actions(orc, S, mc, blk, tgt, T, mlp, exact32):
    """mlp = (w1 [H, D], b1, w2 [4, H], b2) in torch.nn.Linear's layout.  exact32: logits float32, exact (integer weights), bound
    None; otherwise logits float64 with policy_reference.logits64's bound, and act chosen on them."""
    valid, cells = placements(S, blk, T)
    N, states = valid.shape
    act = np.full((N, states), NO_ACTION, np.uint8)
    logits = np.zeros((N, states, 4), np.float32 if exact32 else np.float64)
    bound = None if exact32 else np.zeros((N, states, 4), np.float64)
    step = max(1, (1 << 17) // states)                                   # levels per batch: the one-hot planes stay small
    for n0 in range(0, N, step):
        part = np.zeros_like(valid)
        part[n0:n0 + step] = valid[n0:n0 + step]
        if not part.any():
            continue
        b, nb, ns = _batch(orc, S, mc, blk, tgt, part, cells)
        x =b.encode_onehot().reshape(b.n, -1)
        if exact32:
            z = pref.logits_exact32(x, mlp)
        else:
            z, bound[nb, ns] = pref.logits64(x, mlp)
        act[nb, ns] = pref.select(z, None, pref.GREEDY)
        logits[nb, ns] = z
    return act, logits, bound


def successors(orc, S, mc, blk, tgt, T, act):
    valid, cells = placements(S, blk, T)
    N, states = valid.shape
    act = np.asarray(act)
    assert act.dtype == np.uint8 and act.shape == (N, states)
    b, nb, ns = _batch(orc, S, mc, blk, tgt, valid, cells)
    a = act[nb, ns]
    moves = a <= 3
    b.step(np.where(moves, a, 0).astype(np.uint8), obs=False)
    assert (b.pos < S * S).all()
    succ = np.broadcast_to(np.arange(states, dtype=np.int64), (N, states)).copy()
    succ[nb[moves], ns[moves]] = tref.index_of(S, b.pos)[moves]
    assert valid[nb, succ[nb, ns]].all(), "a valid placement has an invalid successor"
    return succ


def walk_exact(orc, S, mc, blk, tgt, T, act):
    """int32 [N, states]: the least d with succ^d(i) won, tref.INVALID_PLACEMENT, or tref.UNREACHABLE."""
    valid, cells = placements(S, blk, T)
    N, states = valid.shape
    b, nb, ns = _batch(orc, S, mc, blk, tgt, valid, cells)
    won = b.won() != 0
    succ = successors(orc, S, mc, blk, tgt, T, act)
    dist = np.full(N * states, tref.UNREACHABLE, np.int32)
    dist[np.flatnonzero(~valid.ravel())] = tref.INVALID_PLACEMENT
    own = nb * states + ns
    dist[own[won]] = 0
    nxt = (nb * states + succ[nb, ns])[~won]
    own = own[~won]
    while True:
        new = np.minimum(dist[own], np.minimum(dist[nxt], tref.UNREACHABLE - 1) + 1)
        if np.array_equal(new, dist[own]):
            break
        dist[own] = new
    return dist.reshape(N, states)


def walk(orc, S, mc, blk, tgt, T, act, max_depth=tref.MAX_DEPTH):
    return tref.cut(walk_exact(orc, S, mc, blk, tgt, T, act), max_depth)


def score(orc, S, mc, blk, tgt, T, ptable, act, table):
    """ptable, act, table: uint8 [N, states] of any bytes."""
    valid, _ = placements(S, blk, T)
    p, o = np.asarray(ptable).astype(np.int64), np.asarray(table).astype(np.int64)
    succ = successors(orc, S, mc, blk, tgt, T, act)
    solvable, solved = valid & (o >= 1) & (o <= 252), valid & (p >= 1) & (p <= 252)
    agree = solvable & (np.asarray(act) <= 3) & (np.take_along_axis(o, succ, axis=1) == o - 1)
    both = solved & solvable
    cols = (valid, solvable, solved, solved & (p == o), agree, np.where(both, p - o, 0), valid & (p == 254), valid & (p == 0))
    return np.stack([c.sum(axis=1) for c in cols], axis=1).astype(np.int32)


def expert_actions(orc, S, mc, blk, tgt, T, table):
    """(action uint8 [N, states], best uint8 [N, states]) of table_reference.lookup on every valid placement of `table` (uint8
    [N, states]); 255 and 0 on invalid ones."""
    valid, cells = placements(S, blk, T)
    N, states = valid.shape
    nb, ns = np.nonzero(valid)
    pos = np.ascontiguousarray(cells[:, ns].astype(orc.cell_dtype(S)))
    _, best, action = tref.lookup(orc, S, np.ascontiguousarray(np.asarray(blk, np.uint32)[:, nb]), pos, table, rows=nb)
    act, bits = np.full((N, states), NO_ACTION, np.uint8), np.zeros((N, states), np.uint8)
    act[nb, ns], bits[nb, ns] = action, best
    return act, bits


def expert_vote_mlp(orc, S, mc, blk, tgt, T):
    """An integer network, exact in float32, whose hidden units are the identity on the tile planes (H = C in single colour, T * C
    in multi colour) and whose w2[a][unit (t, c)] is the number of placements, over all levels given, with tile t on cell c (single
    colour: any tile) whose best-move bit a is set; every other weight is zero.  Random integer networks solve a few per cent
    of the placements with chains of at most three moves; this one solves about half, some of them with detours."""
    C = S * S
    Tt = np.asarray(tgt).shape[0]
    table = tref.table(orc, S, mc, blk, tgt, T)
    _, bits = expert_actions(orc, S, mc, blk, tgt, T, table)
    valid, cells = placements(S, blk, T)
    H = T * C if mc else C
    D = (1 + T + Tt if mc else 3) * C
    w1, w2 = np.zeros((H, D), np.float32), np.zeros((4, H), np.float32)
    for t in range(T if mc else 1):
        for c in range(C):
            w1[t * C + c, (1 + t) * C + c] = 1
    for t in range(T):
        unit = (t * C if mc else 0) + cells[t]                           # [states]
        for a in range(4):
            votes = (valid & (((bits >> a) & 1) != 0)).sum(axis=0)       # over the levels
            np.add.at(w2[a], unit, votes.astype(np.float32))
    return w1, np.zeros(H, np.float32), w2, np.zeros(4, np.float32)


def summary(orc, S, mc, blk, tgt, T, mlp):
    """What a test input carries, from the yardstick's own numbers: a dict of counts over all levels."""
    act, z, _ = actions(orc, S, mc, blk, tgt, T, mlp, True)
    table = tref.table(orc, S, mc, blk, tgt, T)
    pt = walk(orc, S, mc, blk, tgt, T, act)
    sc = score(orc, S, mc, blk, tgt, T, pt, act, table).sum(axis=0)
    valid, _ = placements(S, blk, T)
    ties = ((z == z.max(axis=2, keepdims=True)).sum(axis=2) > 1) & valid
    dist = (pt >= 1) & (pt <= 252)
    return {"valid": int(sc[0]), "solvable": int(sc[1]), "solved": int(sc[2]), "optimal": int(sc[3]), "agree": int(sc[4]),
            "with_excess": int((dist & (table >= 1) & (table <= 252) & (pt != table)).sum()), "excess": int(sc[5]),
            "dist_ge_3": int((dist & (pt >= 3)).sum()), "longest": int(pt[dist].max(initial=0)),
            "never": int((valid & (table >= 1) & (table <= 252) & (pt == 255)).sum()), "ties": float(ties.sum() / max(1, valid.sum())),
            "deep_at_2": int((walk(orc, S, mc, blk, tgt, T, act, 2) == 254).sum())}
