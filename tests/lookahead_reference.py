"""CPU yardstick of the lookahead (test infrastructure, no test of its own): the definition of include/tiler_slider_lookahead.h
restated on NumPy over the CPU oracle.  The frontier is expanded ply by ply - every board of ply p - 1 stepped by the oracle with
each of the four actions, levels replicated, `done` and `step_count` cleared, max_steps out of reach -, IS_WON and INVALID_MOVE are
read from the oracle's flags, the leaves are evaluated in float64 by policy_reference.logits64 / ac_reference.outputs64 on the
oracle's one-hot planes, and the values are backed up with a rigorous bound on the error of ANY float32 evaluation.  It shares no
code with tiler_slider_amd/csrc/ts_lookahead.hip and imports neither torch nor the libraries at import time.

THE BOUND, with u = 2**-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1, as
in policy_reference).  A leaf value X^ computed in float32 lies within BX of the exact X: BX is logits64's / outputs64's own bound,
and for QMAX the largest of the four (max is 1-Lipschitz in the sup norm: |max a - max b| <= max |a - b|).  One backup step
computes q^ = w_step + w_win [won] + w_invalid [!moved] + g X^ (g the discount; X^ replaced by 0 where the move wins): a sum of four
terms, one of them a product, in any order, fused or not - at most four roundings touch any term, so

    |q^ - q| <= g BX + gamma_4 (|w_step| + |w_win| [won] + |w_invalid| [!moved] + g (|X| + BX))

and the maximum over the four actions carries the largest of the four bounds to the ply above.  With exactly representable
inputs whose partial sums are exact (integer weights, g a power of two) every float32 evaluation IS the float64 value."""
import numpy as np

import ac_reference as aref
import policy_reference as pref

LEAF_ZERO, LEAF_VALUE, LEAF_QMAX = 0, 1, 2
NO_ACTION = 255
FLAG_IS_WON, FLAG_INVALID_MOVE = 0x01, 0x02
BIG_STEPS = 1 << 30
CHUNK = 1 << 15

gamma_n = pref.gamma


def _batch(orc, S, mc, blk, tgt, cells):
    return orc.OracleBatch(S, mc, BIG_STEPS, blk, np.ascontiguousarray(cells), tgt)


def won_on(orc, S, mc, blk, tgt, cells):
    """bool [M]: the oracle's win test on the given cells."""
    return _batch(orc, S, mc, blk, tgt, cells).won().astype(bool)


def expand(orc, S, mc, blk, tgt, cells, depth):
    """The frontier of every ply 1 .. depth: a list of dicts (cells [T, 4^p M], won bool [4^p M], invalid bool [4^p M]).  Board
    (seq, m) of ply p - the action sequence seq = a_1 4^(p-1) + ... + a_p played on sample m - stands at column seq M + m."""
    M = cells.shape[1]
    plies, cur = [], np.ascontiguousarray(cells)
    for p in range(1, depth + 1):
        n = cur.shape[1]  # 4^(p-1) M, parent-major
        reps = n // M
        out_cells = np.empty((cells.shape[0], 4 * n), cells.dtype)
        won, invalid = np.empty(4 * n, bool), np.empty(4 * n, bool)
        lv_blk, lv_tgt = np.tile(blk, (1, reps)), np.tile(tgt, (1, reps))
        # child (parent seq, a) stands at seq' = 4 seq + a: view the columns as [parents, 4, M]
        oc = out_cells.reshape(cells.shape[0], reps, 4, M)
        wv, iv = won.reshape(reps, 4, M), invalid.reshape(reps, 4, M)
        for a in range(4):
            b = _batch(orc, S, mc, lv_blk, lv_tgt, cur)
            b.done[...] = 0
            b.step_count[...] = 0
            f = b.step(np.full(n, a, np.uint8), obs=False)["flags"]
            assert not (f & ~np.uint8(FLAG_IS_WON | FLAG_INVALID_MOVE | 0x04)).any()
            oc[:, :, a, :] = b.pos.reshape(cells.shape[0], reps, M)
            wv[:, a, :] = ((f & FLAG_IS_WON) != 0).reshape(reps, M)
            iv[:, a, :] = ((f & FLAG_INVALID_MOVE) != 0).reshape(reps, M)
        plies.append({"cells": out_cells, "won": won, "invalid": invalid})
        cur = out_cells
    return plies


def planes(orc, S, mc, blk, tgt, cells):
    """float32 [n, D]: the oracle's one-hot planes of the given boards."""
    b = _batch(orc, S, mc, blk, tgt, cells)
    return b.encode_onehot().reshape(b.n, -1)


def leaf_values64(x, leaf, mlp, head):
    """(X, BX) float64 [n] of planes x [n, D]."""
    if leaf == LEAF_VALUE:
        _, _, v, vb = aref.outputs64(x, mlp, head)
        return v, vb
    z, zb = pref.logits64(x, mlp)
    return z.max(axis=1), zb.max(axis=1)


def leaves(orc, S, mc, blk, tgt, ply, M, leaf, mlp=None, head=None, evaluate=None):
    """(X, BX) of every board of the last ply, evaluated in chunks; `evaluate(x) -> (X, BX)` replaces leaf_values64."""
    n = ply["cells"].shape[1]
    X, BX = np.zeros(n), np.zeros(n)
    if leaf == LEAF_ZERO:
        return X, BX
    evaluate = evaluate or (lambda x: leaf_values64(x, leaf, mlp, head))
    col = np.arange(n) % M   # the sample, hence the level, of a column
    for lo in range(0, n, CHUNK):
        sl = slice(lo, min(n, lo + CHUNK))
        x = planes(orc, S, mc, np.ascontiguousarray(blk[:, col[sl]]), np.ascontiguousarray(tgt[:, col[sl]]), ply["cells"][:, sl])
        X[sl], BX[sl] = evaluate(x)
    return X, BX


def backup(plies, won0, X, BX, gamma, w, M):
    """(q [M, 4], qbound [M, 4], win_in uint8 [M]) from the leaf values of the last ply; gamma and w = (w_step, w_win, w_invalid)
    are read as the float32 values the library is given."""
    g = float(np.float32(gamma))
    ws, ww, wi = (float(np.float32(v)) for v in w)
    below = np.zeros(X.shape[0], np.int64)
    for ply in reversed(plies):
        won, inv = ply["won"], ply["invalid"]
        x, bx = np.where(won, 0.0, X), np.where(won, 0.0, BX)
        q = ws + ww * won + wi * inv + g * x
        qb = g * bx + gamma_n(4) * (abs(ws) + abs(ww) * won + abs(wi) * inv + g * (np.abs(x) + bx))
        win = np.where(won, 1, np.where(below > 0, below + 1, 0))
        parents = q.shape[0] // (4 * M)
        q4, qb4, win4 = q.reshape(parents, 4, M), qb.reshape(parents, 4, M), win.reshape(parents, 4, M)
        X, BX = q4.max(axis=1).reshape(-1), qb4.max(axis=1).reshape(-1)
        below = np.where(win4 > 0, win4, 1 << 20).min(axis=1).reshape(-1)
        below = np.where(below == 1 << 20, 0, below)
    q, qb = q4[0].T.copy(), qb4[0].T.copy()   # the root: parents == 1
    q[won0], qb[won0] = 0.0, 0.0
    return q, qb, np.where(won0, 0, below).astype(np.uint8)


def search(orc, S, mc, blk, tgt, cells, depth, leaf, gamma, w, mlp=None, head=None, plies=None):
    """The definition on M samples (levels blk [W, M], tgt [Tt, M], cells [T, M]): a dict of q, qbound float64 [M, 4], value
    float64 [M], best uint8 [M] (of the float64 q: meaningful where the arithmetic is exact), win_in uint8 [M], won0 and
    invalid0 bool [M] / [M, 4] - what the root saw.  `plies`: expand() of the same samples to this depth or deeper, computed once
    by a caller that searches them several times."""
    M = cells.shape[1]
    won0 = won_on(orc, S, mc, blk, tgt, cells)
    plies = expand(orc, S, mc, blk, tgt, cells, depth) if plies is None else plies[:depth]
    X, BX = leaves(orc, S, mc, blk, tgt, plies[-1], M, leaf, mlp, head)
    q, qb, win_in = backup(plies, won0, X, BX, gamma, w, M)
    best = np.where(won0, NO_ACTION, np.argmax(q == q.max(axis=1, keepdims=True), axis=1)).astype(np.uint8)
    return {"q": q, "qbound": qb, "value": q.max(axis=1), "best": best, "win_in": win_in, "won0": won0,
            "invalid0": plies[0]["invalid"].reshape(4, M).T.copy(), "plies": plies}


def trajectory(orc, S, mc, blk, tgt, first, pos_log, depth, leaf, gamma, w, mlp=None, head=None):
    """search() on the K N samples of a logged trajectory (c[0] = first, c[k] = pos_log[k - 1]), results reshaped to [K, N, ...]."""
    K, N = pos_log.shape[0], first.shape[1]
    cells = np.concatenate([first[None], pos_log[:K - 1]], axis=0)                  # [K, T, N]
    flat = np.ascontiguousarray(cells.transpose(1, 0, 2).reshape(first.shape[0], K * N))
    got = search(orc, S, mc, np.tile(blk, (1, K)), np.tile(tgt, (1, K)), flat, depth, leaf, gamma, w, mlp, head)
    return {k: v.reshape((K, N) + v.shape[1:]) for k, v in got.items() if k != "plies"}


# ---------------------------------------------------------------------------------------------- the inputs of the GPU tests
def near_win_levels(orc, S, T, K, n, mc, Tt=None, seed=0x100CA4EAD):
    """(blk, init, tgt) of n levels of generate_mt19937 whose targets are overwritten by the cells the tiles reach after 1 + n % 4
    seeded moves (fill_actions) from the start: every board is at most four moves from a win by construction.  Three boards of
    every second group of four start behind the first of those moves (one move nearer; the move repeated changes nothing, which
    gives the dense 8x8 / 8 boards an invalid root move too).  With Tt > T the extra targets repeat the last tile's cell (single
    colour: a set, so the board can still be won)."""
    Tt = T if Tt is None else Tt
    seeds = np.arange(n, dtype=np.uint32) + np.uint32(seed & 0xffff)
    if S == 1:   # one cell: whatever there is stands on it
        return np.zeros((1, n), np.uint32), np.zeros((T, n), np.uint8), np.zeros((Tt, n), np.uint8)
    if T == 0:   # no tiles: a drawn level's obstacles and targets
        blk, init, tgt = orc.generate_mt19937(S, 1, max(Tt, 1), K, seeds)
        return blk, np.ascontiguousarray(init[:0]), np.ascontiguousarray(tgt[:Tt])
    blk, init, tgt = orc.generate_mt19937(S, T, Tt, K, seeds)
    tgt = tgt.copy()
    b = _batch(orc, S, mc, blk, tgt, init)
    init = init.copy()
    moves = 1 + np.arange(n) % 4
    for j in range(4):
        before = b.pos.copy()
        b.done[...] = 0
        b.step_count[...] = 0
        b.step(orc.fill_actions(n, seed, j), obs=False)
        b.pos[...] = np.where(j < moves, b.pos, before)
        if j == 0:   # every other group of four starts behind its first move where more follow: repeating that move is invalid
            init[...] = np.where((moves >= 2) & ((np.arange(n) // 4) % 2 == 1), b.pos, init)
    for t in range(Tt):
        tgt[t] = b.pos[min(t, T - 1)]
    return blk, init, tgt


def conditions(ref):
    """The shares the GPU tests rely on, of one search() result: a win inside the horizon, each action the best (among the boards
    not won on entry), an invalid root move, a board won on entry."""
    alive = ~ref["won0"].reshape(-1)
    best = ref["best"].reshape(-1)[alive]
    return {"win": float((ref["win_in"].reshape(-1) > 0).mean()),
            "best": [float((best == a).mean()) if best.size else 0.0 for a in range(4)],
            "invalid": float(ref["invalid0"].reshape(-1, 4)[alive].any(axis=1).mean()) if alive.any() else 0.0,
            "won0": float((~alive).mean())}


def int_network(rng, D, H):
    """(mlp, head) of integers: the weights in [-4, 4] (policy_reference.random_mlp "int"), the head in [-2, 2]."""
    return pref.random_mlp(rng, D, H, "int"), aref.int_head(rng, H)


def features(S, T, Tt, mc):
    return (1 + T + Tt if mc else 3) * S * S
