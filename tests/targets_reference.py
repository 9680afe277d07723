"""CPU yardstick of the trajectory targets (test infrastructure, no test of its own): the definitions of
include/tiler_slider_targets.h restated on NumPy and the CPU oracle.  The trajectories are those of rollout_reference.rollout /
policy_reference.rollout; m() is restated on NumPy (and held to OracleBatch.step(reward=True) by sum_k m(pos_log[k]) ==
reward_sum); the recursion runs in float64; labels are table_reference.lookup applied to c[k], step by step.  It shares no code
with tiler_slider_amd/csrc/ts_targets.hip.  Imports neither torch nor the libraries at import time.

THE BOUND of the returns: |got - ref| <= gamma(3 (K - k) + 10) * Abar_k with gamma(n) = n u / (1 - n u), u = 2**-24
(policy_reference.gamma), and Abar_k the same recursion on absolute values:
    Abar_k = |r-terms| + gamma |V+| + |V| + gamma lambda Abar+
Derived, not measured: a float32 evaluation in any order, with or without fused multiply-adds, multiplies every term of the
real-arithmetic expansion of A_k (or ret_k) by a product of (1 + d), |d| <= u, one per rounding on the term's path (Higham,
section 3.1).  A term that enters at step j passes at most 10 roundings at its own step (six additions of the reward's terms
after its own product, the product and the addition of gamma V+, the subtraction of V, the addition of the carry; ret's V_k
passes one) and at most 3 per step on its way down to k (the rounding of gamma * lambda, the product with the carry, the
addition), and one more for ret = A + V: 3 (j - k) + 10 <= 3 (K - k) + 10 in all.
"""
from collections import namedtuple

import numpy as np

import policy_reference as pref
import rollout_reference as rref
import table_reference as tref

FLAG_IS_WON, FLAG_INVALID_MOVE = 0x01, 0x02
FLAG_SUCCESS, FLAG_TIMEOUT, FLAG_STEPPED_DONE, FLAG_AUTORESET, FLAG_BAD_ACTION = 0x04, 0x08, 0x10, 0x20, 0x40
VOID, END = FLAG_STEPPED_DONE | FLAG_AUTORESET | FLAG_BAD_ACTION, FLAG_SUCCESS | FLAG_TIMEOUT

Weights = namedtuple("Weights", ("step", "win", "timeout", "invalid", "dist", "progress"), defaults=(0.0, 1.0, 0.0, 0.0, 0.0, 0.0))


def m_of(S, mc, cells, tgt):
    """int64 [N]: the Manhattan reward of ts_reward (include/tiler_slider.h) on cells [T, N] and targets [Tt, N], ids clipped to
    S * S - 1.  Multi colour: minus the distances of tile t to target t over the first min(T, Tt); single colour: minus, over the
    tiles, the distance to the nearest target (0 without targets)."""
    c = np.minimum(np.asarray(cells).astype(np.int64), S * S - 1)
    g = np.minimum(np.asarray(tgt).astype(np.int64), S * S - 1)
    T, Tt, N = c.shape[0], g.shape[0], c.shape[1]
    total = np.zeros(N, np.int64)
    if mc:
        for t in range(min(T, Tt)):
            total += np.abs(c[t] // S - g[t] // S) + np.abs(c[t] % S - g[t] % S)
    elif Tt > 0:
        for t in range(T):
            d = np.abs(c[t][None] // S - g // S) + np.abs(c[t][None] % S - g % S)   # [Tt, N]
            total += d.min(axis=0)
    return -total


def cells_of(first, pos_log, k):
    """c[k]: `first`, then the row below in the log."""
    return first if k == 0 else pos_log[k - 1]


def m_logs(S, mc, first, pos_log, tgt):
    """(m_before, m_after) int64 [K, N]: m(c[k]) and m(pos_log[k])."""
    K = pos_log.shape[0]
    after = np.stack([m_of(S, mc, pos_log[k], tgt) for k in range(K)])
    before = np.stack([m_of(S, mc, cells_of(first, pos_log, k), tgt) for k in range(K)])
    return before, after


def _recursion(flags_log, m_before, m_after, values, last_value, gamma, lam, w, dtype, exact=False, ignore_ends=False, gamma_for_gl=False):
    """The definition in `dtype`.  exact: every intermediate is asserted to survive a round trip through float32.  The two wrong
    variants exist for the CPU test that shows the bound notices them."""
    f = np.asarray(flags_log)
    K, N = f.shape
    t = dtype
    w = Weights(*(t(x) for x in w))
    g = t(gamma)
    gl = g if gamma_for_gl else t(g * t(lam))
    V = np.zeros((K, N), t) if values is None else np.asarray(values).astype(t)
    VL = np.zeros(N, t) if last_value is None else np.asarray(last_value).astype(t)
    mb, ma = np.asarray(m_before).astype(t), np.asarray(m_after).astype(t)
    out = {k: np.zeros((K, N), t) for k in ("reward", "adv", "ret", "abar")}
    out["mask"] = np.zeros((K, N), np.uint8)
    carry, abar = np.zeros(N, t), np.zeros(N, np.float64)

    def keep(x):
        if exact:
            assert np.array_equal(np.asarray(x, np.float32).astype(np.float64), np.asarray(x, np.float64)), "an intermediate is not a float32"
        return x

    for k in range(K - 1, -1, -1):
        void = (f[k] & VOID) != 0
        end = np.zeros(N, bool) if ignore_ends else (f[k] & END) != 0
        flag = lambda bit: ((f[k] & bit) != 0).astype(t)
        terms = (np.broadcast_to(w.step, (N,)), w.win * flag(FLAG_SUCCESS), w.timeout * flag(FLAG_TIMEOUT), w.invalid * flag(FLAG_INVALID_MOVE),
                 keep(w.dist * ma[k]), keep(w.progress * keep(ma[k] - mb[k])))
        r = np.zeros(N, t)
        for term in terms:
            r = keep((r + term).astype(t))
        vplus = np.where(end, t(0), VL if k == K - 1 else V[k + 1])
        delta = keep((keep((r + keep(g * vplus)).astype(t)) - V[k]).astype(t))
        a = keep((delta + np.where(end, t(0), keep(gl * carry))).astype(t))
        ab = sum(np.abs(x.astype(np.float64)) for x in terms) + float(gamma) * np.abs(vplus.astype(np.float64)) + np.abs(V[k].astype(np.float64)) \
            + np.where(end, 0.0, float(gamma) * float(lam) * abar)
        live = ~void
        carry = np.where(live, a, carry).astype(t)
        abar = np.where(live, ab, abar)
        out["reward"][k] = np.where(live, r, t(0))
        out["adv"][k] = np.where(live, a, t(0))
        out["ret"][k] = np.where(live, keep((a + V[k]).astype(t)), t(0))
        out["abar"][k] = np.where(live, ab, 0.0)
        out["mask"][k] = live
    return out


def returns64(flags_log, m_before, m_after, values, last_value, gamma, lam, w, exact=False):
    """dict reward, adv, ret float64 [K, N], mask uint8 [K, N] and bound float64 [K, N] (0 on void steps: they must be exactly 0)."""
    out = _recursion(flags_log, m_before, m_after, values, last_value, gamma, lam, w, np.float64, exact=exact)
    K = out["adv"].shape[0]
    out["bound"] = pref.gamma(3.0 * (K - np.arange(K)) + 10.0)[:, None] * out.pop("abar")
    return out


def returns32(flags_log, m_before, m_after, values, last_value, gamma, lam, w, **wrong):
    """A float32 NumPy evaluation, term by term (no fused multiply-add); wrong: ignore_ends=True or gamma_for_gl=True."""
    out = _recursion(flags_log, m_before, m_after, values, last_value, gamma, lam, w, np.float32, **wrong)
    out.pop("abar")
    return out


def labels(orc, S, blk, first, pos_log, table, rows=None):
    """(moves int16, best uint8, action uint8) [K, N]: table_reference.lookup on c[k], step by step."""
    got = [tref.lookup(orc, S, blk, cells_of(first, pos_log, k), table, rows) for k in range(pos_log.shape[0])]
    return tuple(np.stack([g[i] for g in got]) for i in range(3))


# name -> (S, T, obstacles, multi colour, boards, level seed, policy, epsilon, rollout seed, mode, K, max_steps): the trajectories of
# tests/test_targets_cpu.py and tests/test_gpu_targets.py.  "given": 5 % of the action bytes are above 3 (BAD_ACTION).
CASES = {"auto": (4, 2, 2, False, 257, 11, rref.TABLE, 0.3, 5, 1, 24, 6),
         "long": (4, 2, 2, False, 257, 11, rref.TABLE, 0.3, 5, 1, 200, 20),
         "strict": (4, 2, 2, False, 257, 11, rref.TABLE, 0.3, 5, 0, 24, 6),
         "given": (4, 2, 2, False, 257, 11, rref.GIVEN, 0.0, 5, 1, 24, 6),
         "mc5": (5, 3, 3, True, 257, 12, rref.TABLE, 0.3, 6, 1, 5, 4),
         "s8": (8, 2, 10, False, 257, 13, rref.TABLE, 0.3, 7, 1, 24, 12)}

_cache = {}


def given_actions(n, K, seed):
    """uint8 [K, n]: uniform moves, 5 % of them replaced by bytes above 3."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (K, n)).astype(np.uint8)
    bad = rng.random((K, n)) < 0.05
    return np.where(bad, rng.integers(4, 256, (K, n)).astype(np.uint8), a).astype(np.uint8)


def trajectory(orc, name):
    """dict of one case, computed once and shared (nobody writes into it): the level (blk, init, tgt), its table, the yardstick's
    rollout `log` (rollout_reference.rollout's dict), first = the cells before step 0, and m_before / m_after."""
    if name in _cache:
        return _cache[name]
    S, T, obstacles, mc, n, lseed, policy, eps, rseed, mode, K, max_steps = CASES[name]
    blk, init, tgt = orc.generate(S, T, T, obstacles, n, seed=lseed)
    table = tref.table(orc, S, mc, blk, tgt, T)
    actions = given_actions(n, K, rseed) if policy == rref.GIVEN else None
    log = rref.rollout(orc, S, mc, max_steps, blk, init, tgt, K, policy, mode, actions=actions, table=table, threshold=rref.threshold_of(eps), seed=rseed)
    first = init.copy()   # a freshly reset board stands on its initial cells
    mb, ma = m_logs(S, mc, first, log["pos_log"], tgt)
    assert np.array_equal(ma.sum(axis=0), log["reward_sum"]), "the restated m() is not the oracle's reward"
    case = dict(S=S, T=T, mc=mc, n=n, K=K, max_steps=max_steps, mode=mode, policy=policy, eps=eps, seed=rseed, blk=blk, init=init, tgt=tgt,
                table=table, actions=actions, log=log, first=first, m_before=mb, m_after=ma)
    for v in (blk, init, tgt, table, first, mb, ma, log["pos_log"], log["flags_log"], log["act_log"]):
        v.setflags(write=False)
    _cache[name] = case
    return case


def share(flags_log, bits):
    return float(((np.asarray(flags_log) & bits) != 0).mean())


def gaussian_values(K, n, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((K, n)).astype(np.float32), rng.standard_normal(n).astype(np.float32)


def integer_values(K, n, seed=4):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, (K, n)).astype(np.float32), rng.integers(-8, 9, n).astype(np.float32)


INT_WEIGHTS = Weights(step=-1, win=5, timeout=-3, invalid=-2, dist=1, progress=2)

# kernel name -> (S, T, obstacles): one case per kernel of the targets library, the shapes of the rollout library's occupancy
# cases; tests/test_targets_cpu.py pins the names to the code object
_OCC_SHAPES = {1: (1, 0), 2: (2, 1), 3: (2, 1), 4: (2, 2), 5: (2, 3), 6: (2, 6), 7: (2, 8), 8: (2, 10)}
OCCUPANCY_CASES = {f"{stem}<{S}>": (S, T, K) for S, (T, K) in _OCC_SHAPES.items() for stem in ("k_traj_returns", "k_traj_labels")}


def occupancy_levels(orc, S, T, K_obstacles, n, seed):
    """(blk, init, tgt) of n random levels; where tiles, targets and obstacles do not all fit on distinct cells (1x1, 2x2 with two
    tiles and an obstacle) the targets are drawn on their own and may lie under tiles or obstacles."""
    if 2 * T + K_obstacles > S * S:
        blk, init, _ = orc.generate(S, T, 0, K_obstacles, n, seed=seed)
        _, _, tgt = orc.generate(S, 0, T, 0, n, seed=seed + 1)
        return blk, init, tgt
    return orc.generate(S, T, T, K_obstacles, n, seed=seed)
