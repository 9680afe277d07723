"""CPU yardstick of the neural-policy rollouts (test infrastructure, no test of its own): the definition of
include/tiler_slider_policy.h restated on NumPy and the CPU oracle.  The network's input is `OracleBatch.encode_onehot()`, the
logits are computed in float64 together with a rigorous bound on the error of ANY float32 evaluation, the selection rule is
restated on given logits, and the free-running loop steps the oracle as tests/rollout_reference.py does.  It shares no code with
tiler_slider_amd/csrc/ts_policy.hip.  Imports neither torch nor the libraries at import time.

The bound (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: a sum or inner product of n terms evaluated in
any order, with or without fused multiply-adds, has relative backward error gamma_n per term), with u = 2**-24 and
gamma_n = n u / (1 - n u):  the first layer adds m + 1 terms (the bias and the rows of the m ones of x, no product), so the
computed pre-activation differs from the exact one by at most e_j = gamma_{m+1} (|b1_j| + sum_active |w1[f][j]|); ReLU is
1-Lipschitz and exact; the second layer is an inner product of H + 1 terms on the perturbed h:
    bound_a = sum_j e_j |w2[j][a]| + gamma_{H+1} (|b2_a| + sum_j (|h_j| + e_j) |w2[j][a]|)."""
import numpy as np

import rollout_reference as rref

GREEDY, SAMPLE = 0, 1
U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def random_mlp(rng, D, H, kind="gauss"):
    """(w1 [H, D], b1 [H], w2 [4, H], b2 [4]) float32 in torch.nn.Linear's layout; kind "int": integers in [-4, 4] (every partial
    sum is an integer far below 2**24: float32 is exact in any order)."""
    if kind in ("int", "int128"):
        draw = lambda *s: rng.integers(-4, 5, s).astype(np.float32)
    else:
        draw = lambda *s: rng.standard_normal(s).astype(np.float32)
    w1, b1, w2, b2 = draw(H, D), draw(H), draw(4, H), draw(4)
    if kind == "int128":   # logits that are multiples of 128: exp(z - max z) is exactly 0 or 1 in float32, so SAMPLE is exact too
        w2, b2 = w2 * np.float32(128), b2 * np.float32(128)
    return w1, b1, w2, b2


def logits_exact32(x, mlp):
    """float32 logits of an integer-weight network on x [n, D]: every partial sum is an integer below 2**24, so this is the exact
    value whatever order the matrix products sum in.  (The yardstick of the large exact cases: no float64 copy of x.)"""
    w1, b1, w2, b2 = mlp
    assert all((a == np.round(a)).all() for a in mlp)
    z = np.maximum(x @ w1.T + b1, np.float32(0)) @ w2.T + b2
    assert z.dtype == np.float32 and np.abs(z).max(initial=0) < 2 ** 24
    return z


def logits64(x, mlp):
    """(z float64 [n, 4], bound float64 [n, 4]) for x [n, D] of zeros and ones."""
    w1, b1, w2, b2 = (np.asarray(a, np.float64) for a in mlp)
    x = np.asarray(x, np.float64)
    H = w1.shape[0]
    m = x.sum(axis=1, keepdims=True)
    pre = x @ w1.T + b1
    h = np.maximum(pre, 0.0)
    z = h @ w2.T + b2
    e = gamma(m + 1) * (np.abs(b1)[None, :] + x @ np.abs(w1).T)
    bound = e @ np.abs(w2).T + gamma(H + 1) * (np.abs(b2)[None, :] + (np.abs(h) + e) @ np.abs(w2).T)
    return z, bound


def board_logits(b, mlp):
    """logits64 on the oracle batch as it stands."""
    return logits64(b.encode_onehot().reshape(b.n, -1), mlp)


def uniforms(r):
    """u of the definition: bits 32 .. 55 of the draw, times 2**-24 (exact in float32 and float64)."""
    return ((r >> np.uint64(32)) & np.uint64(0xffffff)).astype(np.float64) * U


def select(z, r, mode):
    """e of the definition on the logits z [n, 4] as given (float32 or float64: the arithmetic is done in z's precision)."""
    z = np.asarray(z)
    if mode == GREEDY:
        return np.argmax(z == z.max(axis=1, keepdims=True), axis=1).astype(np.uint8)
    w = np.exp(z - z.max(axis=1, keepdims=True))
    c = np.cumsum(w, axis=1)
    x = uniforms(r).astype(z.dtype) * c[:, 3]
    return np.minimum((x[:, None] >= c).sum(axis=1), 3).astype(np.uint8)


def sample_margin(z32, r):
    """SAMPLE: the distance of u from the nearest boundary of the normalised CDF computed in float64 from the logged logits."""
    z = np.asarray(z32, np.float64)
    w = np.exp(z - z.max(axis=1, keepdims=True))
    cdf = np.cumsum(w, axis=1)[:, :3] / w.sum(axis=1, keepdims=True)
    return np.abs(uniforms(r)[:, None] - cdf).min(axis=1)


def choose(z, r, mode, threshold):
    """(a, explore) of the definition."""
    e = select(z, r, mode)
    explore = (r & np.uint64(0xffffffff)) < np.uint64(threshold)
    return np.where(explore, (r >> np.uint64(62)).astype(np.uint8), e).astype(np.uint8), explore


def rollout(orc, S, mc, max_steps, blk, init, tgt, mlp, steps, select_mode, mode=0, *, pos=None, step_count=None, done=None, threshold=0,
            seed=0, step_index=0, board_offset=0, exact32=False):
    """The free-running loop with the logits taken in float32 from the float64 values (exact for integer weights), from the state
    (pos, step_count, done) - default: freshly reset; exact32: logits_exact32 instead.  Returns the nine outputs, logits_log, the state after the loop and what the
    run exercised: per-board `won`, `timed_out`, `reset`; `explored` and `ties` board-steps; `action_share` [4]."""
    b = orc.OracleBatch(S, mc, max_steps, blk, init, tgt)
    n, T = b.n, b.n_tiles
    if pos is not None:
        b.pos[...] = pos
    if step_count is not None:
        b.step_count[...] = step_count
    if done is not None:
        b.done[...] = done
    out = {k: np.zeros(n, np.int32) for k in ("wins", "finished", "first_win", "win_moves", "reward_sum")}
    out["flags"] = np.zeros(n, np.uint8)
    out["act_log"], out["flags_log"] = np.zeros((steps, n), np.uint8), np.zeros((steps, n), np.uint8)
    out["pos_log"] = np.zeros((steps, T, n), b.pos.dtype)
    out["logits_log"] = np.zeros((steps, n, 4), np.float32)
    explored = ties = 0
    for k in range(steps):
        r = rref.draws(n, seed, step_index + k, board_offset)
        z = logits_exact32(b.encode_onehot().reshape(n, -1), mlp) if exact32 else board_logits(b, mlp)[0].astype(np.float32)
        a, explore = choose(z, r, select_mode, threshold)
        explored += int(explore.sum())
        ties += int(((z == z.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        res = b.step(a, mode=mode, obs=False, reward=True)
        f = res["flags"]
        success = (f & rref.FLAG_SUCCESS) != 0
        out["wins"] += success
        out["finished"] += (f & (rref.FLAG_SUCCESS | rref.FLAG_TIMEOUT)) != 0
        out["first_win"] = np.where(success & (out["first_win"] == 0), k + 1, out["first_win"]).astype(np.int32)
        out["win_moves"] += np.where(success, b.step_count, 0).astype(np.int32)
        out["reward_sum"] += res["reward"]
        out["flags"] = f.copy()
        out["act_log"][k], out["flags_log"][k], out["pos_log"][k], out["logits_log"][k] = a, f, b.pos, z
    out["pos"], out["step_count"], out["done"] = b.pos.copy(), b.step_count.copy(), b.done.copy()
    out["won"] = out["wins"] > 0
    out["timed_out"] = ((out["flags_log"] & rref.FLAG_TIMEOUT) != 0).any(axis=0) if steps else np.zeros(n, bool)
    out["reset"] = ((out["flags_log"] & rref.FLAG_AUTORESET) != 0).any(axis=0) if steps else np.zeros(n, bool)
    out["explored"], out["ties"] = explored, ties
    out["action_share"] = np.bincount(out["act_log"].ravel(), minlength=4)[:4] / float(max(1, n * steps))
    return out


OUTPUTS = rref.OUTPUTS + ("logits_log",)

# (S, T, obstacles, multi colour, boards, max_steps, steps, epsilon, H, mode, seed): the exact, free-running cases of
# tests/test_gpu_policy.py - integer weights, GREEDY; the seeds were chosen with exact_case() on the CPU so that every assertion
# of it holds on the yardstick's own numbers
EXACT_CASES = ((4, 2, 2, False, 3000, 6, 40, 0.0, 16, 1, 1),
               (4, 2, 2, True, 3000, 10, 40, 0.25, 7, 1, 1),
               (5, 3, 3, True, 2000, 12, 40, 0.25, 12, 1, 0),
               (8, 2, 10, False, 1000, 8, 30, 0.0, 16, 1, 14),
               (4, 2, 2, False, 3000, 6, 40, 0.25, 16, 0, 0))


def exact_case(orc, case):
    """Levels, network and the yardstick's answer of one exact case, with the assertions that keep it from passing on idle boards."""
    S, T, K, mc, n, max_steps, steps, eps, H, mode, seed = EXACT_CASES[case]
    blk, init, tgt = orc.generate_mt19937(S, T, T, K, np.arange(n, dtype=np.uint32))
    D = (1 + 2 * T if mc else 3) * S * S
    mlp = random_mlp(np.random.default_rng(1000 * case + seed), D, H, "int")
    want = rollout(orc, S, mc, max_steps, blk, init, tgt, mlp, steps, GREEDY, mode, threshold=rref.threshold_of(eps),
                   seed=0x9011C7 + case, step_index=case * 100, board_offset=case * 31)
    total = float(n * steps)
    print(f"exact case {case}: boards winning {want['won'].mean():.3f}, timing out {want['timed_out'].mean():.3f}, resetting "
          f"{want['reset'].mean():.3f}; action shares {want['action_share'].round(3).tolist()}, explored {want['explored'] / total:.3f}, "
          f"ties {want['ties'] / total:.3f}")
    assert want["won"].any() and want["timed_out"].any()
    if mode == 1:
        assert want["reset"].any()
    else:
        assert ((want["flags_log"] & rref.FLAG_STEPPED_DONE) != 0).any()
    assert (want["action_share"] >= 0.01).all(), want["action_share"]
    assert want["ties"] >= 0.01 * total
    if eps > 0:
        assert want["explored"] >= 0.01 * total
    return (blk, init, tgt), mlp, want


# kernel name -> (S, T, obstacles, select or None for the logits kernel): one case per kernel of the policy library
_OCC_SHAPES = {1: (1, 0), 2: (2, 1), 3: (2, 1), 4: (2, 2), 5: (2, 3), 6: (2, 6), 7: (2, 8), 8: (2, 10)}
OCCUPANCY_CASES = {f"k_policy_rollout<{S}, {sel}>": (S, T, K, sel) for S, (T, K) in _OCC_SHAPES.items() for sel in (GREEDY, SAMPLE)}
OCCUPANCY_CASES.update({f"k_policy_logits<{S}>": (S, T, K, None) for S, (T, K) in _OCC_SHAPES.items()})
