"""CPU yardstick of the trainable policies (test infrastructure, no test of its own): the definition of
include/tiler_slider_train.h restated on NumPy.  Only the cell source changes from tests/policy_reference.py: every sample's x is
that board's one-hot features, built here with NumPy from the cells (and held to OracleBatch.encode_onehot() by
tests/test_train_cpu.py).  Logits in float64 with policy_reference's per-logit bound; gradients in float64 by the closed form of
the header, with a per-entry bound that holds for ANY float32 evaluation.  It shares no code with tiler_slider_amd/csrc/ts_train.hip
and imports neither torch nor the libraries at import time.  Networks are in torch.nn.Linear's layout as in policy_reference
(w1 [H, D], b1 [H], w2 [4, H], b2 [4]); gradients come back in the KERNEL layout ([D, H], [H], [H, 4], [4]).

THE GRADIENT BOUND (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1 and 4.2: a sum or inner product of n
terms, in any order or tree, with or without fused multiply-adds, has error at most gamma_n sum |terms| - gamma_{n-1} for a plain
sum; u = 2**-24, gamma_n = n u / (1 - n u)).  Hats are computed float32 values.  For sample i and unit j:
  * |pre^ - pre| <= e = gamma_{m+1} (|b1_j| + sum_active |w1[f][j]|), policy_reference's bound; h = max(pre, 0) is 1-Lipschitz
    and exact, so |h^ - h| <= e and |h^| <= |h| + e.
  * dh^ is an inner product of four exact terms: |dh^ - dh| <= d = gamma_4 sum_a |w2[j][a]| |dz_a|, and |dh^| <= |dh| + d.
  * dp^ = (pre^ > 0) ? dh^ : 0.  Where |pre| > e the computed sign is the true one and |dp^ - dp| <= d.  Where |pre| <= e - an
    AMBIGUOUS pair - the kernel may take either side of the ReLU: |dp^ - dp| <= |dh| + d.  Either way |dp^| <= |dh| + d.
  * gb2_a sums M exact terms:                   |err| <= gamma_M sum |dz_a|
  * gw2[j][a] is an inner product of M terms on the perturbed h:
                                                |err| <= sum e |dz_a| + gamma_{M+1} sum (|h| + e) |dz_a|
  * gb1_j and gw1[f][j] sum the M perturbed dp^ of the samples that have the feature (all of them for b1), in any tree - the
    kernel's per-board partial sums, LDS accumulators and atomic flushes are one such tree:
                                                |err| <= sum (d + [ambiguous] |dh|) + gamma_M sum (|dh| + d)
M counts every sample that has the feature, zeros included (adding an exact zero is exact, so this only loosens the bound).  The
bound is for sums that start from zero: a prefilled buffer adds one more term, which the exact tests cover instead."""
import numpy as np

import policy_reference as pref

U = pref.U
gamma = pref.gamma


def features(S, T, Tt, mc):
    return (1 + T + Tt if mc else 3) * S * S


def int_mlp(rng, D, H, lo=-2, hi=2):
    """Integer weights in [lo, hi] in torch.nn.Linear's layout."""
    draw = lambda *s: rng.integers(lo, hi + 1, s).astype(np.float32)
    return draw(H, D), draw(H), draw(4, H), draw(4)


def kernel_layout(mlp):
    w1, b1, w2, b2 = mlp
    return np.ascontiguousarray(w1.T), np.ascontiguousarray(b1), np.ascontiguousarray(w2.T), np.ascontiguousarray(b2)


def onehot(S, mc, blk, cells, tgt, sets=True):
    """x float32 [n, D] of n boards: blk uint32 [words, n], cells [T, n] and tgt [Tt, n] raw cell ids (clamped here to S*S - 1).
    sets=False drops the counts-once rule of single colour (a shared cell then counts twice): only for the self-check that the
    exact comparison notices."""
    C = S * S
    T, n = cells.shape
    Tt = tgt.shape[0]
    cells = np.minimum(cells.astype(np.int64), C - 1)
    tgt = np.minimum(tgt.astype(np.int64), C - 1)
    planes = 1 + T + Tt if mc else 3
    x = np.zeros((n, planes, C), np.float32)
    bits = np.zeros(n, np.uint64)
    for w in range(blk.shape[0]):
        bits |= blk[w].astype(np.uint64) << np.uint64(32 * w)
    for p in range(C):
        x[:, 0, p] = ((bits >> np.uint64(p)) & np.uint64(1)).astype(np.float32)
    rows = np.arange(n)
    for t in range(T):
        np.add.at(x, (rows, 1 + t if mc else 1, cells[t]), 1.0)
    for j in range(Tt):
        np.add.at(x, (rows, 1 + T + j if mc else 2, tgt[j]), 1.0)
    if sets:
        x = np.minimum(x, np.float32(1))
    return x.reshape(n, planes * C)


def sample_cells(first, pos_log, K):
    """c [K, T, N] of the header: c[0] = first, c[k] = pos_log[k - 1]."""
    c = np.empty((K,) + first.shape, first.dtype)
    c[0] = first
    if K > 1:
        c[1:] = pos_log[:K - 1]
    return c


def samples_onehot(S, mc, blk, first, pos_log, tgt, K, sets=True):
    """x [K * N, D], sample (k, n) at row k * N + n."""
    c = sample_cells(first, pos_log, K)
    return np.concatenate([onehot(S, mc, blk, c[k], tgt, sets) for k in range(K)], axis=0)


def shared_cell_share(first, pos_log, K, C):
    """The share of samples in which two tiles lie on one (clamped) cell."""
    c = np.minimum(sample_cells(first, pos_log, K).astype(np.int64), C - 1)
    T = c.shape[1]
    if T < 2:
        return 0.0
    s = np.sort(c, axis=1)
    return float((s[:, 1:] == s[:, :-1]).any(axis=1).mean())


def forward64(x, mlp):
    """(pre, h, z, e) in float64: e [M, H] bounds the error of a float32 pre-activation."""
    w1, b1, w2, b2 = (np.asarray(a, np.float64) for a in mlp)
    x = np.asarray(x, np.float64)
    pre = x @ w1.T + b1
    h = np.maximum(pre, 0.0)
    z = h @ w2.T + b2
    m = x.sum(axis=1, keepdims=True)
    e = gamma(m + 1) * (np.abs(b1)[None, :] + x @ np.abs(w1).T)
    return pre, h, z, e


def logits64(x, mlp):
    """(z, bound) of policy_reference on the samples' planes."""
    return pref.logits64(x, mlp)


def grads64(x, mlp, dz, relu_at_zero=0.0):
    """The four gradients of the header in float64, kernel layout: dict w1 [D, H], b1 [H], w2 [H, 4], b2 [4].  relu_at_zero: the
    derivative taken at pre == 0 (the contract: 0)."""
    w2 = np.asarray(mlp[2], np.float64)
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    pre, h, _, _ = forward64(x, mlp)
    dh = dz @ w2                                      # [M, H]
    dp = np.where(pre > 0, dh, np.where(pre == 0, relu_at_zero * dh, 0.0))
    return {"w1": x.T @ dp, "b1": dp.sum(axis=0), "w2": h.T @ dz, "b2": dz.sum(axis=0)}


def grad_bounds(x, mlp, dz):
    """(bounds, ambiguous): the per-entry bound of the module's docstring for sums that start from zero, in the shapes of
    grads64, and the boolean [M, H] of ambiguous (sample, unit) pairs."""
    w2 = np.abs(np.asarray(mlp[2], np.float64))       # [4, H]
    x, adz = np.asarray(x, np.float64), np.abs(np.asarray(dz, np.float64))
    dzs = np.asarray(dz, np.float64)
    M = x.shape[0]
    pre, h, _, e = forward64(x, mlp)
    dh = np.abs(dzs @ np.asarray(mlp[2], np.float64))
    d = gamma(4) * (adz @ w2)
    ambiguous = np.abs(pre) <= e
    eps = d + np.where(ambiguous, dh, 0.0)            # |dp^ - dp|
    mag = dh + d                                      # |dp^|
    count = x.sum(axis=0)                             # samples that have feature f
    bounds = {
        "b2": gamma(M) * adz.sum(axis=0),
        "w2": e.T @ adz + gamma(M + 1) * ((np.abs(h) + e).T @ adz),
        "b1": eps.sum(axis=0) + gamma(M) * mag.sum(axis=0),
        "w1": x.T @ eps + gamma(count)[:, None] * (x.T @ mag),
    }
    return bounds, ambiguous


def exactness_guard(x, mlp, dz, prefill=None):
    """For integer inputs: every term of every sum the kernels form is an integer and sum |terms| < 2**24 for every gradient
    entry, every pre-activation and every logit - so every order of float32 sums, fused or not, is exact."""
    w1, b1, w2, b2 = (np.asarray(a, np.float64) for a in mlp)
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    for a in (w1, b1, w2, b2, x, dz):
        assert (a == np.round(a)).all(), "the exact cases need integer inputs"
    limit = 2.0 ** 24
    apre = x @ np.abs(w1).T + np.abs(b1)
    assert apre.max(initial=0) < limit
    assert (apre @ np.abs(w2).T + np.abs(b2)).max(initial=0) < limit
    adh = np.abs(dz) @ np.abs(w2)
    sums = {"w1": x.T @ adh, "b1": adh.sum(axis=0), "w2": apre.T @ np.abs(dz), "b2": np.abs(dz).sum(axis=0)}
    for name, s in sums.items():
        extra = 0.0 if prefill is None else np.abs(np.asarray(prefill[name], np.float64))
        assert (s + extra).max(initial=0) < limit, name
    return True


def torch_grads64(x, mlp, dz):
    """float64 torch autograd on the dense planes, kernel layout: the cross-check of grads64's closed form."""
    import torch
    w1, b1, w2, b2 = (torch.tensor(np.asarray(a, np.float64), requires_grad=True) for a in mlp)
    z = torch.relu(torch.tensor(np.asarray(x, np.float64)) @ w1.T + b1) @ w2.T + b2
    z.backward(torch.tensor(np.asarray(dz, np.float64)))
    return {"w1": w1.grad.T.numpy().copy(), "b1": b1.grad.numpy().copy(), "w2": w2.grad.T.numpy().copy(), "b2": b2.grad.numpy().copy()}


# kernel name -> (S, T, obstacles): one case per kernel of the training library, run at 4,096 waves by tests/test_gpu_train.py
_OCC_SHAPES = {1: (1, 0), 2: (2, 1), 3: (2, 1), 4: (2, 2), 5: (2, 3), 6: (2, 6), 7: (2, 8), 8: (2, 10)}
OCCUPANCY_CASES = {f"k_train_{which}<{S}>": (S, T, K) for S, (T, K) in _OCC_SHAPES.items() for which in ("forward", "backward")}


# ---------------------------------------------------------------------------------------------- the exact backward cases
# (S, T, Tt, obstacles, multi colour, what, seed): tests/test_gpu_train.py runs each at 257 boards for every (H, K) of BACKWARD_HK.
# Cells are drawn at random, not played, so that tiles do share cells.  The seeds were chosen with backward_case() on the CPU so
# that every assertion of it holds on the yardstick's own numbers.
BACKWARD_CASES = ((4, 2, 2, 2, False, "", 0), (5, 3, 3, 3, True, "", 0), (8, 8, 8, 6, True, "not in LDS", 0), (3, 4, 4, 1, False, "", 0),
                  (1, 1, 1, 0, True, "", 0), (4, 0, 2, 3, False, "zero tiles", 0), (4, 3, 2, 2, True, "T != Tt", 0),
                  (4, 3, 3, 2, False, "repeated targets", 0), (4, 2, 2, 2, False, "beyond", 0), (8, 3, 3, 10, True, "beyond", 0))
BACKWARD_HK = tuple((H, K) for H in (1, 7, 64) for K in (1, 2, 5))
N_BOARDS = 257


def random_levels(orc, S, T, Tt, K_obstacles, n, seed):
    """n random levels of any shape: obstacles and targets drawn apart (cells are drawn by the caller)."""
    blk, _, _ = orc.generate(S, 0, 0, K_obstacles, n, seed=seed)
    _, _, tgt = orc.generate(S, 0, Tt, 0, n, seed=seed + 1)
    return blk, tgt


def backward_case(orc, case, H, K, n=N_BOARDS):
    """Levels, cells, network, dz, prefill and the yardstick's answer of one exact case, with the assertions that it bites.  The
    network and dz are redrawn (a fixed sequence of seeds, on the yardstick's own numbers alone) until they do; a 1x1 board has one
    constant input, so with a single hidden unit it cannot both sit on the kink of the ReLU and have a gradient: there the
    kink is not asked for."""
    S, T, Tt, Ko, mc, what, seed = BACKWARD_CASES[case]
    C = S * S
    rng = np.random.default_rng(10000 * case + 100 * H + K + 7919 * seed)
    blk, tgt = random_levels(orc, S, T, Tt, Ko, n, 0x7A11 + case)
    if C > 1:
        blk[(C - 1) // 32] &= ~np.uint32(1 << ((C - 1) % 32))      # no board has an obstacle on the last cell: an untouched row
    if what == "repeated targets":
        tgt[2] = tgt[0]
    top = 256 if what == "beyond" else C                            # ids S*S .. 255 are clamped to S*S - 1
    first = rng.integers(0, top, (T, n)).astype(np.uint8)
    pos_log = rng.integers(0, top, (K, T, n)).astype(np.uint8)
    if what == "beyond":
        keep = rng.random((K, T, n)) < 0.7
        pos_log = np.where(keep, pos_log % C, pos_log).astype(np.uint8)
        first = np.where(keep[0], first % C, first).astype(np.uint8)
        tgt[Tt - 1, rng.random(n) < 0.3] = 255
    x = samples_onehot(S, mc, blk, first, pos_log, tgt, K)
    D = features(S, T, Tt, mc)
    assert x.shape == (K * n, D)
    planes = [p for p in range(D // C) if x[:, p * C:(p + 1) * C].any()]
    want_kink = not (C == 1 and H == 1)
    for attempt in range(64):
        mlp = int_mlp(rng, D, H)
        dz = rng.integers(-1, 2, (K, n, 4)).astype(np.float32)
        flat = dz.reshape(K * n, 4)
        g = grads64(x, mlp, flat)
        pre, _, z, _ = forward64(x, mlp)
        dh = flat.astype(np.float64) @ mlp[2].astype(np.float64)
        bites = float(((pre == 0) & (dh != 0)).mean())
        if (bites >= 0.01 or not want_kink) and all(g["w1"][p * C:(p + 1) * C].any() for p in planes):
            break
    kl = kernel_layout(mlp)
    prefill = {name: rng.integers(-3, 4, a.shape).astype(np.float32) for name, a in zip(("w1", "b1", "w2", "b2"), kl)}
    exactness_guard(x, mlp, flat, prefill)
    want = {name: (prefill[name].astype(np.float64) + g[name]).astype(np.float32) for name in g}
    shared = shared_cell_share(first, pos_log, K, C)
    untouched = x.sum(axis=0) == 0
    ctx = (case, H, K)
    assert bites >= 0.01 or not want_kink, (ctx, bites)
    if T >= 2:
        assert shared >= 0.01, (ctx, shared)
    for p in planes:
        assert g["w1"][p * C:(p + 1) * C].any(), (ctx, "plane", p)
    if C > 1 and Ko > 0:
        assert untouched.any(), ctx
    assert (want["w1"][untouched] == prefill["w1"][untouched]).all()
    return dict(S=S, T=T, Tt=Tt, mc=mc, blk=blk, tgt=tgt, first=first, pos_log=pos_log, mlp=mlp, dz=dz, prefill=prefill, want=want,
                logits=z.astype(np.float32).reshape(K, n, 4), x=x, bites=bites, shared=shared, untouched=untouched)
