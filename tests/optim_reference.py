"""The float64 NumPy yardstick of the fused optimiser (include/tiler_slider_optim.h) and the bounds a float32 evaluation is held to.

adam64() restates the header's definition line by line in float64 on lists of float32 arrays.  The scalars the call receives as
float32 (lr, eps, weight_decay, max_grad_norm) are rounded to float32 first; the betas are doubles, as in ts_adam_cfg.

THE ONE-STEP BOUNDS.  Beside p', m', v' and gn the yardstick returns, per element, the magnitudes the bounds are taken against:

    Mm = |beta1 m| + (1 - beta1) |g^|
    Mv = beta2 v + (1 - beta2) g^^2
    Mp = |p| + lr (Mm / bc1) / denom               bc1 = 1 - beta1^t',  denom = sqrt(v' / bc2) + eps

and a float32 result must satisfy |got - want| <= 16 * 2^-24 * M + 2^-126 (TOL(M)).  Derivation: u = 2^-24 is half a float32 ulp
relative.  m' is two products and a sum of float32 inputs whose constants (float32(beta1), float32(1 - beta1), c) carry u each:
each term is off by at most 3 u of its own magnitude, the sum by u more - at most 5 u Mm once g^ = c g is counted, and a fused
multiply-add only removes roundings.  v' squares g^ (2 u for the two c g, u for the product), weighs it (2 u), and adds: below
7 u Mv.  p' chains m'/bc1 (5 u + u for bc1 + u), v'/bc2 (7 u + 2 u), a correctly rounded square root (halves the relative error:
4.5 u, + u), the sum with eps (u), the quotient (u), the product with lr (u) - about 16 u of the update term in the very worst
case, with every rounding at its bound and of the same sign - and the decayed parameter p (1 - lr weight_decay) with 3 u |p|, then
one more for the difference.  16 u M covers each of the three; 2^-126 is the underflow threshold, below which float32 loses
relative precision.  Measured on the CPU (test_optim_cpu.py): plain float32 NumPy stays at 2.0 (p), 2.5 (m) and 5.1 u (v) over 200 random
cases and torch's CPU float32 AdamW at 1.7 - typical roundings cancel; the bound does not rely on that.  A real defect (a swapped beta,
a bias correction from the wrong t, a clip from a stale norm) is off by thousands of u.

grad_norm must equal float32(gn) to within one float32 rounding: |got - float32(gn)| <= 2^-23 |gn| (one ulp).
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126

Step = namedtuple("Step", ("p", "m", "v", "gn", "skipped", "t", "Mp", "Mm", "Mv", "c"))


def tol(M):
    return 16 * U * M + TINY


def f32(x):
    return float(np.float32(x))


def adam64(p, g, m, v, t, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=0.0, skip_nonfinite=False):
    """One call on lists of arrays at counters[0] = t: Step of float64 lists p, m, v (the inputs unchanged where the step is
    skipped), gn, skipped, the new t, and the per-element magnitudes Mp, Mm, Mv."""
    lr, eps, wd, mx = f32(lr), f32(eps), f32(weight_decay), f32(max_grad_norm or 0.0)
    p, g, m, v = ([np.asarray(a, np.float64) for a in x] for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        gn = float(np.sqrt(sum(float((a * a).sum()) for a in g)))
        c = min(1.0, mx / (gn + 1e-6)) if mx > 0 else 1.0
    if skip_nonfinite and not np.isfinite(gn):
        return Step(p, m, v, gn, True, t, None, None, None, c)
    t1 = t + 1
    bc1, bc2 = 1.0 - beta1 ** t1, 1.0 - beta2 ** t1
    P, M, V, Mp, Mm, Mv = [], [], [], [], [], []
    with np.errstate(all="ignore"):
        for pi, gi, mi, vi in zip(p, g, m, v):
            gh = c * gi
            m1 = beta1 * mi + (1 - beta1) * gh
            v1 = beta2 * vi + (1 - beta2) * gh * gh
            denom = np.sqrt(v1 / bc2) + eps
            P.append(pi * (1 - lr * wd) - lr * (m1 / bc1) / denom)
            M.append(m1)
            V.append(v1)
            mm = np.abs(beta1 * mi) + (1 - beta1) * np.abs(gh)
            Mm.append(mm)
            Mv.append(v1)
            Mp.append(np.abs(pi) + lr * (mm / bc1) / denom)
    return Step(P, M, V, gn, False, t1, Mp, Mm, Mv, c)


def adam32(p, g, m, v, t, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=0.0):
    """The same step in plain float32 NumPy, with the constants rounded as the header says: what the bound is tried on."""
    F = np.float32
    lr, eps, wd, mx = F(lr), F(eps), F(weight_decay), F(max_grad_norm or 0.0)
    gn = float(np.sqrt(sum(float((np.asarray(a, np.float64) ** 2).sum()) for a in g)))
    c = F(min(1.0, float(mx) / (gn + 1e-6)) if mx > 0 else 1.0)
    t1 = t + 1
    bc1, bc2 = F(1.0 - beta1 ** t1), F(1.0 - beta2 ** t1)
    b1, b2, o1, o2 = F(beta1), F(beta2), F(1.0 - beta1), F(1.0 - beta2)
    P, M, V = [], [], []
    for pi, gi, mi, vi in zip(p, g, m, v):
        gh = c * gi.astype(F)
        m1 = b1 * mi.astype(F) + o1 * gh
        v1 = b2 * vi.astype(F) + o2 * (gh * gh)
        P.append(pi.astype(F) * (F(1) - lr * wd) - lr * (m1 / bc1) / (np.sqrt(v1 / bc2) + eps))
        M.append(m1)
        V.append(v1)
    return P, M, V


def worst(got, want, M):
    """The largest |got - want| over all elements of the lists, in units of 2^-24 M (inf for a NaN)."""
    w = 0.0
    for a, b, mm in zip(got, want, M):
        if a.size:
            with np.errstate(all="ignore"):
                r = (np.abs(np.asarray(a, np.float64) - b) - TINY) / (U * mm)
            w = max(w, float(np.nan_to_num(r, nan=np.inf).max()))
    return w


def within(got, want, M):
    return all(bool((np.abs(np.asarray(a, np.float64) - b) <= tol(mm)).all()) for a, b, mm in zip(got, want, M))


def gradients(shapes, seed, lo=1e-4, hi=1e2):
    """float32 gradients with |g| log-uniform in [lo, hi] and a random sign."""
    rng = np.random.default_rng(seed)
    out = []
    for n in shapes:
        mag = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
        out.append((mag * rng.choice((-1.0, 1.0), n)).astype(np.float32))
    return out


def state(shapes, seed, t):
    """(p, m, v) float32: parameters of unit size; at t = 0 zero moments, otherwise moments as t steps of such gradients leave."""
    rng = np.random.default_rng(seed + 7919)
    p = [rng.standard_normal(n).astype(np.float32) for n in shapes]
    if t == 0:
        return p, [np.zeros(n, np.float32) for n in shapes], [np.zeros(n, np.float32) for n in shapes]
    m = [(rng.standard_normal(n) * 3.0).astype(np.float32) for n in shapes]
    v = [(rng.uniform(0.01, 50.0, n)).astype(np.float32) for n in shapes]
    return p, m, v


def exact_case(one=False):
    """1,024 elements in tensors of (1000, 24): g = +-2^k with k in -3 .. 3 (+-1 with `one`: grad_norm is exactly 32), p small
    integers, m = v = 0 at t = 0; beta1 = 0.5, beta2 = 0.75, eps = 0, lr = 2^-4, no decay, no clip.  Every intermediate is a
    float32: p' = p - lr sign(g), m' = g / 2, v' = g^2 / 4 bit for bit.  (cfg, p, g, want p, want m, want v)."""
    rng = np.random.default_rng(21)
    shapes = (1000, 24)
    k = [np.zeros(n, np.int64) if one else rng.integers(-3, 4, n) for n in shapes]
    g = [(np.ldexp(1.0, ki) * rng.choice((-1.0, 1.0), ki.size)).astype(np.float32) for ki in k]
    p = [rng.integers(-8, 9, n).astype(np.float32) for n in shapes]
    cfg = dict(lr=2.0 ** -4, beta1=0.5, beta2=0.75, eps=0.0, weight_decay=0.0, max_grad_norm=0.0)
    want_p = [pi - np.float32(2.0 ** -4) * np.sign(gi) for pi, gi in zip(p, g)]
    return cfg, p, g, want_p, [gi / 2 for gi in g], [gi * gi / 4 for gi in g]
