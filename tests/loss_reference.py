"""CPU yardstick of the fused actor-critic loss (test infrastructure, no test of its own): the definition of
include/tiler_slider_loss.h restated on NumPy in float64, with an a-priori per-entry error bound for ANY float32 evaluation of
it, and the guard that names the samples on which a float32 evaluation may honestly take the other side of PPO's clip.  It
shares no code with tiler_slider_amd/csrc/ts_loss.hip and imports neither torch nor the libraries at import time.

THE BOUND is carried through the formula as (value, absolute error) pairs - class E below - with u = 2**-24:
  * an input is exact; a float32 constant computed from an input (1 - clip) carries u |value|
  * a + b:   e_a + e_b, and one rounding u (|a + b| + e_a + e_b)
  * a * b:   |a| e_b + |b| e_a + e_a e_b, and one rounding (a fused multiply-add rounds once less: the bound holds for it)
  * a / b:   (e_a + |a / b| e_b) / (|b| - e_b), and one rounding
  * a sum of n terms in ANY order or tree: sum e_i + (n - 1) u sum (|t_i| + e_i)   (Higham, Accuracy and Stability, section 4.2)
  * exp(a), the hardware's: x -> 2**(x log2 e).  The product rounds once and log2 e is a rounded constant, 2 u |x| log2 e in the
    exponent, which the exponential turns into a relative 2 u |x|; the instruction itself is documented at 1 ulp = 2 u.
    Relative (2 |x| + 2.5) u, on top of exp(e_a) - 1 from the argument's own error - this is where the absolute error of z - max z
    is carried through the exponential - and 2**-126 absolute for a result flushed to zero.
  * log(a), the hardware's: log2 at 1 ulp, times a rounded ln 2, one rounding: 4 u |log a|, on top of e_a / (a - e_a).
  * max and the selects are exact.
mu and sigma come from float64 sums (the header says so): their error is the rounding to float32 and a float64 term
(M + 8) 2**-52 mean(adv^2), negligible unless sigma is.
Every bound is multiplied by SLACK = 1.0625 for the second-order terms the rules above drop where they say "and one rounding".

THE SCALAR BOUND is the issue's: 64 * 2**-24 * c * sum |term| - at most 24 levels of summation for M <= 2**24, up to 8 ulp a term,
rounded up - where the terms of a sum are the quantities that enter it: l_pi, value_coef l_v and entropy_coef H for L; r - 1 and
log r for the approximate KL (its summand is itself a difference; its two parts are the terms that carry the rounding).
count is exact, the share of cut samples may differ by the ambiguous samples, mu is bounded as above.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
SLACK = 1.0625
FLUSH = 2.0 ** -126
SCALARS = ("loss", "policy", "value", "entropy", "approx_kl", "clip_frac", "count", "mu")
MODES = ("a2c", "ppo", "ce")


class E:
    """A float64 array and a bound of the absolute error of its float32 evaluation."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    def _round(self, v, e):
        return E(v, e + U * (np.abs(v) + e))

    def __add__(self, o):
        o = o if isinstance(o, E) else E(o)
        return self._round(self.v + o.v, self.e + o.e)

    def __neg__(self):
        return E(-self.v, self.e)

    def __sub__(self, o):
        o = o if isinstance(o, E) else E(o)
        return self + (-o)

    def __mul__(self, o):
        o = o if isinstance(o, E) else E(o)
        return self._round(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        v = self.v / o.v
        den = np.abs(o.v) - o.e
        assert (den > 0).all(), "a divisor that may be zero"
        return self._round(v, (self.e + np.abs(v) * o.e) / den)

    def exp(self):
        v = np.exp(self.v)
        return E(v, v * (np.expm1(self.e) + (2.0 * np.abs(self.v) + 2.5) * U * np.exp(self.e)) + FLUSH)

    def log(self):
        assert (self.v - self.e > 0).all()
        v = np.log(self.v)
        return E(v, self.e / (self.v - self.e) + 4.0 * U * np.abs(v))

    def pick(self, a):
        return E(np.take_along_axis(self.v, a[:, None], 1)[:, 0], np.take_along_axis(np.asarray(self.e), a[:, None], 1)[:, 0])


def esum(terms):
    """The sum of a list of E in any order or tree."""
    v = sum(t.v for t in terms)
    e = sum(t.e for t in terms)
    mag = sum(np.abs(t.v) + t.e for t in terms)
    return E(v, e + (len(terms) - 1) * U * mag)


def _log_softmax(z):
    """(lp, e, s) as E over [M, 4] / [M]: through the max."""
    mx = z.max(axis=1, keepdims=True)
    x = E(z) - E(mx)
    e = x.exp()
    s = esum([E(e.v[:, j], e.e[:, j]) for j in range(4)])
    ls = s.log()
    lp = x - E(ls.v[:, None], ls.e[:, None])
    return lp, e, s


Loss = namedtuple("Loss", ("dlogits", "dvalues", "scalars", "live", "dlogits_bound", "dvalues_bound", "scalars_bound", "ambiguous", "terms"))


def loss64(logits, act, mask=None, adv=None, old_logits=None, values=None, ret=None, clip=0.0, value_coef=0.5, entropy_coef=0.0,
           normalize_adv=False):
    """The header's definition in float64 on flat samples (logits [M, 4], the others [M]): Loss(dlogits [M, 4], dvalues [M] or
    None, scalars [8], live, the three bounds, the ambiguous samples, the per-sample terms)."""
    clip, value_coef, entropy_coef = (float(np.float32(x)) for x in (clip, value_coef, entropy_coef))   # as the call receives them
    z = np.asarray(logits, np.float64).reshape(-1, 4)
    M = z.shape[0]
    act = np.asarray(act).reshape(M).astype(np.int64)
    live = act <= 3
    if mask is not None:
        live &= np.asarray(mask).reshape(M) != 0
    a = np.minimum(act, 3)
    count = int(live.sum())
    n = max(count, 1)
    c = E(np.full(M, 1.0 / n), U / n)
    z = np.where(live[:, None], z, 0.0)     # what a sample that is not live holds is never looked at
    f = lambda t: None if t is None else np.where(live, np.asarray(t, np.float64).reshape(M), 0.0)
    adv, values, ret = f(adv), f(values), f(ret)
    mu = 0.0 if adv is None else adv[live].sum() / n
    if adv is None:
        A = E(np.ones(M))
    elif normalize_adv and (count == 0 or (adv[live] == adv[live][0]).all()):
        A = E(np.zeros(M))      # one live sample, or all alike: the float64 mean is that float32 itself and adv - mu is exactly 0
    elif normalize_adv:
        sigma = np.sqrt(((adv[live] - mu) ** 2).sum() / n) if count else 0.0
        e_var = (M + 8) * 2.0 ** -52 * (adv[live] ** 2).sum() / n       # of a float64 E[adv^2] - mu^2
        e_sigma = np.sqrt(e_var) if sigma * sigma <= e_var else e_var / sigma
        A = (E(adv) - E(mu, U * abs(mu) + e_var)) / E(sigma + 1e-8, U * (sigma + 1e-8) + e_sigma)
    else:
        A = E(adv)
    lp, e, s = _log_softmax(z)
    p = e / E(s.v[:, None], s.e[:, None])
    H = -esum([E(p.v[:, j], p.e[:, j]) * E(lp.v[:, j], lp.e[:, j]) for j in range(4)])
    lpa = lp.pick(a)
    ambiguous = np.zeros(M, bool)
    zero = E(np.zeros(M))
    if old_logits is not None:
        zo = np.where(live[:, None], np.asarray(old_logits, np.float64).reshape(M, 4), 0.0)
        d = lpa - _log_softmax(zo)[0].pick(a)
        r = d.exp()
        lo, hi = E(1.0 - clip, U * abs(1.0 - clip)), E(1.0 + clip, U * (1.0 + clip))
        near = lambda edge: np.abs(r.v - edge.v) <= SLACK * (r.e + edge.e)
        # inside the interval by more than the bound the clamp returns r itself and the two products are the SAME float: a tie,
        # the unclipped side.  Outside it by more than the bound the sign of A decides: ambiguous where A may be of either sign.
        outside = (r.v < lo.v) | (r.v > hi.v)
        ambiguous = live & (near(lo) | near(hi) | (outside & (A.v != 0) & (np.abs(A.v) <= SLACK * A.e)))
        rc = E(np.clip(r.v, lo.v, hi.v), np.maximum(r.e, np.maximum(lo.e, hi.e)))
        u1, u2 = r * A, rc * A
        unclipped = u1.v <= u2.v
        lpi = E(np.where(unclipped, -u1.v, -u2.v), np.maximum(u1.e, u2.e))
        g = E(np.where(unclipped, -u1.v, 0.0), np.where(unclipped, u1.e, 0.0))
        kl_terms = (r - E(1.0), d)
        kl = kl_terms[0] - d
        cut = (~unclipped).astype(np.float64)
    else:
        lpi, g, kl, cut, kl_terms = -(A * lpa), -A, zero, np.zeros(M), (zero, zero)
    onehot = (a[:, None] == np.arange(4)[None, :]).astype(np.float64)
    col = lambda t: E(t.v[:, None], np.asarray(t.e)[:, None])
    dz = col(c) * (col(g) * (E(onehot) - p) + E(entropy_coef) * p * (lp + col(H)))
    dlogits = np.where(live[:, None], dz.v, 0.0)
    dlogits_bound = np.where(live[:, None], SLACK * dz.e, 0.0)
    dvalues = dvalues_bound = None
    lv = zero
    if values is not None:
        dv = E(values) - E(ret)
        lv = dv * dv
        k = E(2.0) * c * E(value_coef)
        dvv = k * dv
        dvalues, dvalues_bound = np.where(live, dvv.v, 0.0), np.where(live, SLACK * dvv.e, 0.0)
    w = live.astype(np.float64)
    tot = lambda t: float((t * w).sum()) / n
    kl_mag = tot(np.abs(kl_terms[0].v) + np.abs(kl_terms[1].v))
    scalars = np.array([tot(lpi.v + value_coef * lv.v - entropy_coef * H.v), tot(lpi.v), tot(lv.v), tot(H.v), tot(kl.v), tot(cut), count,
                        mu])
    sb = 64.0 * U
    scalars_bound = np.array([sb * tot(np.abs(lpi.v) + abs(value_coef) * lv.v + abs(entropy_coef) * np.abs(H.v)), sb * tot(np.abs(lpi.v)), sb * tot(lv.v),
                              sb * tot(np.abs(H.v)), sb * kl_mag, (int(ambiguous.sum()) + 0.5) / n * (1 + 4 * U) + 4 * U, 0.0,
                              4 * U * (tot(np.abs(adv)) if adv is not None else 0.0)])
    terms = dict(lpi=lpi.v, lv=lv.v, H=H.v, kl=kl.v, cut=cut, A=A.v, p=p.v, lp=lp.v)
    return Loss(dlogits, dvalues, scalars, live, dlogits_bound, dvalues_bound, scalars_bound, ambiguous, terms)


def worst(err, bound):
    """The largest error / bound over the entries whose bound is positive (0.0 if there is none).  Where a bound is exactly 0 -
    value_coef = 0, an advantage standardised to 0 without an entropy term - the error must be exactly 0: no 0 / 0 enters a
    ratio, and an error there makes the result infinite."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    exact = bound == 0
    if (err[exact] != 0).any():
        return float("inf")
    return float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0


def loss32(logits, act, mask=None, adv=None, old_logits=None, values=None, ret=None, clip=0.0, value_coef=0.5, entropy_coef=0.0,
           normalize_adv=False, order=0):
    """A float32 NumPy evaluation of the definition: (dlogits, dvalues, scalars).  order 0 follows the formula as written
    (p = exp(lp), sums left to right); order 1 takes p = e / s, sums the other way round - the samples from the last to the first, as a binary tree - and factors the
    gradient differently."""
    f32 = np.float32
    z = np.asarray(logits, f32).reshape(-1, 4)
    M = z.shape[0]
    act = np.asarray(act).reshape(M).astype(np.int64)
    live = act <= 3
    if mask is not None:
        live &= np.asarray(mask).reshape(M) != 0
    a = np.minimum(act, 3)
    count = int(live.sum())
    c = f32(1.0) / f32(max(count, 1))
    g32 = lambda t: None if t is None else np.where(live, np.asarray(t, f32).reshape(M), f32(0))
    adv, values, ret = g32(adv), g32(values), g32(ret)
    z = np.where(live[:, None], z, f32(0))
    cols = (0, 1, 2, 3) if order == 0 else (3, 2, 1, 0)

    def lsm(z):
        x = z - z.max(axis=1, keepdims=True)
        e = np.exp(x)
        s = f32(0)
        for j in cols:
            s = s + e[:, j]
        return x - np.log(s)[:, None], e, s

    lp, e, s = lsm(z)
    p = np.exp(lp) if order == 0 else e / s[:, None]
    H = f32(0)
    for j in cols:
        H = H - p[:, j] * lp[:, j]
    mu = f32(0)
    if adv is None:
        A = np.ones(M, f32)
    else:
        mu = f32(adv[live].astype(np.float64).sum() / max(count, 1))
        A = adv
        if normalize_adv:
            sigma = f32(np.sqrt(max((adv[live].astype(np.float64) ** 2).sum() / max(count, 1) - float(mu) ** 2, 0.0)) + 1e-8)
            A = (adv - mu) / sigma
    pick = lambda t: np.take_along_axis(t, a[:, None], 1)[:, 0]
    lpa = pick(lp)
    onehot = (a[:, None] == np.arange(4)[None, :]).astype(f32)
    kl, cut = np.zeros(M, f32), np.zeros(M, f32)
    if old_logits is not None:
        zo = np.where(live[:, None], np.asarray(old_logits, f32).reshape(M, 4), f32(0))
        d = lpa - pick(lsm(zo)[0])
        r = np.exp(d)
        u1, u2 = r * A, np.clip(r, f32(1) - f32(clip), f32(1) + f32(clip)) * A
        unclipped = u1 <= u2
        lpi, g = np.where(unclipped, -u1, -u2), np.where(unclipped, -u1, f32(0))
        kl, cut = (r - f32(1)) - d, (~unclipped).astype(f32)
    else:
        lpi, g = -A * lpa, -A
    beta = f32(entropy_coef)
    if order == 0:
        dz = c * (g[:, None] * (onehot - p) + beta * p * (lp + H[:, None]))
    else:
        dz = (c * g)[:, None] * onehot - (c * g)[:, None] * p + (c * beta) * (p * lp + p * H[:, None])
    dz = np.where(live[:, None], dz, f32(0)).astype(f32)
    dvalues, lv = None, np.zeros(M, f32)
    if values is not None:
        dv = values - ret
        lv = dv * dv
        dvalues = np.where(live, (f32(2) * c * f32(value_coef)) * dv if order == 0 else f32(2) * (c * (f32(value_coef) * dv)), f32(0)).astype(f32)

    def tree(t):
        """From the last sample to the first, halved until one is left: ceil(log2 M) levels.  (A running sum has M - 1 levels: its
        a-priori error, (M - 1) u sum |t|, is beyond the scalar bound's 64 u sum |t| - and its premise of 24 levels - from M = 66.)"""
        t = t[::-1]
        while t.size > 1:
            t = np.append(t, f32(0)) if t.size % 2 else t
            t = t[0::2] + t[1::2]
        return t[0] if t.size else f32(0)

    def tot(t):
        t = np.where(live, t, f32(0)).astype(f32)
        return c * (t.sum(dtype=f32) if order == 0 else tree(t))

    spi, sv, sh = tot(lpi), tot(lv), tot(H)
    scalars = np.array([spi + f32(value_coef) * sv - beta * sh, spi, sv, sh, tot(kl), tot(cut), f32(count), mu], f32)
    return dz, dvalues, scalars


def torch_loss(logits, act, mask=None, adv=None, old_logits=None, values=None, ret=None, clip=0.0, value_coef=0.5, entropy_coef=0.0,
               normalize_adv=False):
    """The plain-torch loss a user writes (README: log_softmax, gather, the mask, the sums), on torch tensors of any float
    dtype; differentiable in logits and values.  Returns the scalar loss."""
    import torch
    live = act <= 3
    if mask is not None:
        live = live & (mask != 0)
    w = live.to(logits.dtype)
    count = w.sum().clamp(min=1)
    logp = torch.log_softmax(logits, dim=-1)
    played = logp.gather(-1, act.clamp(max=3).long().unsqueeze(-1)).squeeze(-1)
    A = torch.ones_like(played) if adv is None else adv
    if normalize_adv:
        mu = (A * w).sum() / count
        sigma = ((((A - mu) ** 2) * w).sum() / count).sqrt()
        A = (A - mu) / (sigma + 1e-8)
    if old_logits is not None:
        old = torch.log_softmax(old_logits, dim=-1).gather(-1, act.clamp(max=3).long().unsqueeze(-1)).squeeze(-1)
        r = (played - old).exp()
        policy = -torch.minimum(r * A, r.clamp(1 - clip, 1 + clip) * A)
    else:
        policy = -A * played
    total = policy - entropy_coef * -(logp.exp() * logp).sum(-1)
    if values is not None:
        total = total + value_coef * (values - ret) ** 2
    return (torch.where(live, total, torch.zeros_like(total))).sum() / count


def case(mode, M, seed, scale=3.0, spread=None, void=0.2):
    """Inputs of one test case as a dict of float32 / uint8 arrays plus the keyword arguments of the mode: Gaussian logits of
    `scale` (or four logits spread evenly over `spread`, shuffled per sample), a fifth of the samples not live - by the mask or
    by an action byte above 3 - and NaN in every input of a sample that is not live."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    z = (rng.standard_normal((M, 4)) * scale).astype(f32)
    if spread is not None:
        base = np.linspace(-spread / 2, spread / 2, 4)
        z = np.stack([rng.permutation(base) for _ in range(M)]).astype(f32) + (rng.standard_normal((M, 4)) * 0.01).astype(f32)
    act = rng.integers(0, 4, M).astype(np.uint8)
    mask = (rng.random(M) >= void / 2).astype(np.uint8)
    act[rng.random(M) < void / 2] = rng.choice(np.array([4, 200, 255], np.uint8))
    kw = dict(logits=z, act=act)
    if mode == "ce":
        kw.update(entropy_coef=0.0)
    else:
        kw.update(mask=mask, adv=(rng.standard_normal(M) * 0.7 + 0.3).astype(f32), values=rng.standard_normal(M).astype(f32),
                  ret=rng.standard_normal(M).astype(f32), value_coef=0.5, entropy_coef=0.01)
    if mode == "ppo":
        kw.update(old_logits=(z + rng.standard_normal((M, 4)) * 0.5).astype(f32), clip=0.2, normalize_adv=True)
    live = (act <= 3) & ((mask != 0) if "mask" in kw else True)
    for name in ("logits", "old_logits", "adv", "values", "ret"):
        if name in kw:
            kw[name] = kw[name].copy()
            kw[name][~live] = np.nan
    return kw


NAMES = ("old", "val", "adv", "mask")
# the sixteen (old, val, adv, mask) settings: one compiled body of k_loss_main each; (adv, mask) names k_loss_stats' four
BODIES = tuple((o, v, a, m) for o in (0, 1) for v in (0, 1) for a in (0, 1) for m in (0, 1))
# ... and the 24 configurations the tests run: every body, and every body with adv once more with normalize_adv
CONFIGS = tuple((b, nz) for b in BODIES for nz in ((False, True) if b[2] else (False,)))
# (clip, value_coef, entropy_coef) off the defaults: a narrow clip under a heavy value and entropy term; 1 - clip < 0, no weight
# on the value term and an entropy penalty; a clip that never cuts
COEFFICIENTS = ((0.05, 2.0, 0.3), (1.5, 0.0, -0.05), (1e30, 0.5, 0.0))
STALES = (0.5, 3.0)


def body_id(old, val, adv, mask, normalize=False):
    """"old+val+adv+mask", "adv+mask", "none"; "-norm" behind a body that standardises its advantages."""
    return ("+".join(n for n, on in zip(NAMES, (old, val, adv, mask)) if on) or "none") + ("-norm" if normalize else "")


def case_of(old, val, adv, mask, M, seed, *, normalize=False, clip=0.2, value_coef=0.5, entropy_coef=0.01, stale=0.5, scale=3.0):
    """Inputs for any of the sixteen bodies, by case()'s recipe: Gaussian logits of `scale`, about a tenth of the samples dead by
    an action byte in {4, 200, 255} (drawn per sample) and, where there is a mask, another tenth by the mask; NaN in every float
    input of a sample that is not live.  old_logits - logits is Gaussian of `stale`.  Every array is drawn whether the body takes
    it or not, so two bodies of one seed share their logits and actions; sample 0 is always live, so that M = 1 is a sample."""
    assert adv or not normalize, "normalize_adv needs adv"
    rng = np.random.default_rng(seed)
    f32 = np.float32
    z = (rng.standard_normal((M, 4)) * scale).astype(f32)
    drift = rng.standard_normal((M, 4)) * stale
    act = rng.integers(0, 4, M).astype(np.uint8)
    byte = rng.choice(np.array([4, 200, 255], np.uint8), M)
    dead, off = rng.random(M) < 0.1, rng.random(M) < 0.1
    a, v, rt = (rng.standard_normal(M) * 0.7 + 0.3).astype(f32), rng.standard_normal(M).astype(f32), rng.standard_normal(M).astype(f32)
    dead[:1] = off[:1] = False
    act[dead] = byte[dead]
    kw = dict(logits=z, act=act, entropy_coef=entropy_coef)
    live = ~dead
    if mask:
        kw.update(mask=(~off).astype(np.uint8))
        live &= ~off
    if adv:
        kw.update(adv=a)
        if normalize:
            kw.update(normalize_adv=True)
    if old:
        kw.update(old_logits=(z + drift).astype(f32), clip=clip)
    if val:
        kw.update(values=v, ret=rt, value_coef=value_coef)
    for name in ("logits", "old_logits", "adv", "values", "ret"):
        if name in kw:
            kw[name][~live] = np.nan
    return kw


def exact_case(count_log2=8, extra=1):
    """The exact case: all four logits of a sample equal, integer adv, integer values - ret, a power of two of live samples and
    `extra` samples that are not live (NaN logits, adv and values there), entropy_coef = 0: every product of the gradient is a
    float32, so dlogits = -A (delta - 1/4) c and dvalues = 2 c value_coef (v - ret) hold bit for bit."""
    rng = np.random.default_rng(5)
    f32 = np.float32
    n = 1 << count_log2
    M = n + extra
    void = np.zeros(M, bool)
    void[rng.choice(M, extra, replace=False)] = True
    z = np.repeat(rng.integers(-5, 6, (M, 1)).astype(f32), 4, axis=1)
    act = rng.integers(0, 4, M).astype(np.uint8)
    mask = np.ones(M, np.uint8)
    adv = rng.integers(-4, 5, M).astype(f32)
    values, ret = rng.integers(-8, 9, M).astype(f32), rng.integers(-8, 9, M).astype(f32)
    half = void & (np.arange(M) % 2 == 0)
    mask[half] = 0
    act[void & ~half] = 255
    for t in (z, adv, values, ret):
        t[void] = np.nan
    c = f32(1.0 / n)
    onehot = (act[:, None] == np.arange(4)[None, :]).astype(f32)
    dz = np.where(void[:, None], f32(0), -adv[:, None] * (onehot - f32(0.25)) * c).astype(f32)
    dv = np.where(void, f32(0), f32(2) * c * f32(0.5) * (values - ret)).astype(f32)
    kw = dict(logits=z, act=act, mask=mask, adv=adv, values=values, ret=ret, value_coef=0.5, entropy_coef=0.0)
    return kw, dz, dv, n
