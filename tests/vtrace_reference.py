"""CPU yardstick of the V-trace targets (test infrastructure, no test of its own): the definition of include/tiler_slider_vtrace.h
restated on NumPy in float64, with an a-priori per-entry bound of the error of ANY float32 evaluation of it.  It shares no code
with tiler_slider_amd/csrc/ts_vtrace.hip and imports neither torch nor the libraries at import time.  Flags, actions and cells
come from targets_reference.trajectory; the Manhattan terms are its m_before / m_after.

THE BOUND is carried through the formula as (value, absolute error) pairs with the rules of tests/loss_reference.py - class E
there: product, sum in any order or tree (esum), the hardware's exp and log, and the division, which the header promises to be the
correctly rounded one: (e_a + |a / b| e_b) / (|b| - e_b) and one rounding - and two more:
  * min(constant, a) is 1-Lipschitz: the value is clipped, the error is kept
  * eps / 4, 1 - eps, beta and 1 - beta reach the kernel as float32 constants: u |value| each (0 where the value is a float32)
Where the order of evaluation is free the bound takes the form that covers every order: r_k is a sum of six terms in any order;
r + gamma V+ - V is a sum of eight; D_k is a sum of delta and (gamma c) D+; adv is bounded in both of its forms,
rho (r + gamma (V+ + D+) - V) and delta + (gamma rho) D+, and the larger bound is taken.  The carry's own error goes down the
recursion with it.  Derived, not tuned; every bound is multiplied by loss_reference.SLACK = 1.0625 as there.

mu == 0 happens in real arithmetic (TS_POLICY_GREEDY with eps = 0: an action that is neither the argmax nor the expert's), so
float32 and float64 agree on where: w is +infinity there exactly, log_mu -infinity exactly, rho and min(c_bar, w) the bars exactly.
A bar that is itself infinite on such a sample leaves nothing finite to compare: vtrace64 refuses the combination.
"""
import numpy as np

import targets_reference as gr
from loss_reference import E, SLACK, U, esum

GREEDY, SAMPLE = 0, 1
TWO32 = 1 << 32
OUTPUTS = ("reward", "adv", "ret", "weight", "log_mu")
CASES = ("auto", "strict", "given", "long")
CELL_CASES = ("mc5", "s8")
# (epsilon, beta) of the issue, both selects: the sixteen combinations are CASES x PARAMS x SELECTS
PARAMS = ((0.125, 0.5), (0.0, 0.5))
SELECTS = (GREEDY, SAMPLE)
GAMMA, LAM = 0.97, 0.9
# floors each test asserts on the yardstick before it looks at anything else (shares of all steps / of the live samples)
FLOORS = dict(void=0.05, end=0.03, w_above=0.25, w_below=0.40, expert_played=0.15, expert_differs=0.15, mu_zero=0.30)
WEIGHTS = gr.Weights(step=-0.01, win=1.0, timeout=-0.5, invalid=-0.1, dist=0.05, progress=0.25)
FLAT = WEIGHTS._replace(dist=0.0, progress=0.0)


def threshold_of(x):
    return int(round(float(x) * 2**32))


def inputs(c, K=None):
    """dict of the random inputs of one trajectory (targets_reference.trajectory's dict), from default_rng(5): mu_logits =
    2 N(0, 1), pi_logits = mu_logits + N(0, 1), expert_log 255 with probability 0.4, the played action with 0.3, uniform 0 .. 3
    otherwise, and gaussian_values.  Drawn at the trajectory's own K and cut to the first K steps: a prefix of a log is a log."""
    full, n = c["K"], c["n"]
    rng = np.random.default_rng(5)
    mu = (2.0 * rng.standard_normal((full, n, 4))).astype(np.float32)
    pi = (mu + rng.standard_normal((full, n, 4)).astype(np.float32)).astype(np.float32)
    u = rng.random((full, n))
    played = np.minimum(c["log"]["act_log"], 3).astype(np.uint8)
    expert = np.where(u < 0.4, np.uint8(255), np.where(u < 0.7, played, rng.integers(0, 4, (full, n)).astype(np.uint8))).astype(np.uint8)
    V, VL = gr.gaussian_values(full, n)
    K = full if K is None else K
    return dict(mu_logits=mu[:K], pi_logits=pi[:K], expert_log=expert[:K], values=V[:K], last_value=VL, flags_log=c["log"]["flags_log"][:K],
                act_log=c["log"]["act_log"][:K], m_before=c["m_before"][:K], m_after=c["m_after"][:K])


def _const(x):
    """A real constant as the kernel holds it: rounded to float32 once."""
    x = float(x)
    return E(x, 0.0 if float(np.float32(x)) == x else U * abs(x))


def _softmax_at(z, a):
    """E [M]: softmax(z)[a] through the max, p = e / s."""
    x = E(z) - E(z.max(axis=1, keepdims=True))
    e = x.exp()
    s = esum([E(e.v[:, j], e.e[:, j]) for j in range(4)])
    return e.pick(a) / s


def vtrace64(flags_log, act_log, m_before, m_after, mu_logits, pi_logits=None, expert_log=None, values=None, last_value=None, gamma=GAMMA,
             lam=LAM, w=FLAT, rho_bar=1.0, c_bar=1.0, select=SAMPLE, explore_threshold=0, beta_threshold=0):
    """The header's definition in float64.  dict: reward, adv, ret, weight, log_mu float64 [K, N], mask uint8 [K, N], and
    bound_<output> float64 [K, N] (0 on void steps and where the value is exact by rule), mu [K, N] and live bool [K, N]."""
    f = np.asarray(flags_log)
    K, N = f.shape
    gamma, lam, rho_bar, c_bar = (float(np.float32(x)) for x in (gamma, lam, rho_bar, c_bar))   # as the call receives them
    wt = gr.Weights(*(float(np.float32(x)) for x in w))
    eps, beta = explore_threshold / TWO32, beta_threshold / TWO32
    M = K * N
    a = np.minimum(np.asarray(act_log).reshape(M), 3).astype(np.int64)
    x = np.full(M, 255, np.int64) if expert_log is None else np.asarray(expert_log).reshape(M).astype(np.int64)
    zm = np.asarray(mu_logits, np.float64).reshape(M, 4)
    p_sample = _softmax_at(zm, a)
    pe = E((a == zm.argmax(axis=1)).astype(np.float64)) if select == GREEDY else p_sample   # argmax: the lowest of the largest
    taught = (beta_threshold != 0) & (x != 255)
    mixed = _const(beta) * E((a == x).astype(np.float64)) + _const(1.0 - beta) * pe
    inner = E(np.where(taught, mixed.v, pe.v), np.where(taught, mixed.e, pe.e))
    mu = _const(eps / 4.0) + _const(1.0 - eps) * inner
    pi = p_sample if pi_logits is None else _softmax_at(np.asarray(pi_logits, np.float64).reshape(M, 4), a)
    none = mu.v == 0
    assert not (none.any() and (np.isinf(rho_bar) or np.isinf(c_bar))), "mu == 0 under an infinite bar: nothing finite is left"
    wq = pi / E(np.where(none, 1.0, mu.v), np.where(none, 0.0, mu.e))
    weight = E(np.where(none, np.inf, wq.v), np.where(none, 0.0, wq.e))
    lm = E(np.where(none, 1.0, mu.v), np.where(none, 0.0, mu.e)).log()
    log_mu = E(np.where(none, -np.inf, lm.v), np.where(none, 0.0, lm.e))
    rho = E(np.where(none, rho_bar, np.minimum(rho_bar, wq.v)), np.where(none, 0.0, wq.e))
    c = _const(lam) * E(np.where(none, c_bar, np.minimum(c_bar, wq.v)), np.where(none, 0.0, wq.e))
    grid = lambda t: E(t.v.reshape(K, N), np.asarray(t.e).reshape(K, N))
    rho, c = grid(rho), grid(c)
    row = lambda t, k: E(t.v[k], t.e[k])
    V = np.zeros((K, N)) if values is None else np.asarray(values, np.float64)
    VL = np.zeros(N) if last_value is None else np.asarray(last_value, np.float64)
    mb, ma = np.asarray(m_before, np.float64), np.asarray(m_after, np.float64)
    out = {k: np.zeros((K, N)) for k in ("reward", "adv", "ret") + tuple("bound_" + o for o in OUTPUTS)}
    out["mask"] = np.zeros((K, N), np.uint8)
    g = _const(gamma)
    carry = E(np.zeros(N))
    for k in range(K - 1, -1, -1):
        live = (f[k] & gr.VOID) == 0
        end = (f[k] & gr.END) != 0
        flag = lambda bit: ((f[k] & bit) != 0).astype(np.float64)
        terms = [E(np.full(N, wt.step)), E(wt.win * flag(gr.FLAG_SUCCESS)), E(wt.timeout * flag(gr.FLAG_TIMEOUT)), E(wt.invalid * flag(gr.FLAG_INVALID_MOVE)),
                 E(wt.dist) * E(ma[k]), E(wt.progress) * E(ma[k] - mb[k])]
        r = esum(terms)
        vplus = np.where(end, 0.0, VL if k == K - 1 else V[k + 1])
        rk, ck = row(rho, k), row(c, k)
        delta = rk * esum(terms + [g * E(vplus), E(-V[k])])
        back = (g * ck) * carry
        d_not_end = esum([delta, back])
        d = E(np.where(end, delta.v, d_not_end.v), np.where(end, delta.e, d_not_end.e))
        ret = E(V[k]) + d
        form_a = rk * esum(terms + [g * (E(vplus) + carry), E(-V[k])])
        form_b = esum([delta, (g * rk) * carry])
        adv = E(np.where(end, delta.v, form_a.v), np.where(end, delta.e, np.maximum(form_a.e, form_b.e)))
        carry = E(np.where(live, d.v, carry.v), np.where(live, d.e, carry.e))
        for name, t in (("reward", r), ("adv", adv), ("ret", ret)):
            out[name][k] = np.where(live, t.v, 0.0)
            out["bound_" + name][k] = np.where(live, SLACK * t.e, 0.0)
        out["mask"][k] = live
    live = out["mask"] != 0
    for name, t in (("weight", weight), ("log_mu", log_mu)):
        out[name] = np.where(live, t.v.reshape(K, N), 0.0)
        out["bound_" + name] = np.where(live, SLACK * np.asarray(t.e).reshape(K, N), 0.0)
    out["mu"], out["live"] = mu.v.reshape(K, N), live
    return out


def shares(want, flags_log, act_log, expert_log):
    """The quantities of the floors, measured on a yardstick result: void and end over all steps, the others over the live samples."""
    f, live = np.asarray(flags_log), want["live"]
    a, x = np.minimum(np.asarray(act_log), 3), np.asarray(expert_log)
    w = want["weight"][live]
    return dict(void=float(((f & gr.VOID) != 0).mean()), end=float((((f & gr.END) != 0) & live).mean()), w_above=float((w > 1).mean()),
                w_below=float((w < 1).mean()), expert_played=float(((x != 255) & (a == x))[live].mean()),
                expert_differs=float(((x != 255) & (a != x))[live].mean()), mu_zero=float((want["mu"][live] == 0).mean()))


def check_floors(got, select, explore_threshold):
    """Assert FLOORS on shares(); mu_zero is asked for under GREEDY with eps = 0 only - elsewhere mu > 0 everywhere, which is
    asserted instead."""
    for key, floor in FLOORS.items():
        if key == "mu_zero":
            if select == GREEDY and explore_threshold == 0:
                assert got[key] >= floor, (key, got[key])
            else:
                assert got[key] == 0.0, (key, got[key])
        else:
            assert got[key] >= floor, (key, got[key])
    return got


def worst(got, want):
    """dict output -> the largest |got - want| / bound over the entries with a positive bound.  Where the bound is 0 - void steps,
    the infinite weights - got must equal want exactly (inf == inf): otherwise the share is infinite.  mask must be equal."""
    res = {}
    for name in OUTPUTS:
        g, v, b = np.asarray(got[name], np.float64), want[name], want["bound_" + name]
        exact = b == 0
        if not np.array_equal(g[exact], v[exact]):
            res[name] = float("inf")
            continue
        with np.errstate(invalid="ignore"):
            err = np.abs(g[~exact] - v[~exact])
        res[name] = float((err / b[~exact]).max()) if (~exact).any() else 0.0
        if np.isnan(res[name]):
            res[name] = float("inf")
    res["mask"] = 0.0 if np.array_equal(np.asarray(got["mask"]) != 0, want["mask"] != 0) else float("inf")
    return res


def vtrace32(flags_log, act_log, m_before, m_after, mu_logits, pi_logits=None, expert_log=None, values=None, last_value=None, gamma=GAMMA,
             lam=LAM, w=FLAT, rho_bar=1.0, c_bar=1.0, select=SAMPLE, explore_threshold=0, beta_threshold=0, order=0, wrong=None):
    """A float32 NumPy evaluation of the definition, term by term (no fused multiply-add), in one of three orders:
      0: softmax sums left to right; the backup as the header writes it
      1: softmax sums right to left; the reward summed backwards; D = delta + (gamma c) D+, adv = delta + (gamma rho) D+
      2: softmax sums as pairs; delta = rho r + rho gamma V+ - rho V, distributed; D = (gamma D+) c + delta
    wrong: None, or one of "ends" (ends ignored), "adv_rho" (adv without its rho), "c_lam" (c without lam) - the variants the
    CPU test shows to lie outside the bound."""
    t = np.float32
    f = np.asarray(flags_log)
    K, N = f.shape
    g, lm, rb, cb = t(gamma), t(lam), t(rho_bar), t(c_bar)
    wt = gr.Weights(*(t(x) for x in w))
    eps, beta = explore_threshold / TWO32, beta_threshold / TWO32
    eps4, one_eps, bt, one_bt = t(eps / 4.0), t(1.0 - eps), t(beta), t(1.0 - beta)
    a = np.minimum(np.asarray(act_log), 3).astype(np.int64)
    x = np.full((K, N), 255, np.int64) if expert_log is None else np.asarray(expert_log).astype(np.int64)
    cols = {0: (0, 1, 2, 3), 1: (3, 2, 1, 0)}.get(order)

    def softmax_at(z):
        z = np.asarray(z, t)
        e = np.exp(z - z.max(axis=-1, keepdims=True))
        if cols is None:
            s = (e[..., 0] + e[..., 1]) + (e[..., 2] + e[..., 3])
        else:
            s = e[..., cols[0]]
            for j in cols[1:]:
                s = s + e[..., j]
        return np.take_along_axis(e, a[..., None], -1)[..., 0] / s

    zm = np.asarray(mu_logits, t)
    p_sample = softmax_at(zm)
    pe = (a == zm.argmax(axis=-1)).astype(t) if select == GREEDY else p_sample
    taught = (beta_threshold != 0) & (x != 255)
    inner = np.where(taught, bt * (a == x).astype(t) + one_bt * pe, pe).astype(t)
    mu = (eps4 + one_eps * inner).astype(t)
    pi = p_sample if pi_logits is None else softmax_at(pi_logits)
    with np.errstate(divide="ignore", invalid="ignore"):
        wgt = np.where(mu > 0, pi / np.where(mu > 0, mu, t(1)), t(np.inf)).astype(t)
        log_mu = np.where(mu > 0, np.log(np.where(mu > 0, mu, t(1))), t(-np.inf)).astype(t)
    rho = np.minimum(rb, wgt)
    c = np.minimum(cb, wgt) if wrong == "c_lam" else lm * np.minimum(cb, wgt)
    V = np.zeros((K, N), t) if values is None else np.asarray(values, t)
    VL = np.zeros(N, t) if last_value is None else np.asarray(last_value, t)
    mb, ma = np.asarray(m_before).astype(t), np.asarray(m_after).astype(t)
    out = {k: np.zeros((K, N), t) for k in OUTPUTS}
    out["mask"] = np.zeros((K, N), np.uint8)
    carry = np.zeros(N, t)
    for k in range(K - 1, -1, -1):
        live = (f[k] & gr.VOID) == 0
        end = np.zeros(N, bool) if wrong == "ends" else (f[k] & gr.END) != 0
        flag = lambda bit: ((f[k] & bit) != 0).astype(t)
        terms = [np.full(N, wt.step, t), wt.win * flag(gr.FLAG_SUCCESS), wt.timeout * flag(gr.FLAG_TIMEOUT), wt.invalid * flag(gr.FLAG_INVALID_MOVE),
                 wt.dist * ma[k], wt.progress * (ma[k] - mb[k])]
        r = np.zeros(N, t)
        for term in (terms if order != 1 else terms[::-1]):
            r = r + term
        vplus = np.where(end, t(0), VL if k == K - 1 else V[k + 1]).astype(t)
        if order == 2:
            delta = (rho[k] * r + (rho[k] * g) * vplus) - rho[k] * V[k]
        else:
            delta = rho[k] * ((r + g * vplus) - V[k])
        if order == 0:
            d = delta + g * (c[k] * carry)
            adv = rho[k] * ((r + g * (vplus + carry)) - V[k])
        elif order == 1:
            d = delta + (g * c[k]) * carry
            adv = delta + (g * rho[k]) * carry
        else:
            d = (g * carry) * c[k] + delta
            adv = (rho[k] * g) * carry + delta
        d, adv = np.where(end, delta, d).astype(t), np.where(end, delta, adv).astype(t)
        if wrong == "adv_rho":
            adv = np.where(end, (r + g * vplus) - V[k], (r + g * (vplus + carry)) - V[k]).astype(t)
        carry = np.where(live, d, carry).astype(t)
        out["reward"][k] = np.where(live, r, t(0))
        out["adv"][k] = np.where(live, adv, t(0))
        out["ret"][k] = np.where(live, V[k] + d, t(0))
        out["weight"][k] = np.where(live, wgt[k], t(0))
        out["log_mu"][k] = np.where(live, log_mu[k], t(0))
        out["mask"][k] = live
    return out


# kernel name -> (S, T, obstacles): one case per kernel of the library.  k_traj_vtrace<0> reads no cells, at any size
OCCUPANCY_CASES = {"k_traj_vtrace<0>": (4, 2, 2), **{f"k_traj_vtrace<{S}>": (S, T, K) for S, (T, K) in gr._OCC_SHAPES.items()}}
