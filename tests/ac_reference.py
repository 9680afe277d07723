"""CPU yardstick of the actor-critic network (test infrastructure, no test of its own): the definition of
include/tiler_slider_ac.h restated on NumPy by extending tests/train_reference.py.  The value head is stacked as a FIFTH ROW of
w2 (and a fifth entry of b2, a fifth column of dz): forward64, logits64, grads64, exactness_guard and torch_grads64 of
train_reference are written for any number of outputs, so the five-output network goes through them unchanged and the results
are split again.  (The LIBRARY keeps wv and bv apart from w2 and b2; only this yardstick stacks them.)  It shares no code with
tiler_slider_amd/csrc/ts_ac.hip and imports neither torch nor the libraries at import time.  Networks are in torch.nn.Linear's
layout (w1 [H, D], b1 [H], w2 [4, H], b2 [4]; head = (wv [H], bv [1])); gradients come back in the KERNEL layout.

THE GRADIENT BOUND is train_reference's with one change: dh^ is an inner product of FIVE exact terms, so
d = gamma_5 (sum_a |w2[j][a]| |dz_a| + |wv[j]| |dv|).  The bound of gw2 - sum e |dz_a| + gamma_{M+1} sum (|h| + e) |dz_a| - is
formed for all five columns; its fifth is the bound of gwv, and gb2's fifth entry the bound of gbv."""
import numpy as np

import train_reference as tr

gamma = tr.gamma
NAMES = ("w1", "b1", "w2", "b2", "wv", "bv")


def int_head(rng, H, lo=-2, hi=2):
    """Integer (wv [H], bv [1]) in [lo, hi]."""
    return rng.integers(lo, hi + 1, H).astype(np.float32), rng.integers(lo, hi + 1, 1).astype(np.float32)


def random_head(rng, H):
    return rng.standard_normal(H).astype(np.float32), rng.standard_normal(1).astype(np.float32)


def stack(mlp, head):
    """The five-output network: wv the fifth row of w2, bv the fifth entry of b2."""
    w1, b1, w2, b2 = mlp
    wv, bv = head
    return w1, b1, np.concatenate([w2, np.asarray(wv).reshape(1, -1)], axis=0), np.concatenate([b2, np.asarray(bv).reshape(1)])


def stack_cotangents(dz, dv):
    """[M, 5]: dv the fifth column of dz [M, 4]."""
    return np.concatenate([np.asarray(dz), np.asarray(dv).reshape(-1, 1)], axis=1)


def split(g):
    """A dict of train_reference's four gradients of the five-output network -> the six of the header, kernel layout."""
    return {"w1": g["w1"], "b1": g["b1"], "w2": np.ascontiguousarray(g["w2"][:, :4]), "b2": np.ascontiguousarray(g["b2"][:4]),
            "wv": np.ascontiguousarray(g["w2"][:, 4]), "bv": np.ascontiguousarray(g["b2"][4:5])}


def kernel_layout(mlp, head):
    """(w1 [D, H], b1 [H], w2 [H, 4], b2 [4], wv [H], bv [1])."""
    return tr.kernel_layout(mlp) + (np.ascontiguousarray(head[0]), np.ascontiguousarray(head[1]))


def outputs64(x, mlp, head):
    """(z [M, 4], zbound, v [M], vbound): float64 values and policy_reference's per-output bound on any float32 evaluation."""
    z, bound = tr.logits64(x, stack(mlp, head))
    return z[:, :4], bound[:, :4], z[:, 4], bound[:, 4]


def grads64(x, mlp, head, dz, dv, relu_at_zero=0.0):
    """The six gradients of the header in float64, kernel layout."""
    return split(tr.grads64(x, stack(mlp, head), stack_cotangents(dz, dv), relu_at_zero))


def torch_grads64(x, mlp, head, dz, dv):
    """float64 torch autograd of the dense five-output network."""
    return split(tr.torch_grads64(x, stack(mlp, head), stack_cotangents(dz, dv)))


def grad_bounds(x, mlp, head, dz, dv):
    """(bounds, ambiguous) as train_reference.grad_bounds, for the six gradients: gamma(5) in the bound of dh, the w2 and b2 bounds
    over five columns."""
    s = stack(mlp, head)
    w2 = np.abs(np.asarray(s[2], np.float64))         # [5, H]
    d5 = np.asarray(stack_cotangents(dz, dv), np.float64)
    x, adz = np.asarray(x, np.float64), np.abs(d5)
    M = x.shape[0]
    pre, h, _, e = tr.forward64(x, s)
    dh = np.abs(d5 @ np.asarray(s[2], np.float64))
    d = gamma(5) * (adz @ w2)
    ambiguous = np.abs(pre) <= e
    eps = d + np.where(ambiguous, dh, 0.0)            # |dp^ - dp|
    mag = dh + d                                      # |dp^|
    count = x.sum(axis=0)
    bounds = {
        "b2": gamma(M) * adz.sum(axis=0),
        "w2": e.T @ adz + gamma(M + 1) * ((np.abs(h) + e).T @ adz),
        "b1": eps.sum(axis=0) + gamma(M) * mag.sum(axis=0),
        "w1": x.T @ eps + gamma(count)[:, None] * (x.T @ mag),
    }
    return split(bounds), ambiguous


def stack_prefill(prefill):
    return {"w1": prefill["w1"], "b1": prefill["b1"], "w2": np.concatenate([prefill["w2"], prefill["wv"].reshape(-1, 1)], axis=1),
            "b2": np.concatenate([prefill["b2"], prefill["bv"].reshape(1)])}


def exactness_guard(x, mlp, head, dz, dv, prefill=None):
    """train_reference.exactness_guard extended to the fifth column: integer inputs, every sum of absolute terms below 2**24 -
    for the value and the gradients of wv and bv too."""
    return tr.exactness_guard(x, stack(mlp, head), stack_cotangents(dz, dv), None if prefill is None else stack_prefill(prefill))


# kernel name -> (S, T, obstacles): OCCUPANCY_CASES' shapes, one case per kernel of the actor-critic library
OCCUPANCY_CASES = {name.replace("k_train_", "k_ac_"): shape for name, shape in tr.OCCUPANCY_CASES.items()}

BACKWARD_CASES = tr.BACKWARD_CASES
BACKWARD_HK = tr.BACKWARD_HK


def backward_case(orc, case, H, K, n=tr.N_BOARDS):
    """train_reference.backward_case - levels, cells, network, dz, prefill - with a value head, dv in {-1, 0, 1} and prefills of
    gwv and gbv added, the yardstick's answer for all six gradients, and the assertions that the case bites on the yardstick's own
    numbers: a non-zero wv gradient, a ReLU kink with a non-zero FIVE-term dh, a shared cell in single colour, and a gradient of
    w1 that changes when dv is dropped (the value path reaches the trunk).  The head and dv are redrawn (a fixed sequence of
    seeds) until they do.  H may be any width, not only BACKWARD_HK's."""
    c = tr.backward_case(orc, case, H, K, n)
    S, T, Tt, Ko, mc, what, _ = tr.BACKWARD_CASES[case]
    C = S * S
    rng = np.random.default_rng(77000 + 10000 * case + 100 * H + K)
    x, mlp = c["x"], c["mlp"]
    flat = c["dz"].reshape(K * n, 4)
    want_kink = not (C == 1 and H == 1)
    pre = tr.forward64(x, mlp)[0]
    for attempt in range(64):
        head = int_head(rng, H)
        dv = rng.integers(-1, 2, (K, n)).astype(np.float32)
        g = grads64(x, mlp, head, flat, dv.reshape(-1))
        dh = stack_cotangents(flat, dv.reshape(-1)).astype(np.float64) @ stack(mlp, head)[2].astype(np.float64)
        bites = float(((pre == 0) & (dh != 0)).mean())
        reaches = bool((grads64(x, mlp, head, flat, np.zeros(K * n, np.float32))["w1"] != g["w1"]).any())
        if (bites >= 0.01 or not want_kink) and g["wv"].any() and reaches:
            break
    prefill = dict(c["prefill"])
    prefill["wv"], prefill["bv"] = rng.integers(-3, 4, H).astype(np.float32), rng.integers(-3, 4, 1).astype(np.float32)
    exactness_guard(x, mlp, head, flat, dv.reshape(-1), prefill)
    want = {name: (prefill[name].astype(np.float64) + g[name]).astype(np.float32) for name in NAMES}
    ctx = (case, H, K)
    assert bites >= 0.01 or not want_kink, (ctx, bites)
    assert g["wv"].any(), (ctx, "no wv gradient")
    assert reaches, (ctx, "dv does not reach w1")
    if T >= 2 and not mc:
        assert c["shared"] >= 0.01, (ctx, c["shared"])
    v = outputs64(x, mlp, head)[2]
    out = dict(c)
    out.update(head=head, dv=dv, prefill=prefill, want=want, values=v.astype(np.float32).reshape(K, n), bites=bites, wv_grad=bool(g["wv"].any()),
               reaches=reaches)
    return out
