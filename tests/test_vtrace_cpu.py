"""The V-trace targets without a GPU: the library's C-ABI (include/tiler_slider_vtrace.h), its launch plan, its code object, the
wrapper's refusals, and the CPU yardstick (tests/vtrace_reference.py): against a scalar recursion that shares no code with it,
against targets_reference.returns64 through the header's two identities, around float32 evaluations in three orders, and
against three wrong variants.  Every test of the yardstick first asserts the floors on its inputs, so that the GPU test cannot pass
on idle input."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from cabi_harness import _declared, _dims, _exported, _instruction_counts, _kernel_metadata, _kernel_names, _scan_last_vgpr, _struct_fields
from conftest import ROOT
from tiler_slider_amd import _vtrace_cabi as vc

MAX_STEPS = 65535
GREEDY, SAMPLE = 0, 1
TWO32 = 1 << 32
INF = float("inf")


def test_vtrace_library_exports_what_its_header_declares():
    from tiler_slider_amd import _cabi, _libraries, _policy_cabi, _targets_cabi
    L = vc.lib()
    assert _exported(vc.LIB_PATH) == _declared("tiler_slider_vtrace.h") == sorted(vc.EXPORTS) and len(vc.EXPORTS) == 5
    assert L.ts_vtrace_abi_version() == vc.ABI_VERSION == 1
    assert vc in _libraries.SINCE and _libraries.name(vc) == "vtrace"
    assert _libraries.SINCE.index(vc) < _libraries.SINCE.index(_libraries._rptable_cabi)
    header = open(os.path.join(ROOT, "include", "tiler_slider_vtrace.h")).read()
    assert int(re.search(r"#define TS_VTRACE_ABI_VERSION (\d+)", header).group(1)) == vc.ABI_VERSION
    for name in ("OUT_REWARD", "OUT_ADV", "OUT_RET", "OUT_MASK", "OUT_WEIGHT", "OUT_LOG_MU", "IN_CELLS", "IN_FIRST", "IN_VALUES", "IN_LAST_VALUE",
                 "IN_EXPERT", "IN_PI"):
        assert int(re.search(rf"#define TS_VTRACE_{name} (0x[0-9a-f]+)u", header).group(1), 16) == getattr(vc, name), name
    bits = [getattr(vc, n) for n in ("OUT_REWARD", "OUT_ADV", "OUT_RET", "OUT_MASK", "OUT_WEIGHT", "OUT_LOG_MU", "IN_CELLS", "IN_FIRST", "IN_VALUES",
                                     "IN_LAST_VALUE", "IN_EXPERT", "IN_PI")]
    assert bits == [1 << i for i in range(12)] and vc.OUT_ALL == 0x3f
    assert (vc.GREEDY, vc.SAMPLE) == (_policy_cabi.GREEDY, _policy_cabi.SAMPLE) == (GREEDY, SAMPLE)
    # the definition, word for word
    prose = re.sub(r"[\s*]+", " ", header)
    for said in ("a = min(act_log[k][n], 3)", "x = expert_log ? expert_log[k][n] : 255", "eps = explore_threshold 2^-32, beta = beta_threshold 2^-32",
                 "TS_POLICY_SAMPLE: softmax(mu_logits[k][n])", "TS_POLICY_GREEDY: 1 at the lowest argmax of mu_logits[k][n], 0 elsewhere",
                 "inner = (beta_threshold != 0 && x != 255) ? beta [a == x] + (1 - beta) p_e[a] : p_e[a]", "mu = eps / 4 + (1 - eps) inner",
                 "pi = softmax(pi_logits ? pi_logits[k][n] : mu_logits[k][n])[a]", "w = mu > 0 ? pi / mu : +infinity",
                 "rho = min(rho_bar, w), c = lam min(c_bar, w)", "void_k: every output 0, mask 0; the carry is left as it is",
                 "delta = rho (r_k + gamma V+_k - V_k)", "D_k = delta + (end_k ? 0 : gamma c D+)", "ret = V_k + D_k",
                 "adv = rho (r_k + gamma (end_k ? 0 : V+_k + D+) - V_k)", "weight = w, log_mu = log(mu) (-infinity where mu == 0), reward = r_k, mask = 1; D+ <- D_k",
                 "A TIMEOUT cuts the bootstrap there, and it cuts it here", "THE SOFTMAX IS THE MODEL", "at most 2^-24",
                 "NOT PART OF THE CONTRACT", "IS THE CORRECTLY ROUNDED IEEE DIVISION", "No atomics are used",
                 "w is exactly 1.0 on every live sample", "`ret` is then ts_traj_returns' ret for every lam, and `adv` is its adv at lam = 1",
                 "A TEMPLATE PARAMETER, NOT A BRANCH"):
        assert said in prose, said
    for struct in ("ts_returns_in", "ts_returns_out", "ts_targets_desc", "ts_policy_cfg"):
        assert not re.search(rf"typedef struct {struct} ", header), struct
    targets_header = open(os.path.join(ROOT, "include", "tiler_slider_targets.h")).read()
    in_fields = _struct_fields(header, "ts_vtrace_in")
    assert in_fields == [f for f, _ in vc.VtraceIn._fields_]
    assert in_fields[:15] == _struct_fields(targets_header, "ts_returns_in") == [f for f, _ in _targets_cabi.ReturnsIn._fields_]
    assert in_fields[15:] == ["act_log", "expert_log", "mu_logits", "pi_logits", "select", "reserved", "explore_threshold", "beta_threshold", "rho_bar", "c_bar"]
    assert _struct_fields(header, "ts_vtrace_out") == [f for f, _ in vc.VtraceOut._fields_] == list(vc.OUT_FIELDS)
    assert list(vc.OUT_FIELDS) == ["reward", "adv", "ret", "weight", "log_mu", "mask"]
    desc_fields = _struct_fields(header, "ts_vtrace_desc")
    assert desc_fields == [f for f, _ in vc.VtraceDesc._fields_]
    assert [f if f != "cells_kernel" else "reserved" for f in desc_fields] == _struct_fields(targets_header, "ts_targets_desc")
    assert (C.sizeof(vc.VtraceIn), C.sizeof(vc.VtraceOut), C.sizeof(vc.VtraceDesc)) == (144, 48, 112)
    assert C.sizeof(vc.VtraceDesc) == C.sizeof(_targets_cabi.TargetsDesc)
    I = vc.VtraceIn
    assert (I.act_log.offset, I.mu_logits.offset, I.select.offset, I.explore_threshold.offset, I.beta_threshold.offset, I.rho_bar.offset, I.c_bar.offset) == \
        (80, 96, 112, 120, 128, 136, 140)
    P = C.c_void_p
    assert L.ts_traj_vtrace.argtypes == [C.POINTER(_cabi.Dims), C.POINTER(_cabi.State), C.POINTER(vc.VtraceIn), C.POINTER(vc.VtraceOut), P]
    proto = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert "int32_t ts_traj_vtrace(const ts_dims *dims, const ts_state *st, const ts_vtrace_in *in, const ts_vtrace_out *out, void *stream);" in proto
    assert "int32_t ts_describe_traj_vtrace(const ts_dims *dims, int32_t steps, uint32_t what, ts_vtrace_desc *desc);" in proto
    assert "int32_t ts_vtrace_supported(const ts_dims *dims);" in proto
    import tiler_slider_amd
    assert callable(tiler_slider_amd.build_vtrace_library) and {"build_vtrace_library", "VtraceTargets"} <= set(tiler_slider_amd.__all__)
    assert tiler_slider_amd.VtraceTargets._fields == ("reward", "adv", "ret", "mask", "weight", "log_mu")
    vt = tiler_slider_amd.VtraceTargets(1, 2, 3, 4, 5, 6)
    assert isinstance(vt.returns, tiler_slider_amd.TrajectoryReturns) and tuple(vt.returns) == (1, 2, 3, 4)
    import __graft_entry__ as entry
    assert callable(entry._smoke_vtrace)


def test_vtrace_supported_is_targets_supported_for_the_returns():
    from tiler_slider_amd import _cabi, _targets_cabi as gc
    L, LG = vc.lib(), gc.lib()
    seen = set()
    for S in range(0, 11):
        for T in range(-1, 11):
            for Tt in (0, T, 9):
                for mc in (0, 1, 2):
                    d = _dims(S, T, mc, Tt=Tt)
                    got = L.ts_vtrace_supported(C.byref(d))
                    assert got == LG.ts_targets_supported(C.byref(d), gc.RETURNS), (S, T, Tt, mc)
                    seen.add(got)
    assert seen == {0, 1, _cabi.ERR_DIMS}
    assert L.ts_vtrace_supported(None) == _cabi.ERR_NULL and L.ts_vtrace_supported(C.byref(_dims(33, 2))) == 0
    assert vc.vtrace_supported(_dims(8, 8)) and not vc.vtrace_supported(_dims(9, 1))
    with pytest.raises(_cabi.TilerSliderLibraryError):
        vc.vtrace_supported(_dims(0, 1))


def _in(p, steps=3, stride=1, gamma=0.5, lam=0.5, w=(0, 1, 0, 0, 0, 0), select=SAMPLE, eps=0, beta=0, rho_bar=1.0, c_bar=1.0, **ptr):
    get = lambda k, default: ptr.get(k, default)
    return vc.VtraceIn(get("first", None), get("pos_log", None), get("flags_log", p), get("values", None), get("last_value", None), steps, stride,
                       gamma, lam, *w, get("act_log", p), get("expert_log", None), get("mu_logits", p), get("pi_logits", None), select, 0, eps, beta,
                       rho_bar, c_bar)


def test_argument_validation_precedes_any_launch():
    """Every refusal below returns its own status, in the header's order: a HIP call on a box without a GPU would have answered
    TS_ERR_HIP."""
    from tiler_slider_amd import _cabi
    L = vc.lib()
    ok, empty = _dims(4, 2), _dims(4, 2, 0, 0)
    buf = (C.c_uint8 * 8192)()
    p = (C.addressof(buf) + 15) & ~15
    st = _cabi.State(None, None, p, None, None, None, None)
    nothing = vc.VtraceOut(*([None] * 6))
    out = lambda **kw: vc.VtraceOut(*(kw.get(f, p if f == "ret" else None) for f in vc.OUT_FIELDS))
    ref = lambda x: C.byref(x) if x is not None else None
    call = lambda d, s, i, o: L.ts_traj_vtrace(ref(d), ref(s), ref(i), ref(o), None)
    nan = float("nan")
    # 1. dims - its TS_ERR_LIMIT before the NULL checks
    assert call(None, st, _in(p), out()) == _cabi.ERR_NULL
    assert call(_dims(0, 2), st, None, None) == _cabi.ERR_DIMS
    assert call(_dims(33, 2), st, None, None) == _cabi.ERR_LIMIT
    # 2. in / out
    assert call(ok, st, None, out()) == _cabi.ERR_NULL
    assert call(ok, st, _in(p), None) == _cabi.ERR_NULL
    assert call(_dims(9, 1), st, None, out()) == _cabi.ERR_NULL          # before the shape
    # 3. an unsupported shape, before the arguments
    for S, T, Tt in ((9, 1, 1), (16, 2, 2), (8, 9, 2), (4, 2, 9)):
        assert call(_dims(S, T, Tt=Tt), st, _in(p, steps=0), out()) == _cabi.ERR_LIMIT, (S, T, Tt)
    # 4. bad arguments, before the empty batch and before any pointer
    for d in (ok, empty):
        for bad in (dict(steps=0), dict(steps=-1), dict(steps=MAX_STEPS + 1), dict(select=2), dict(select=-1), dict(eps=TWO32 + 1), dict(beta=TWO32 + 1),
                    dict(gamma=-0.01), dict(gamma=1.01), dict(gamma=nan), dict(lam=-0.01), dict(lam=1.01), dict(lam=nan), dict(rho_bar=-1e-9),
                    dict(rho_bar=nan), dict(rho_bar=-INF), dict(c_bar=-1.0), dict(c_bar=nan), dict(stride=0), dict(stride=2), dict(stride=3), dict(stride=8)):
            assert call(d, None, _in(None, **bad), nothing) == _cabi.ERR_ARG, bad
    # ... the edges are arguments: they get as far as the pointers
    edges = dict(steps=MAX_STEPS, select=GREEDY, eps=TWO32, beta=TWO32, gamma=1.0, lam=0.0, rho_bar=INF, c_bar=0.0, stride=4)
    assert call(ok, None, _in(None, **edges), nothing) == _cabi.ERR_NULL
    # 5. nothing to do: TS_OK without a launch, no pointer is looked at
    assert call(empty, None, _in(None, flags_log=None, act_log=None, mu_logits=None), nothing) == _cabi.OK
    # 6. missing pointers, before the alignment (p + 4: a misaligned mu_logits; p + 1: a misaligned output)
    bad_out = out(ret=p + 1)
    cells, progress = (0, 1, 0, 0, 1, 0), (0, 1, 0, 0, 0, 1)
    for missing in ("flags_log", "act_log", "mu_logits"):
        assert call(ok, None, _in(p, **{missing: None, **({} if missing == "mu_logits" else dict(mu_logits=p + 4))}), bad_out) == _cabi.ERR_NULL, missing
    assert call(ok, None, _in(p, mu_logits=p + 4), nothing) == _cabi.ERR_NULL                                # no output at all
    assert call(ok, st, _in(p, mu_logits=p + 4, w=cells), bad_out) == _cabi.ERR_NULL                           # pos_log
    assert call(ok, st, _in(p, mu_logits=p + 4, w=progress, pos_log=p), bad_out) == _cabi.ERR_NULL             # first
    assert call(ok, None, _in(p, mu_logits=p + 4, w=cells, pos_log=p), bad_out) == _cabi.ERR_NULL              # st
    assert call(ok, _cabi.State(), _in(p, mu_logits=p + 4, w=cells, pos_log=p), bad_out) == _cabi.ERR_NULL     # st->tgt
    assert call(ok, st, _in(p, mu_logits=p + 4, w=cells, pos_log=p), bad_out) == _cabi.ERR_ARG                 # all there: on to the alignment
    assert call(_dims(4, 2, Tt=0), None, _in(p, mu_logits=p + 4, w=cells, pos_log=p), bad_out) == _cabi.ERR_ARG   # no targets: no st
    assert call(_dims(4, 0), None, _in(p, mu_logits=p + 4, w=progress), bad_out) == _cabi.ERR_ARG              # no tiles: no cells
    assert call(ok, None, _in(p, mu_logits=p + 4), bad_out) == _cabi.ERR_ARG                                  # flat weights: no cells, no st
    # 7. alignment: 16 bytes for the logits, 4 for every other float pointer
    for off in (4, 8, 12):
        assert call(ok, None, _in(p, mu_logits=p + off), out()) == _cabi.ERR_ARG
        assert call(ok, None, _in(p, pi_logits=p + off), out()) == _cabi.ERR_ARG
    for off in (1, 2, 3):
        assert call(ok, None, _in(p, values=p + off), out()) == _cabi.ERR_ARG
        assert call(ok, None, _in(p, last_value=p + off), out()) == _cabi.ERR_ARG
        for f in ("reward", "adv", "ret", "weight", "log_mu"):
            assert call(ok, None, _in(p), out(**{f: p + off})) == _cabi.ERR_ARG, f
    assert L.ts_vtrace_last_hip_error() == 0
    # the describe call: the same plan
    d_ = vc.VtraceDesc()
    desc = lambda d, steps, what, to=d_: L.ts_describe_traj_vtrace(ref(d), steps, what, ref(to))
    assert desc(None, 3, 1) == _cabi.ERR_NULL and desc(ok, 3, 1, None) == _cabi.ERR_NULL
    assert desc(_dims(0, 2), 3, 1) == _cabi.ERR_DIMS and desc(_dims(33, 2), 3, 1) == _cabi.ERR_LIMIT and desc(_dims(9, 1), 0, 0) == _cabi.ERR_LIMIT
    for steps, what in ((0, 1), (MAX_STEPS + 1, 1), (3, 0), (3, vc.IN_CELLS | vc.IN_PI), (3, 1 | 0x1000), (3, 0x80000001)):
        assert desc(ok, steps, what) == _cabi.ERR_ARG and desc(empty, steps, what) == _cabi.ERR_ARG, (steps, what)
    got = vc.describe_traj_vtrace(empty, 7)
    assert (got["blocks"], got["name"], got["samples"], got["bytes_read"], got["bytes_written"], got["chunk_steps"] >= 1) == (0, "", 0, 0, 0, True)


def test_describe_names_exactly_the_compiled_kernels_with_the_plan_restated():
    import vtrace_reference as vr
    compiled = _kernel_names(vc.LIB_PATH)
    assert len(compiled) == vc.MIN_KERNELS == 9 and sorted(vr.OCCUPANCY_CASES) == compiled
    named = set()
    every_in = vc.IN_CELLS | vc.IN_FIRST | vc.IN_VALUES | vc.IN_LAST_VALUE | vc.IN_EXPERT | vc.IN_PI
    chunk = vc.describe_traj_vtrace(_dims(4, 2), 1)["chunk_steps"]
    assert 2 <= chunk <= 16
    for S in range(1, 9):
        for T in range(0, min(S * S, 8) + 1):
            for Tt in (0, T):
                for n, K in ((1, 1), (257, 5), (1 << 20, 100)):
                    dims = _dims(S, T, S % 2, n, Tt=Tt)
                    for what, cells, first in ((vc.OUT_ALL, 0, 0), (vc.OUT_ALL | every_in, 1, 1), (vc.OUT_RET | vc.IN_CELLS, 1, 0), (vc.OUT_MASK | vc.IN_FIRST, 1, 1),
                                               (vc.OUT_ADV | vc.OUT_WEIGHT | vc.IN_VALUES | vc.IN_PI, 0, 0)):
                        d = vc.describe_traj_vtrace(dims, K, what)
                        kernel = S if cells and T > 0 else 0
                        assert d["name"] == f"k_traj_vtrace<{kernel}>" and d["cells_kernel"] == (1 if kernel else 0), (S, T, what, d)
                        assert (d["threads_per_block"], d["lds_bytes"], d["chunk_steps"], d["blocks"], d["samples"]) == (256, 0, chunk, -(-n // 256), K * n)
                        bit = lambda b: 1 if what & b else 0
                        read = K * n * (18 + bit(vc.IN_EXPERT) + 16 * bit(vc.IN_PI) + 4 * bit(vc.IN_VALUES)) + cells * ((K + first) * T * n + Tt * n) \
                            + 4 * n * bit(vc.IN_LAST_VALUE)
                        written = K * n * (4 * sum(bit(b) for b in (vc.OUT_REWARD, vc.OUT_ADV, vc.OUT_RET, vc.OUT_WEIGHT, vc.OUT_LOG_MU)) + bit(vc.OUT_MASK))
                        assert (d["bytes_read"], d["bytes_written"]) == (read, written), (S, T, Tt, n, K, what)
                        named.add(d["name"])
    assert sorted(named) == compiled


def test_every_vtrace_kernel_keeps_its_chunk_in_registers():
    """The code object's own metadata and instructions: no private segment (scratch), no scratch_ instruction, no static LDS, no
    LDS instruction, no barrier, no accumulation registers, no atomics, and the hazard scan clean over all nine kernels."""
    kernels = _kernel_metadata(vc.LIB_PATH)
    assert len(kernels) == len([k for k in kernels if "k_traj_vtrace" in k["name"]]) == vc.MIN_KERNELS
    assert not any(k["group_segment_fixed_size"] or k["private_segment_fixed_size"] or k["agpr_count"] or k["uses_dynamic_stack"] for k in kernels), kernels
    print("vgprs:", {k["name"][-12:]: k["vgpr_count"] for k in kernels})
    assert max(k["vgpr_count"] for k in kernels) <= 168      # three waves per SIMD at the least
    flat = [k for k in kernels if "ILi0E" in k["name"] or "<0>" in k["name"]]
    assert len(flat) == 1 and flat[0]["vgpr_count"] <= 80      # six waves per SIMD in the kernel without cells
    pats = (r"\bscratch_\w+", r"\bs_barrier\b", r"\bds_\w+", r"atomic", r"cmpswap", r"global_load_dwordx4", r"v_exp_f32", r"v_div_fixup_f32")
    mine = {k: v for k, v in _instruction_counts(vc.LIB_PATH, pats).items() if "k_traj_vtrace" in k}
    assert len(mine) == vc.MIN_KERNELS
    for k, (n_scratch, n_barrier, n_ds, n_atomic, n_cas, n_x4, n_exp, n_div) in mine.items():
        assert n_scratch == n_barrier == n_ds == n_atomic == n_cas == 0, (k, n_scratch, n_barrier, n_ds, n_atomic, n_cas)
        assert n_x4 > 0 and n_exp > 0 and n_div > 0, (k, n_x4, n_exp, n_div)     # 16-byte logits rows; the hardware's exp; the IEEE division's last step
    class_a, class_b, n_kernels = _scan_last_vgpr(vc.LIB_PATH)
    assert n_kernels == vc.MIN_KERNELS and class_a == [] and class_b == []


def test_the_source_restates_the_reward_and_includes_no_other_library():
    src = open(vc.SRC).read()
    assert '#include "../../include/tiler_slider_vtrace.h"' in src and '#include "ts_launch.h"' in src
    for other in ("ts_targets.hip", "ts_policy.hip", "ts_mixed.hip", "ts_loss.hip", "ts_mlp.h"):
        assert f'#include "{other}"' not in src
    assert "__expf" in src and "__logf" in src and "atomic" not in src.lower().replace("no atomics", "")
    assert "manhattan" in src and "reward_of" in src
    assert os.path.join(ROOT, "include", "tiler_slider_targets.h") in vc.HEADERS


def test_the_wrapper_refuses_what_it_cannot_compute():
    """trajectory_vtrace's arguments, checked before any device is touched (the environment is never constructed)."""
    import inspect
    from tiler_slider_amd import VecTilerSliderEnv, vtrace
    sig = inspect.signature(VecTilerSliderEnv.trajectory_vtrace)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("rollout", inspect.Parameter.empty), ("logits", None), ("values", None), ("last_value", None), ("gamma", 0.99), ("lam", 1.0), ("rho_bar", 1.0),
        ("c_bar", 1.0), ("select", "sample"), ("epsilon", 0.0), ("beta", 0.0), ("reward", None)]
    env = object.__new__(VecTilerSliderEnv)
    for kw, match in ((dict(gamma=1.5), "gamma"), (dict(lam=-0.1), "lam"), (dict(rho_bar=-1.0), "rho_bar"), (dict(c_bar=float("nan")), "c_bar"),
                      (dict(select="argmax"), "select"), (dict(epsilon=1.5), "epsilon"), (dict(beta=-0.5), "beta")):
        with pytest.raises(ValueError, match=match):
            env.trajectory_vtrace(None, **kw)
    with pytest.raises(TypeError, match="RewardWeights"):
        env.trajectory_vtrace(None, reward=(0, 1, 0, 0, 0, 0))
    assert [vtrace._threshold(x, "x") for x in (0.0, 0.125, 0.5, 1.0, 0.1)] == [0, 1 << 29, 1 << 31, 1 << 32, int(round(0.1 * 2**32))]


# ---------------------------------------------------------------------------------------------- the yardstick and its inputs
def _run(vr, c, K, eps, beta, select, fn=None, **kw):
    i = vr.inputs(c, K)
    args = dict(pi_logits=i["pi_logits"], expert_log=i["expert_log"], values=i["values"], last_value=i["last_value"], select=select,
                explore_threshold=vr.threshold_of(eps), beta_threshold=vr.threshold_of(beta))
    args.update(kw)
    return i, (fn or vr.vtrace64)(i["flags_log"], i["act_log"], i["m_before"], i["m_after"], i["mu_logits"], **args)


def _floors(vr, i, want, select, eps):
    return vr.check_floors(vr.shares(want, i["flags_log"], i["act_log"], i["expert_log"]), select, vr.threshold_of(eps))


def _scalar(i, n, K, N, gamma, lam, w, rho_bar, c_bar, select, eps_t, beta_t, with_pi):
    """Board n by the header, in plain Python floats: lists of (reward, adv, ret, weight, log_mu, mask) per step."""
    eps, beta = eps_t / 2.0 ** 32, beta_t / 2.0 ** 32
    gamma, lam = float(np.float32(gamma)), float(np.float32(lam))
    w = [float(np.float32(x)) for x in w]
    rows, carry = [None] * K, 0.0
    for k in range(K - 1, -1, -1):
        fl = int(i["flags_log"][k, n])
        if fl & (0x10 | 0x20 | 0x40):
            rows[k] = (0.0, 0.0, 0.0, 0.0, 0.0, 0)
            continue
        end = bool(fl & (0x04 | 0x08))
        a = min(int(i["act_log"][k, n]), 3)
        x = int(i["expert_log"][k, n])
        soft = lambda z: [math.exp(float(v) - max(float(u) for u in z)) / sum(math.exp(float(u) - max(float(t) for t in z)) for u in z) for v in z]
        zm = i["mu_logits"][k, n]
        if select == SAMPLE:
            pe = soft(zm)[a]
        else:
            best = [j for j in range(4) if float(zm[j]) == max(float(u) for u in zm)][0]
            pe = 1.0 if a == best else 0.0
        inner = beta * (1.0 if a == x else 0.0) + (1 - beta) * pe if (beta_t != 0 and x != 255) else pe
        mu = eps / 4 + (1 - eps) * inner
        pi = soft(i["pi_logits"][k, n] if with_pi else zm)[a]
        wgt = pi / mu if mu > 0 else INF
        rho, c = min(rho_bar, wgt), lam * min(c_bar, wgt)
        ma, mb = float(i["m_after"][k, n]), float(i["m_before"][k, n])
        r = w[0] + (w[1] if fl & 0x04 else 0.0) + (w[2] if fl & 0x08 else 0.0) + (w[3] if fl & 0x02 else 0.0) + w[4] * ma + w[5] * (ma - mb)
        V = float(i["values"][k, n])
        vplus = 0.0 if end else float(i["last_value"][n] if k == K - 1 else i["values"][k + 1, n])
        delta = rho * (r + gamma * vplus - V)
        d = delta + (0.0 if end else gamma * c * carry)
        adv = rho * (r + gamma * (0.0 if end else vplus + carry) - V)
        rows[k] = (r, adv, V + d, wgt, math.log(mu) if mu > 0 else -INF, 1)
        carry = d
    return rows


@pytest.mark.parametrize("select", (GREEDY, SAMPLE), ids=("greedy", "sample"))
@pytest.mark.parametrize("eps,beta", ((0.125, 0.5), (0.0, 0.5)))
def test_the_yardstick_is_the_scalar_recursion(oracle, eps, beta, select):
    """Every fourth board of "auto" and of "mc5" (with the cell weights), step by step in Python floats, against the vectorised
    yardstick: equal to 1e-12 relative, infinities in the same places."""
    import targets_reference as gr
    import vtrace_reference as vr
    for name, w in (("auto", vr.FLAT), ("mc5", vr.WEIGHTS)):
        c = gr.trajectory(oracle, name)
        i, want = _run(vr, c, c["K"], eps, beta, select, w=w)
        if name == "auto":
            _floors(vr, i, want, select, eps)
        for n in range(0, c["n"], 4):
            rows = _scalar(i, n, c["K"], c["n"], vr.GAMMA, vr.LAM, w, 1.0, 1.0, select, vr.threshold_of(eps), vr.threshold_of(beta), True)
            for j, key in enumerate(("reward", "adv", "ret", "weight", "log_mu", "mask")):
                mine, theirs = np.array([row[j] for row in rows], np.float64), want[key][:, n].astype(np.float64)
                fin = np.isfinite(theirs)
                assert np.array_equal(mine[~fin], theirs[~fin]) and np.allclose(mine[fin], theirs[fin], rtol=1e-12, atol=1e-13), (name, n, key)


@pytest.mark.parametrize("name", ("auto", "strict", "given", "long", "mc5", "s8"))
def test_on_policy_the_weights_are_one_and_the_targets_are_the_returns(oracle, name):
    """The header's two identities on the trajectories of targets_reference.CASES: pi_logits NULL, both thresholds 0, SAMPLE - w is
    exactly 1.0 in float64 and in the three float32 evaluations; with the bars at 1, 2.5 and +infinity `ret` is returns64's ret for
    every lam and, at lam = 1, `adv` is its adv (at another lam, adv bootstraps from the next step's lam-weighted target)."""
    import targets_reference as gr
    import vtrace_reference as vr
    c = gr.trajectory(oracle, name)
    i = vr.inputs(c)
    f32 = lambda x: float(np.float32(x))      # both yardsticks on the numbers the call receives
    w = gr.Weights(*(f32(x) for x in vr.WEIGHTS))
    base = (i["flags_log"], i["act_log"], i["m_before"], i["m_after"], i["mu_logits"])
    for lam in (0.0, f32(0.9), 1.0):
        ref = gr.returns64(i["flags_log"], i["m_before"], i["m_after"], i["values"], i["last_value"], f32(vr.GAMMA), lam, w)
        ref1 = gr.returns64(i["flags_log"], i["m_before"], i["m_after"], i["values"], i["last_value"], f32(vr.GAMMA), 1.0, w)
        for bar in (1.0, 2.5, INF):
            got = vr.vtrace64(*base, values=i["values"], last_value=i["last_value"], lam=lam, w=w, rho_bar=bar, c_bar=bar)
            live = got["live"]
            assert np.array_equal(live, ref["mask"] != 0) and (got["weight"][live] == 1.0).all() and (got["weight"][~live] == 0).all()
            np.testing.assert_allclose(got["ret"], ref["ret"], rtol=1e-12, atol=1e-12)
            if lam == 1.0:
                np.testing.assert_allclose(got["adv"], ref1["adv"], rtol=1e-12, atol=1e-12)
            np.testing.assert_array_equal(got["reward"], ref["reward"])
    for order in (0, 1, 2):
        got = vr.vtrace32(*base, values=i["values"], last_value=i["last_value"], w=w, order=order)
        assert (got["weight"][got["mask"] != 0] == 1.0).all(), order


@pytest.mark.parametrize("select", (GREEDY, SAMPLE), ids=("greedy", "sample"))
@pytest.mark.parametrize("eps,beta", ((0.125, 0.5), (0.0, 0.5)))
@pytest.mark.parametrize("name", ("auto", "strict", "given", "long"))
def test_float32_evaluations_in_three_orders_lie_within_the_bound_and_three_wrong_ones_do_not(oracle, name, eps, beta, select):
    import targets_reference as gr
    import vtrace_reference as vr
    c = gr.trajectory(oracle, name)
    i, want = _run(vr, c, c["K"], eps, beta, select)
    print(name, eps, beta, select, _floors(vr, i, want, select, eps))
    for order in (0, 1, 2):
        _, got = _run(vr, c, c["K"], eps, beta, select, fn=vr.vtrace32, order=order)
        share = vr.worst(got, want)
        print(f"{name} eps={eps} beta={beta} select={select} order={order}: worst share of the bound "
              + ", ".join(f"{k} {v:.3f}" for k, v in share.items() if k != "mask"))
        assert max(share.values()) <= 1.0, (order, share)
    for wrong, keys in (("ends", ("adv", "ret")), ("adv_rho", ("adv",)), ("c_lam", ("adv", "ret"))):
        _, got = _run(vr, c, c["K"], eps, beta, select, fn=vr.vtrace32, wrong=wrong)
        share = vr.worst(got, want)
        assert all(share[k] > 1.0 for k in keys) and share["weight"] <= 1.0 and share["reward"] <= 1.0, (wrong, share)


@pytest.mark.parametrize("name", ("mc5", "s8"))
def test_the_cell_cases_lie_within_the_bound_with_all_six_weights(oracle, name):
    import targets_reference as gr
    import vtrace_reference as vr
    c = gr.trajectory(oracle, name)
    assert all(x != 0 for x in vr.WEIGHTS)
    for select in (GREEDY, SAMPLE):
        i, want = _run(vr, c, c["K"], 0.125, 0.5, select, w=vr.WEIGHTS)
        assert (i["m_after"] != 0).any() and (i["m_after"] != i["m_before"]).any()
        for order in (0, 1, 2):
            _, got = _run(vr, c, c["K"], 0.125, 0.5, select, fn=vr.vtrace32, order=order, w=vr.WEIGHTS)
            share = vr.worst(got, want)
            print(f"{name} select={select} order={order}: " + ", ".join(f"{k} {v:.3f}" for k, v in share.items() if k != "mask"))
            assert max(share.values()) <= 1.0, (order, share)
