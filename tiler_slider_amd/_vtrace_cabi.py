"""ctypes binding of lib/libtiler_slider_vtrace.so — the V-trace targets' C-ABI declared in include/tiler_slider_vtrace.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES; it is an entry of _libraries.SINCE, which says why it is not one of LIBRARIES.  There is no CPU fallback:
if the library is missing or does not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi, _targets_cabi
from ._cabi import Desc, Dims, State
from ._policy_cabi import GREEDY, SAMPLE, SELECTS

SRC = os.path.join(_cabi._PKG, "csrc", "ts_vtrace.hip")
HEADERS = _targets_cabi.HEADERS + [os.path.join(_cabi.ROOT, "include", "tiler_slider_vtrace.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_vtrace.so")
HEADER, PREFIX, LABEL = "tiler_slider_vtrace.h", "ts_vtrace_", "vtrace "

ABI_VERSION = 1
MIN_KERNELS = 9  # k_traj_vtrace<0 .. 8>: what compile_guarded must find

OUT_REWARD, OUT_ADV, OUT_RET, OUT_MASK, OUT_WEIGHT, OUT_LOG_MU = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
IN_CELLS, IN_FIRST, IN_VALUES, IN_LAST_VALUE, IN_EXPERT, IN_PI = 0x40, 0x80, 0x100, 0x200, 0x400, 0x800
OUT_ALL = OUT_REWARD | OUT_ADV | OUT_RET | OUT_MASK | OUT_WEIGHT | OUT_LOG_MU

EXPORTS = ("ts_vtrace_abi_version", "ts_vtrace_last_hip_error", "ts_vtrace_supported", "ts_traj_vtrace", "ts_describe_traj_vtrace")


class VtraceIn(C.Structure):
    """ts_vtrace_in: ts_returns_in's fields, the actions, the expert's moves, the behaviour and the target logits, and how the
    rollout selected: select, the two thresholds; then the two bars."""
    _fields_ = _targets_cabi.ReturnsIn._fields_ + [
        ("act_log", C.c_void_p), ("expert_log", C.c_void_p), ("mu_logits", C.c_void_p), ("pi_logits", C.c_void_p), ("select", C.c_int32),
        ("reserved", C.c_int32), ("explore_threshold", C.c_uint64), ("beta_threshold", C.c_uint64), ("rho_bar", C.c_float), ("c_bar", C.c_float)]


OUT_FIELDS = ("reward", "adv", "ret", "weight", "log_mu", "mask")


class VtraceOut(C.Structure):
    """ts_vtrace_out: float32 [K][N] reward, adv, ret, weight, log_mu and uint8 [K][N] mask; each optional."""
    _fields_ = [(name, C.c_void_p) for name in OUT_FIELDS]


class VtraceDesc(Desc):
    """ts_vtrace_desc: what one ts_traj_vtrace would launch."""
    _fields_ = [("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32), ("chunk_steps", C.c_int32), ("cells_kernel", C.c_int32),
                ("blocks", C.c_int64), ("samples", C.c_int64), ("bytes_read", C.c_int64), ("bytes_written", C.c_int64),
                ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_vtrace_supported.argtypes = [DP]
    L.ts_vtrace_supported.restype = C.c_int32
    L.ts_traj_vtrace.argtypes = [DP, SP, C.POINTER(VtraceIn), C.POINTER(VtraceOut), P]
    L.ts_traj_vtrace.restype = C.c_int32
    L.ts_describe_traj_vtrace.argtypes = [DP, C.c_int32, C.c_uint32, C.POINTER(VtraceDesc)]
    L.ts_describe_traj_vtrace.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def vtrace_supported(dims):
    """ts_vtrace_supported(dims) as a bool; raises for invalid dims.  No GPU needed."""
    rc = lib().ts_vtrace_supported(C.byref(dims))
    if rc < 0:
        check(rc, "ts_vtrace_supported")
    return rc == 1


def describe_traj_vtrace(dims, steps=1, what=OUT_ALL):
    """dict of ts_describe_traj_vtrace: the launch ts_traj_vtrace would make for the outputs and inputs of `what`.  No GPU needed."""
    desc = VtraceDesc()
    check(lib().ts_describe_traj_vtrace(C.byref(dims), int(steps), int(what), C.byref(desc)), "ts_describe_traj_vtrace")
    return desc.as_dict()
