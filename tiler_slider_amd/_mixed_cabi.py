"""ctypes binding of lib/libtiler_slider_mixed.so — the mixed rollouts' C-ABI declared in include/tiler_slider_mixed.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES; it is an entry of _libraries.SINCE, which says why it is not one of LIBRARIES.  There is no CPU fallback:
if the library is missing or does not load, every entry point raises.
The network is csrc/ts_mlp.h's, listed through _policy_cabi.HEADERS.
"""
import ctypes as C
import os

from . import _cabi, _policy_cabi
from ._cabi import Desc, Dims, State
from ._policy_cabi import GREEDY, SAMPLE, SELECTS, Mlp

SRC = os.path.join(_cabi._PKG, "csrc", "ts_mixed.hip")
HEADERS = _policy_cabi.HEADERS + [os.path.join(_cabi.ROOT, "include", h) for h in (
    "tiler_slider_reach.h", "tiler_slider_rtable.h", "tiler_slider_mixed.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_mixed.so")
HEADER, PREFIX, LABEL = "tiler_slider_mixed.h", "ts_mixed_", "mixed "

ABI_VERSION = 1
DENSE, REACH = 0, 1
KINDS = {"dense": DENSE, "reach": REACH}
WHO_NETWORK, WHO_EXPERT, WHO_RANDOM = 0, 1, 2
SALT = 0x6a09e667f3bcc909
OUT_EXPERT_LOG, OUT_MOVES_LOG, OUT_BEST_LOG, OUT_WHO_LOG = 0x400, 0x800, 0x1000, 0x2000
MIN_KERNELS = 32  # k_mixed_rollout<1 .. 8, GREEDY / SAMPLE, DENSE / REACH>: what compile_guarded must find

EXPORTS = ("ts_mixed_abi_version", "ts_mixed_last_hip_error", "ts_mixed_supported", "ts_mixed_rollout", "ts_describe_mixed_rollout")


class MixedCfg(C.Structure):
    """ts_mixed_cfg: ts_policy_cfg's fields, beta, and the table of either kind."""
    _fields_ = [("steps", C.c_int32), ("mode", C.c_uint32), ("select", C.c_int32), ("write_state", C.c_int32), ("seed", C.c_uint64),
                ("step_index", C.c_int64), ("board_offset", C.c_int64), ("explore_threshold", C.c_uint64), ("beta_threshold", C.c_uint64),
                ("kind", C.c_int32), ("reserved", C.c_int32), ("dense", C.c_void_p), ("table", C.c_void_p), ("slots", C.c_int64),
                ("count", C.c_void_p), ("n_rows", C.c_int64), ("rows", C.c_void_p)]


OUT_FIELDS = _policy_cabi.OUT_FIELDS + ("expert_log", "moves_log", "best_log", "who_log")


class MixedOut(C.Structure):
    """ts_mixed_out: fourteen optional device pointers - the ten of ts_policy_out and the four logs of the lookup."""
    _fields_ = [(name, C.c_void_p) for name in OUT_FIELDS]


class MixedDesc(Desc):
    """ts_mixed_desc: what one ts_mixed_rollout would launch."""
    _fields_ = [("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32), ("weights_in_lds", C.c_int32), ("table_read", C.c_int32),
                ("blocks", C.c_int64), ("logged_bytes", C.c_int64), ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP, CP = C.c_void_p, C.POINTER(Dims), C.POINTER(State), C.POINTER(MixedCfg)
    L.ts_mixed_supported.argtypes = [DP, C.c_int32, C.c_int32]
    L.ts_mixed_supported.restype = C.c_int32
    L.ts_mixed_rollout.argtypes = [DP, SP, C.POINTER(Mlp), CP, C.POINTER(MixedOut), P]
    L.ts_mixed_rollout.restype = C.c_int32
    L.ts_describe_mixed_rollout.argtypes = [DP, C.c_int32, CP, C.c_uint32, C.POINTER(MixedDesc)]
    L.ts_describe_mixed_rollout.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def mixed_supported(dims, hidden, kind):
    """ts_mixed_supported(dims, hidden, kind) as a bool, `kind` one of KINDS' values; raises for invalid dims or an unknown kind.
    No GPU needed."""
    rc = lib().ts_mixed_supported(C.byref(dims), int(hidden), int(kind))
    if rc < 0:
        check(rc, "ts_mixed_supported")
    return rc == 1


def describe_mixed_rollout(dims, hidden, cfg, out_mask=0):
    """dict of ts_describe_mixed_rollout: the launch ts_mixed_rollout would make.  No GPU needed."""
    desc = MixedDesc()
    check(lib().ts_describe_mixed_rollout(C.byref(dims), int(hidden), C.byref(cfg), int(out_mask), C.byref(desc)), "ts_describe_mixed_rollout")
    return desc.as_dict()
