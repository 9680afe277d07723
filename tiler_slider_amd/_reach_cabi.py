"""ctypes binding of lib/libtiler_slider_reach.so — the hashed solver's C-ABI declared in include/tiler_slider_reach.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES; it is an entry of _libraries.ADDED, which says why it is not one of LIBRARIES.  There is no CPU fallback:
if the library is missing or does not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Desc, Dims, State

SRC = os.path.join(_cabi._PKG, "csrc", "ts_reach.hip")
HEADERS = _cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi.ROOT, "include", h) for h in ("tiler_slider_search.h", "tiler_slider_reach.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_reach.so")
HEADER, PREFIX, LABEL = "tiler_slider_reach.h", "ts_reach_", "reach "

ABI_VERSION = 1
SOLVE_FULL = -3
REACH_MAX_SIZE, REACH_MAX_TILES, REACH_MAX_DEPTH, REACH_MAX_CAPACITY = 8, 8, 32767, 1 << 30
MIN_KERNELS = 8  # k_reach<1 .. 8>

EXPORTS = ("ts_reach_abi_version", "ts_reach_last_hip_error", "ts_reach_supported", "ts_reach_workspace_bytes", "ts_reach_solve",
           "ts_describe_reach")


class ReachCfg(C.Structure):
    """ts_reach_cfg: depth and state budget of a search, and the workspace it runs in."""
    _fields_ = [("max_depth", C.c_int32), ("capacity", C.c_int32), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class ReachOut(C.Structure):
    """ts_reach_out: moves is required, best and states may be NULL."""
    _fields_ = [("moves", C.c_void_p), ("best", C.c_void_p), ("states", C.c_void_p)]


class ReachDesc(Desc):
    """ts_reach_desc: what one ts_reach_solve would launch."""
    _fields_ = [("threads_per_block", C.c_int32), ("reserved", C.c_int32), ("blocks", C.c_int64), ("boards_in_flight", C.c_int64),
                ("slots_per_board", C.c_int64), ("table_bytes", C.c_int64), ("frontier_bytes", C.c_int64), ("log_bytes", C.c_int64),
                ("bytes_per_board", C.c_int64), ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP, CP = C.c_void_p, C.POINTER(Dims), C.POINTER(State), C.POINTER(ReachCfg)
    L.ts_reach_supported.argtypes = [DP]
    L.ts_reach_supported.restype = C.c_int32
    L.ts_reach_workspace_bytes.argtypes = [DP, C.c_int32, C.c_int64]
    L.ts_reach_workspace_bytes.restype = C.c_int64
    L.ts_reach_solve.argtypes = [DP, SP, CP, C.POINTER(ReachOut), P]
    L.ts_reach_solve.restype = C.c_int32
    L.ts_describe_reach.argtypes = [DP, CP, C.POINTER(ReachDesc)]
    L.ts_describe_reach.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def reach_supported(dims):
    """ts_reach_supported(dims) as a bool; raises for invalid dims.  No GPU needed."""
    rc = lib().ts_reach_supported(C.byref(dims))
    if rc < 0:
        check(int(rc), "ts_reach_supported")
    return rc == 1


def workspace_bytes(dims, capacity, boards_in_flight=1):
    """ts_reach_workspace_bytes: the workspace that lets `boards_in_flight` boards be searched at once.  No GPU needed."""
    n = lib().ts_reach_workspace_bytes(C.byref(dims), int(capacity), int(boards_in_flight))
    if n < 0:
        check(int(n), "ts_reach_workspace_bytes")
    return int(n)


def describe_reach(dims, max_depth=64, capacity=4096, workspace_bytes=1 << 30):
    """dict of ts_describe_reach: the launch ts_reach_solve would make with such a workspace.  No GPU needed."""
    desc = ReachDesc()
    cfg = ReachCfg(int(max_depth), int(capacity), None, int(workspace_bytes))
    check(lib().ts_describe_reach(C.byref(dims), C.byref(cfg), C.byref(desc)), "ts_describe_reach")
    return desc.as_dict()
