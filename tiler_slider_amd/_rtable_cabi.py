"""ctypes binding of lib/libtiler_slider_rtable.so — the reachable distance tables' C-ABI declared in include/tiler_slider_rtable.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES; it is an entry of _libraries.ADDED, which says why it is not one of LIBRARIES.  There is no CPU fallback:
if the library is missing or does not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Desc, Dims, State

SRC = os.path.join(_cabi._PKG, "csrc", "ts_rtable.hip")
HEADERS = _cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi.ROOT, "include", h) for h in (
    "tiler_slider_search.h", "tiler_slider_reach.h", "tiler_slider_table.h", "tiler_slider_rtable.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_rtable.so")
HEADER, PREFIX, LABEL = "tiler_slider_rtable.h", "ts_rtable_", "rtable "

ABI_VERSION = 1
SOLVE_ABSENT = -4
ROOT_INIT, ROOT_POS = 0, 1
ROOTS = {"init": ROOT_INIT, "pos": ROOT_POS}
MIN_KERNELS = 16  # k_rtable_build<1 .. 8>, k_rtable_lookup<1 .. 8>

EXPORTS = ("ts_rtable_abi_version", "ts_rtable_last_hip_error", "ts_rtable_supported", "ts_rtable_slots", "ts_rtable_workspace_bytes",
           "ts_rtable_build", "ts_rtable_lookup", "ts_describe_rtable_build")


class RtableCfg(C.Structure):
    """ts_rtable_cfg: depth, state budget and root of a build, and the workspace it runs in."""
    _fields_ = [("max_depth", C.c_int32), ("capacity", C.c_int32), ("root", C.c_int32), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64)]


class RtableOut(C.Structure):
    """ts_rtable_out: table and count are required, root_moves and deepest may be NULL."""
    _fields_ = [("table", C.c_void_p), ("count", C.c_void_p), ("root_moves", C.c_void_p), ("deepest", C.c_void_p)]


class RtableDesc(Desc):
    """ts_rtable_desc: what one ts_rtable_build would launch."""
    _fields_ = [("threads_per_block", C.c_int32), ("reserved", C.c_int32), ("blocks", C.c_int64), ("levels_in_flight", C.c_int64),
                ("slots", C.c_int64), ("table_bytes", C.c_int64), ("workspace_bytes", C.c_int64), ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP, CP = C.c_void_p, C.POINTER(Dims), C.POINTER(State), C.POINTER(RtableCfg)
    L.ts_rtable_supported.argtypes = [DP]
    L.ts_rtable_supported.restype = C.c_int32
    L.ts_rtable_slots.argtypes = [C.c_int32]
    L.ts_rtable_slots.restype = C.c_int64
    L.ts_rtable_workspace_bytes.argtypes = [DP, C.c_int32, C.c_int64]
    L.ts_rtable_workspace_bytes.restype = C.c_int64
    L.ts_rtable_build.argtypes = [DP, SP, CP, C.POINTER(RtableOut), P]
    L.ts_rtable_build.restype = C.c_int32
    L.ts_rtable_lookup.argtypes = [DP, SP, P, C.c_int64, P, C.c_int64, P, P, P, P, P]
    L.ts_rtable_lookup.restype = C.c_int32
    L.ts_describe_rtable_build.argtypes = [DP, CP, C.POINTER(RtableDesc)]
    L.ts_describe_rtable_build.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def rtable_supported(dims):
    """ts_rtable_supported(dims) as a bool; raises for invalid dims.  No GPU needed."""
    rc = lib().ts_rtable_supported(C.byref(dims))
    if rc < 0:
        check(int(rc), "ts_rtable_supported")
    return rc == 1


def slots(capacity):
    """ts_rtable_slots: the 64-bit slots of one level's row.  No GPU needed."""
    n = lib().ts_rtable_slots(int(capacity))
    if n < 0:
        check(int(n), "ts_rtable_slots")
    return int(n)


def workspace_bytes(dims, capacity, levels_in_flight=1):
    """ts_rtable_workspace_bytes: the workspace that lets `levels_in_flight` levels be built at once.  No GPU needed."""
    n = lib().ts_rtable_workspace_bytes(C.byref(dims), int(capacity), int(levels_in_flight))
    if n < 0:
        check(int(n), "ts_rtable_workspace_bytes")
    return int(n)


def describe_rtable_build(dims, max_depth=252, capacity=4096, workspace_bytes=1 << 30, root=ROOT_INIT):
    """dict of ts_describe_rtable_build: the launch ts_rtable_build would make with such a workspace.  No GPU needed."""
    desc = RtableDesc()
    cfg = RtableCfg(int(max_depth), int(capacity), int(root), None, int(workspace_bytes))
    check(lib().ts_describe_rtable_build(C.byref(dims), C.byref(cfg), C.byref(desc)), "ts_describe_rtable_build")
    return desc.as_dict()
