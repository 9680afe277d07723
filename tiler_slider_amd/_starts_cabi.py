"""ctypes binding of lib/libtiler_slider_starts.so — the curriculum starts' C-ABI declared in include/tiler_slider_starts.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES, which says why it is a library of its own.  There is no CPU fallback: if the library is missing or does
not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Desc, Dims, State

SRC = os.path.join(_cabi._PKG, "csrc", "ts_starts.hip")
HEADERS = (_cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi._PKG, "csrc", "ts_bytes.h")]
           + [os.path.join(_cabi.ROOT, "include", h) for h in ("tiler_slider_search.h", "tiler_slider_table.h", "tiler_slider_starts.h")])
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_starts.so")
HEADER, PREFIX, LABEL = "tiler_slider_starts.h", "ts_starts_", "starts "

ABI_VERSION = 1
MIN_KERNELS = 8  # k_starts_place<1 .. 8>: what compile_guarded must find in the device assembly
ALL, DONE = 0, 1
PIECE_BYTES = 16
FORM_NONE, FORM_WAVE = 0, 1

EXPORTS = ("ts_starts_abi_version", "ts_starts_last_hip_error", "ts_starts_supported", "ts_starts_place", "ts_describe_starts_place")


class StartsCfg(C.Structure):
    """ts_starts_cfg: the band for all boards or per board, which boards are selected, what is written, and the draw."""
    _fields_ = [("lo", C.c_int32), ("hi", C.c_int32), ("band", C.c_void_p), ("where", C.c_int32), ("write_pos", C.c_int32),
                ("write_init", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("step_index", C.c_int64),
                ("board_offset", C.c_int64)]


class StartsOut(C.Structure):
    """ts_starts_out: count int32 [N], dist uint8 [N], deepest uint8 [N]; each may be NULL."""
    _fields_ = [("count", C.c_void_p), ("dist", C.c_void_p), ("deepest", C.c_void_p)]


class StartsDesc(Desc):
    """ts_starts_desc: what one ts_starts_place would launch."""
    _fields_ = [("form", C.c_int32), ("lanes_per_board", C.c_int32), ("boards_per_block", C.c_int32), ("threads_per_block", C.c_int32),
                ("bytes_per_lane", C.c_int32), ("passes", C.c_int32), ("states", C.c_int64), ("blocks", C.c_int64), ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_starts_supported.argtypes = [DP]
    L.ts_starts_supported.restype = C.c_int32
    L.ts_starts_place.argtypes = [DP, SP, P, C.c_int64, P, C.POINTER(StartsCfg), C.POINTER(StartsOut), P]
    L.ts_starts_place.restype = C.c_int32
    L.ts_describe_starts_place.argtypes = [DP, C.POINTER(StartsDesc)]
    L.ts_describe_starts_place.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def starts_supported(dims):
    """ts_starts_supported(dims): the shapes of the distance tables; raises for invalid dims.  No GPU needed."""
    rc = lib().ts_starts_supported(C.byref(dims))
    if rc < 0:
        check(int(rc), "ts_starts_supported")
    return bool(rc)


def describe_starts_place(dims):
    """dict of ts_describe_starts_place(dims): the launch ts_starts_place would make.  No GPU needed."""
    desc = StartsDesc()
    check(lib().ts_describe_starts_place(C.byref(dims), C.byref(desc)), "ts_describe_starts_place")
    return desc.as_dict()
