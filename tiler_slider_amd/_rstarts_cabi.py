"""ctypes binding of lib/libtiler_slider_rstarts.so — the reach-table curricula's C-ABI declared in include/tiler_slider_rstarts.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES; it is an entry of _libraries.SINCE, which says why it is not one of LIBRARIES.  There is no CPU fallback:
if the library is missing or does not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Desc, Dims, State
from ._starts_cabi import ALL, DONE, StartsCfg, StartsOut  # the placement's structs are the dense call's, not copies

SRC = os.path.join(_cabi._PKG, "csrc", "ts_rstarts.hip")
HEADERS = _cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi.ROOT, "include", h) for h in (
    "tiler_slider_search.h", "tiler_slider_reach.h", "tiler_slider_table.h", "tiler_slider_rtable.h", "tiler_slider_starts.h",
    "tiler_slider_rstarts.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_rstarts.so")
HEADER, PREFIX, LABEL = "tiler_slider_rstarts.h", "ts_rstarts_", "rstarts "

ABI_VERSION = 1
FIRST = 256  # int32 words of one level's `first` row
FORM_NONE, FORM_LDS, FORM_GLOBAL = 0, 1, 2
MIN_KERNELS = 10  # k_rstarts_index<false>, k_rstarts_index<true>, k_rstarts_place<1 .. 8>

EXPORTS = ("ts_rstarts_abi_version", "ts_rstarts_last_hip_error", "ts_rstarts_supported", "ts_rstarts_index", "ts_rstarts_place",
           "ts_describe_rstarts_index", "ts_describe_rstarts_place")


class RstartsDesc(Desc):
    """ts_rstarts_desc: what one ts_rstarts_index or ts_rstarts_place would launch."""
    _fields_ = [("form", C.c_int32), ("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32), ("lds_states", C.c_int32),
                ("blocks", C.c_int64), ("bytes", C.c_int64), ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_rstarts_supported.argtypes = [DP]
    L.ts_rstarts_supported.restype = C.c_int32
    L.ts_rstarts_index.argtypes = [P, C.c_int64, P, C.c_int64, C.c_int64, P, P, P]
    L.ts_rstarts_index.restype = C.c_int32
    L.ts_rstarts_place.argtypes = [DP, SP, P, P, C.c_int64, C.c_int64, P, C.POINTER(StartsCfg), C.POINTER(StartsOut), P]
    L.ts_rstarts_place.restype = C.c_int32
    L.ts_describe_rstarts_index.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.POINTER(RstartsDesc)]
    L.ts_describe_rstarts_index.restype = C.c_int32
    L.ts_describe_rstarts_place.argtypes = [DP, C.POINTER(RstartsDesc)]
    L.ts_describe_rstarts_place.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def rstarts_supported(dims):
    """ts_rstarts_supported(dims): the shapes of the reachable distance tables; raises for invalid dims.  No GPU needed."""
    rc = lib().ts_rstarts_supported(C.byref(dims))
    if rc < 0:
        check(int(rc), "ts_rstarts_supported")
    return rc == 1


def describe_rstarts_index(n_levels, slots, width):
    """dict of ts_describe_rstarts_index(n_levels, slots, W): the launch ts_rstarts_index would make.  No GPU needed."""
    desc = RstartsDesc()
    check(lib().ts_describe_rstarts_index(int(n_levels), int(slots), int(width), C.byref(desc)), "ts_describe_rstarts_index")
    return desc.as_dict()


def describe_rstarts_place(dims):
    """dict of ts_describe_rstarts_place(dims): the launch ts_rstarts_place would make.  No GPU needed."""
    desc = RstartsDesc()
    check(lib().ts_describe_rstarts_place(C.byref(dims), C.byref(desc)), "ts_describe_rstarts_place")
    return desc.as_dict()
