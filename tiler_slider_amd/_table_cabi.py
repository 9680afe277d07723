"""ctypes binding of lib/libtiler_slider_table.so — the distance-to-win tables' C-ABI declared in include/tiler_slider_table.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES, which says why it is a library of its own.  There is no CPU fallback: if the library is missing or does
not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Desc, Dims, State

SRC = os.path.join(_cabi._PKG, "csrc", "ts_table.hip")
HEADERS = _cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi.ROOT, "include", h) for h in ("tiler_slider_search.h", "tiler_slider_table.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_table.so")
HEADER, PREFIX, LABEL = "tiler_slider_table.h", "ts_table_", "table "

ABI_VERSION = 1
TABLE_MAX_DEPTH, TABLE_INVALID, TABLE_DEEP, TABLE_NONE = 252, 253, 254, 255
FORM_NONE, FORM_WAVE, FORM_BLOCK = 0, 1, 2
TUNE_WAVE_MAX_STATES, TUNE_STATES_PER_LANE, TUNE_BLOCK_BELOW_BOARDS = 0, 1, 2
MIN_KERNELS = 23  # k_table_wave<1 .. 8>, k_table_block<2 .. 8>, k_table_lookup<1 .. 8>: what compile_guarded must find in the device assembly

EXPORTS = ("ts_table_abi_version", "ts_table_last_hip_error", "ts_table_states", "ts_table_build", "ts_table_lookup",
           "ts_describe_table_build", "ts_table_tuning")


class TableDesc(Desc):
    """ts_table_desc of include/tiler_slider_table.h: what one ts_table_build would launch."""
    _fields_ = [("form", C.c_int32), ("lanes_per_board", C.c_int32), ("boards_per_block", C.c_int32), ("threads_per_block", C.c_int32),
                ("bitmap_words", C.c_int32), ("lds_bytes_board", C.c_int32), ("lds_bytes_block", C.c_int32), ("lds_bytes_max", C.c_int32),
                ("states", C.c_int64), ("blocks", C.c_int64), ("table_bytes", C.c_int64), ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_table_states.argtypes = [DP]
    L.ts_table_states.restype = C.c_int64
    L.ts_table_build.argtypes = [DP, SP, C.c_int32, P, P]
    L.ts_table_build.restype = C.c_int32
    L.ts_table_lookup.argtypes = [DP, SP, P, C.c_int64, P, P, P, P, P]
    L.ts_table_lookup.restype = C.c_int32
    L.ts_describe_table_build.argtypes = [DP, C.POINTER(TableDesc)]
    L.ts_describe_table_build.restype = C.c_int32
    L.ts_table_tuning.argtypes = [C.c_int32, C.c_int64]
    L.ts_table_tuning.restype = C.c_int64


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def table_states(dims):
    """ts_table_states(dims): the entries of one board's row, 0 where the tables do not support the shape.  No GPU needed."""
    n = lib().ts_table_states(C.byref(dims))
    if n < 0:
        check(int(n), "ts_table_states")
    return int(n)


def describe_table_build(dims):
    """dict of ts_describe_table_build(dims): the launch ts_table_build would make.  No GPU needed."""
    desc = TableDesc()
    check(lib().ts_describe_table_build(C.byref(dims), C.byref(desc)), "ts_describe_table_build")
    return desc.as_dict()
