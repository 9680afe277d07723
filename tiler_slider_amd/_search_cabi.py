"""ctypes binding of lib/libtiler_slider_search.so — the solver's C-ABI declared in include/tiler_slider_search.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES, which says why it is a library of its own.  There is no CPU fallback: if the library is missing or does
not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Desc, Dims, State

SRC = os.path.join(_cabi._PKG, "csrc", "ts_search.hip")
HEADERS = _cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi.ROOT, "include", h) for h in ("tiler_slider_search.h",)]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_search.so")
HEADER, PREFIX, LABEL = "tiler_slider_search.h", "ts_search_", "solver "

ABI_VERSION = 1
SOLVE_NONE, SOLVE_DEPTH = -1, -2
SOLVE_MAX_SIZE, SOLVE_MAX_STATES, SOLVE_MAX_DEPTH = 8, 65536, 32767
FORM_NONE, FORM_WAVE, FORM_BLOCK = 0, 1, 2
TUNE_WAVE_MAX_STATES, TUNE_WORDS_PER_LANE = 0, 1
MIN_KERNELS = 12  # k_solve_wave<1 .. 8>, k_solve_block<3 .. 6>: what compile_guarded must find in the device assembly

EXPORTS = ("ts_search_abi_version", "ts_search_last_hip_error", "ts_solve_states", "ts_solve", "ts_describe_solve",
           "ts_search_tuning")


class SolveDesc(Desc):
    """ts_solve_desc of include/tiler_slider_search.h: what one ts_solve would launch."""
    _fields_ = [("form", C.c_int32), ("lanes_per_board", C.c_int32), ("boards_per_block", C.c_int32), ("threads_per_block", C.c_int32),
                ("bitmap_words", C.c_int32), ("lds_bytes_board", C.c_int32), ("lds_bytes_block", C.c_int32), ("reserved", C.c_int32),
                ("states", C.c_int64), ("blocks", C.c_int64), ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_solve_states.argtypes = [DP]
    L.ts_solve_states.restype = C.c_int64
    L.ts_solve.argtypes = [DP, SP, C.c_int32, P, P, P]
    L.ts_solve.restype = C.c_int32
    L.ts_describe_solve.argtypes = [DP, C.POINTER(SolveDesc)]
    L.ts_describe_solve.restype = C.c_int32
    L.ts_search_tuning.argtypes = [C.c_int32, C.c_int64]
    L.ts_search_tuning.restype = C.c_int64


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def solve_states(dims):
    """ts_solve_states(dims): the size of the index space, 0 where ts_solve does not support the shape.  No GPU needed."""
    n = lib().ts_solve_states(C.byref(dims))
    if n < 0:
        check(int(n), "ts_solve_states")
    return int(n)


def describe_solve(dims):
    """dict of ts_describe_solve(dims): the launch ts_solve would make.  No GPU needed."""
    desc = SolveDesc()
    check(lib().ts_describe_solve(C.byref(dims), C.byref(desc)), "ts_describe_solve")
    return desc.as_dict()
