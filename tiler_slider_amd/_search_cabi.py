"""ctypes binding of lib/libtiler_slider_search.so — the solver's C-ABI declared in include/tiler_slider_search.h.

A second library beside libtiler_slider_hip.so (the step library's code object is pinned kernel by kernel, so the solver's
kernels live in their own).  Same rules as _cabi.py: built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR
hazard scan and padding), and there is no CPU fallback: if the library is missing or does not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Dims, State, TilerSliderLibraryError

SRC = os.path.join(_cabi._PKG, "csrc", "ts_search.hip")
HEADERS = _cabi.HEADERS + [os.path.join(_cabi.ROOT, "include", "tiler_slider_search.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_search.so")

ABI_VERSION = 1
SOLVE_NONE, SOLVE_DEPTH = -1, -2
SOLVE_MAX_SIZE, SOLVE_MAX_STATES, SOLVE_MAX_DEPTH = 8, 65536, 32767
FORM_NONE, FORM_WAVE, FORM_BLOCK = 0, 1, 2
TUNE_WAVE_MAX_STATES, TUNE_WORDS_PER_LANE = 0, 1
MIN_KERNELS = 12  # k_solve_wave<1 .. 8>, k_solve_block<3 .. 6>: what compile_guarded must find in the device assembly

EXPORTS = ("ts_search_abi_version", "ts_search_last_hip_error", "ts_solve_states", "ts_solve", "ts_describe_solve",
           "ts_search_tuning")


class SolveDesc(C.Structure):
    """ts_solve_desc of include/tiler_slider_search.h: what one ts_solve would launch."""
    _fields_ = [("form", C.c_int32), ("lanes_per_board", C.c_int32), ("boards_per_block", C.c_int32), ("threads_per_block", C.c_int32),
                ("bitmap_words", C.c_int32), ("lds_bytes_board", C.c_int32), ("lds_bytes_block", C.c_int32), ("reserved", C.c_int32),
                ("states", C.c_int64), ("blocks", C.c_int64), ("name", C.c_char * 64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["name"] = self.name.decode()
        return d


def _stale():
    if not os.path.exists(LIB_PATH):
        return True
    built = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(p) > built for p in [SRC] + HEADERS)


def build_library(force=False, verbose=False):
    """Compile the solver's kernels for gfx950 in-tree, through the same guarded steps as the step library."""
    if not force and not _stale():
        return LIB_PATH
    _cabi.compile_guarded(SRC, LIB_PATH, verbose=verbose, keep_asm=os.environ.get("TS_KEEP_ASM") == "1", min_kernels=MIN_KERNELS)
    return LIB_PATH


_lib = None


def lib():
    """The loaded solver library; raises (never falls back) when it is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TilerSliderLibraryError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback.")
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:
        raise TilerSliderLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    missing = [s for s in EXPORTS if not hasattr(L, s)]
    if missing:
        raise TilerSliderLibraryError(f"{LIB_PATH} lacks symbols {missing}; rebuild it")
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_search_abi_version.restype = C.c_int32
    L.ts_search_last_hip_error.restype = C.c_int32
    L.ts_solve_states.argtypes = [DP]
    L.ts_solve_states.restype = C.c_int64
    L.ts_solve.argtypes = [DP, SP, C.c_int32, P, P, P]
    L.ts_solve.restype = C.c_int32
    L.ts_describe_solve.argtypes = [DP, C.POINTER(SolveDesc)]
    L.ts_describe_solve.restype = C.c_int32
    L.ts_search_tuning.argtypes = [C.c_int32, C.c_int64]
    L.ts_search_tuning.restype = C.c_int64
    if L.ts_search_abi_version() != ABI_VERSION:
        raise TilerSliderLibraryError(f"solver ABI version {L.ts_search_abi_version()} != {ABI_VERSION}; rebuild the library")
    _lib = L
    return L


def check(rc, what):
    if rc != _cabi.OK:
        msg = _cabi.lib().ts_status_string(rc).decode()  # the status codes are the step library's
        extra = f" (hipError {lib().ts_search_last_hip_error()})" if rc == _cabi.ERR_HIP else ""
        raise TilerSliderLibraryError(f"{what}: {msg}{extra}")


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
