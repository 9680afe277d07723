"""ctypes binding of lib/libtiler_slider_update.so — the in-place step's C-ABI declared in include/tiler_slider_update.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES, which says why it is a library of its own.  There is no CPU fallback: if the library is missing or does
not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Dims, LaunchDesc, State, StepOut

SRC = os.path.join(_cabi._PKG, "csrc", "ts_update.hip")
HEADERS = (_cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi._PKG, "csrc", "ts_quad.h")]
           + [os.path.join(_cabi.ROOT, "include", h) for h in ("tiler_slider_search.h", "tiler_slider_update.h")])
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_update.so")
HEADER, PREFIX, LABEL = "tiler_slider_update.h", "ts_update_", "update "

ABI_VERSION = 1
UPDATE_MAX_SIZE, UPDATE_MAX_TILES = 8, 8
KERNEL_UPDATE = 6
MIN_KERNELS = 32  # k_step_update<1 .. 8, 2 / 8, float32 / uint8>: what compile_guarded must find in the device assembly

EXPORTS = ("ts_update_abi_version", "ts_update_last_hip_error", "ts_update_supported", "ts_step_update", "ts_describe_step_update")


def _declare(L):
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_update_supported.argtypes = [DP, C.c_uint32]
    L.ts_update_supported.restype = C.c_int32
    L.ts_step_update.argtypes = [DP, SP, P, C.c_uint32, C.POINTER(StepOut), P, P]
    L.ts_step_update.restype = C.c_int32
    L.ts_describe_step_update.argtypes = [DP, C.c_uint32, C.POINTER(LaunchDesc)]
    L.ts_describe_step_update.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def update_supported(dims, outputs):
    """ts_update_supported(dims, outputs) as a bool: False for a shape or a set of outputs the in-place step does not take;
    raises for invalid dims.  No GPU needed."""
    rc = lib().ts_update_supported(C.byref(dims), int(outputs))
    if rc in (_cabi.ERR_LIMIT, _cabi.ERR_ARG):
        return False
    check(rc, "ts_update_supported")
    return True


def full_body(dims):
    """True where k_step_update steps `dims` through its straight-line body (csrc/ts_update.hip): two tiles and two targets on a
    board of at least two cells, which is when the two-tile kernels are full.  Everything else, the eight-tile kernels
    included, takes the general body of the same kernel; results never differ."""
    return dims.n_tiles == 2 and dims.n_targets == 2 and dims.size * dims.size >= 2


def describe_step_update(dims, outputs=_cabi.OUT_OBS):
    """dict of ts_describe_step_update(dims, outputs): the launch ts_step_update would make, in the record of
    _cabi.describe_launch.  No GPU needed."""
    desc = LaunchDesc()
    check(lib().ts_describe_step_update(C.byref(dims), int(outputs), C.byref(desc)), "ts_describe_step_update")
    return desc.as_dict()
