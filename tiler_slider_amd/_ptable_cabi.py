"""ctypes binding of lib/libtiler_slider_ptable.so — the policy tables' C-ABI declared in include/tiler_slider_ptable.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES; it is an entry of _libraries.LATER, which says why it is not one of LIBRARIES.  There is no CPU fallback:
if the library is missing or does not load, every entry point raises.
The network's device functions and the forward's block plan are csrc/ts_mlp.h's, shared with the policy, train and actor-critic
libraries: HEADERS lists it, so editing it marks this library stale too.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Desc, Dims, State
from ._policy_cabi import Mlp

SRC = os.path.join(_cabi._PKG, "csrc", "ts_ptable.hip")
HEADERS = _cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi._PKG, "csrc", "ts_mlp.h")] + [
    os.path.join(_cabi.ROOT, "include", h) for h in ("tiler_slider_search.h", "tiler_slider_table.h", "tiler_slider_rollout.h",
                                                     "tiler_slider_policy.h", "tiler_slider_ptable.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_ptable.so")
HEADER, PREFIX, LABEL = "tiler_slider_ptable.h", "ts_ptable_", "ptable "

ABI_VERSION = 1
NO_ACTION = 255
SCORE_COLUMNS = 8
FORM_NONE, FORM_WAVE, FORM_BLOCK, FORM_FLAT = 0, 1, 2, 3
MIN_KERNELS = 31  # k_ptable_actions<1 .. 8>, k_ptable_walk_wave<1 .. 8>, k_ptable_walk_block<2 .. 8>, k_ptable_score<1 .. 8>

EXPORTS = ("ts_ptable_abi_version", "ts_ptable_last_hip_error", "ts_ptable_supported", "ts_ptable_actions", "ts_ptable_walk",
           "ts_ptable_score", "ts_describe_ptable_actions", "ts_describe_ptable_walk", "ts_describe_ptable_score")


class PtableDesc(Desc):
    """ts_ptable_desc: what one ts_ptable_actions / ts_ptable_walk / ts_ptable_score would launch."""
    _fields_ = [("form", C.c_int32), ("lanes_per_level", C.c_int32), ("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32),
                ("weights_in_lds", C.c_int32), ("passes", C.c_int32), ("states", C.c_int64), ("blocks", C.c_int64), ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP, XP = C.c_void_p, C.POINTER(Dims), C.POINTER(State), C.POINTER(PtableDesc)
    L.ts_ptable_supported.argtypes = [DP, C.c_int32]
    L.ts_ptable_supported.restype = C.c_int32
    L.ts_ptable_actions.argtypes = [DP, SP, C.POINTER(Mlp), P, P, P]
    L.ts_ptable_actions.restype = C.c_int32
    L.ts_ptable_walk.argtypes = [DP, SP, P, C.c_int32, P, P]
    L.ts_ptable_walk.restype = C.c_int32
    L.ts_ptable_score.argtypes = [DP, SP, P, P, P, P, P]
    L.ts_ptable_score.restype = C.c_int32
    L.ts_describe_ptable_actions.argtypes = [DP, C.c_int32, XP]
    L.ts_describe_ptable_actions.restype = C.c_int32
    L.ts_describe_ptable_walk.argtypes = [DP, XP]
    L.ts_describe_ptable_walk.restype = C.c_int32
    L.ts_describe_ptable_score.argtypes = [DP, XP]
    L.ts_describe_ptable_score.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def ptable_supported(dims, hidden=1):
    """ts_ptable_supported(dims, hidden) as a bool; raises for invalid dims.  No GPU needed."""
    rc = lib().ts_ptable_supported(C.byref(dims), int(hidden))
    if rc < 0:
        check(int(rc), "ts_ptable_supported")
    return rc == 1


def describe_ptable_actions(dims, hidden):
    """dict of ts_describe_ptable_actions: the launch ts_ptable_actions would make.  No GPU needed."""
    desc = PtableDesc()
    check(lib().ts_describe_ptable_actions(C.byref(dims), int(hidden), C.byref(desc)), "ts_describe_ptable_actions")
    return desc.as_dict()


def describe_ptable_walk(dims):
    """dict of ts_describe_ptable_walk: the launch ts_ptable_walk would make.  No GPU needed."""
    desc = PtableDesc()
    check(lib().ts_describe_ptable_walk(C.byref(dims), C.byref(desc)), "ts_describe_ptable_walk")
    return desc.as_dict()


def describe_ptable_score(dims):
    """dict of ts_describe_ptable_score: the launch ts_ptable_score would make.  No GPU needed."""
    desc = PtableDesc()
    check(lib().ts_describe_ptable_score(C.byref(dims), C.byref(desc)), "ts_describe_ptable_score")
    return desc.as_dict()
