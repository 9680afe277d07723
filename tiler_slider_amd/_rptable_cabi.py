"""ctypes binding of lib/libtiler_slider_rptable.so — the reach policy tables' C-ABI declared in include/tiler_slider_rptable.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES; it is an entry of _libraries.SINCE, which says why it is not one of LIBRARIES.  There is no CPU fallback:
if the library is missing or does not load, every entry point raises.
The network's device functions are csrc/ts_mlp.h's, shared with the policy, train, actor-critic and policy-table libraries:
HEADERS lists it, so editing it marks this library stale too.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Desc, Dims, State
from ._policy_cabi import Mlp
from ._rtable_cabi import ROOTS  # the root's names are the reach table's, not copies

SRC = os.path.join(_cabi._PKG, "csrc", "ts_rptable.hip")
HEADERS = _cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi._PKG, "csrc", "ts_mlp.h")] + [
    os.path.join(_cabi.ROOT, "include", h) for h in ("tiler_slider_search.h", "tiler_slider_table.h", "tiler_slider_rollout.h",
                                                     "tiler_slider_policy.h", "tiler_slider_ptable.h", "tiler_slider_reach.h",
                                                     "tiler_slider_rtable.h", "tiler_slider_rptable.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_rptable.so")
HEADER, PREFIX, LABEL = "tiler_slider_rptable.h", "ts_rptable_", "rptable "

ABI_VERSION = 1
NO_ACTION = 255
SCORE_COLUMNS = 8
FORM_NONE, FORM_LDS, FORM_GLOBAL = 0, 1, 2
MIN_KERNELS = 32  # k_rptable_actions<1 .. 8>, k_rptable_walk<1 .. 8, false>, k_rptable_walk<1 .. 8, true>, k_rptable_score<1 .. 8>

EXPORTS = ("ts_rptable_abi_version", "ts_rptable_last_hip_error", "ts_rptable_supported", "ts_rptable_actions", "ts_rptable_walk",
           "ts_rptable_score", "ts_describe_rptable_actions", "ts_describe_rptable_walk", "ts_describe_rptable_score")


class RptableCfg(C.Structure):
    """ts_rptable_cfg"""
    _fields_ = [("max_depth", C.c_int32), ("root", C.c_int32)]


class RptableOut(C.Structure):
    """ts_rptable_out: `table` required, the other two optional."""
    _fields_ = [("table", C.c_void_p), ("root_moves", C.c_void_p), ("deepest", C.c_void_p)]


class RptableDesc(Desc):
    """ts_rptable_desc: what one ts_rptable_actions / ts_rptable_walk / ts_rptable_score would launch."""
    _fields_ = [("form", C.c_int32), ("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32), ("lds_slots", C.c_int32),
                ("weights_in_lds", C.c_int32), ("reserved", C.c_int32), ("blocks", C.c_int64), ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP, XP = C.c_void_p, C.POINTER(Dims), C.POINTER(State), C.POINTER(RptableDesc)
    L.ts_rptable_supported.argtypes = [DP, C.c_int32]
    L.ts_rptable_supported.restype = C.c_int32
    L.ts_rptable_actions.argtypes = [DP, SP, C.POINTER(Mlp), P, C.c_int64, P, P, P, P]
    L.ts_rptable_actions.restype = C.c_int32
    L.ts_rptable_walk.argtypes = [DP, SP, P, C.c_int64, P, P, C.POINTER(RptableCfg), C.POINTER(RptableOut), P]
    L.ts_rptable_walk.restype = C.c_int32
    L.ts_rptable_score.argtypes = [DP, SP, P, P, P, C.c_int64, P, P, P]
    L.ts_rptable_score.restype = C.c_int32
    L.ts_describe_rptable_actions.argtypes = [DP, C.c_int32, C.c_int64, XP]
    L.ts_describe_rptable_actions.restype = C.c_int32
    L.ts_describe_rptable_walk.argtypes = [DP, C.c_int64, XP]
    L.ts_describe_rptable_walk.restype = C.c_int32
    L.ts_describe_rptable_score.argtypes = [DP, C.c_int64, XP]
    L.ts_describe_rptable_score.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def rptable_supported(dims, hidden=1):
    """ts_rptable_supported(dims, hidden) as a bool; raises for invalid dims.  No GPU needed."""
    rc = lib().ts_rptable_supported(C.byref(dims), int(hidden))
    if rc < 0:
        check(int(rc), "ts_rptable_supported")
    return rc == 1


def describe_rptable_actions(dims, hidden, slots):
    """dict of ts_describe_rptable_actions: the launch ts_rptable_actions would make.  No GPU needed."""
    desc = RptableDesc()
    check(lib().ts_describe_rptable_actions(C.byref(dims), int(hidden), int(slots), C.byref(desc)), "ts_describe_rptable_actions")
    return desc.as_dict()


def describe_rptable_walk(dims, slots):
    """dict of ts_describe_rptable_walk: the launch ts_rptable_walk would make.  No GPU needed."""
    desc = RptableDesc()
    check(lib().ts_describe_rptable_walk(C.byref(dims), int(slots), C.byref(desc)), "ts_describe_rptable_walk")
    return desc.as_dict()


def describe_rptable_score(dims, slots):
    """dict of ts_describe_rptable_score: the launch ts_rptable_score would make.  No GPU needed."""
    desc = RptableDesc()
    check(lib().ts_describe_rptable_score(C.byref(dims), int(slots), C.byref(desc)), "ts_describe_rptable_score")
    return desc.as_dict()
