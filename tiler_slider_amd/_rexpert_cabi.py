"""ctypes binding of lib/libtiler_slider_rexpert.so — the reach-table experts' C-ABI declared in include/tiler_slider_rexpert.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES; it is an entry of _libraries.ADDED, which says why it is not one of LIBRARIES.  There is no CPU fallback:
if the library is missing or does not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Desc, Dims, State
from ._rollout_cabi import OUT_FIELDS, ROLLOUT_MAX_SIZE, ROLLOUT_MAX_STEPS, ROLLOUT_MAX_TILES, RolloutOut
from ._targets_cabi import LabelsOut

SRC = os.path.join(_cabi._PKG, "csrc", "ts_rexpert.hip")
HEADERS = _cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi.ROOT, "include", h) for h in (
    "tiler_slider_search.h", "tiler_slider_table.h", "tiler_slider_rollout.h", "tiler_slider_reach.h", "tiler_slider_rtable.h",
    "tiler_slider_policy.h", "tiler_slider_train.h", "tiler_slider_targets.h", "tiler_slider_rexpert.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_rexpert.so")
HEADER, PREFIX, LABEL = "tiler_slider_rexpert.h", "ts_rexpert_", "rexpert "

ABI_VERSION = 1
LABELS_OUT_MOVES, LABELS_OUT_BEST, LABELS_OUT_ACTION = 0x01, 0x02, 0x04
MIN_KERNELS = 16  # k_rexpert_rollout<1 .. 8>, k_rexpert_labels<1 .. 8>

EXPORTS = ("ts_rexpert_abi_version", "ts_rexpert_last_hip_error", "ts_rexpert_supported", "ts_rexpert_rollout", "ts_rexpert_labels",
           "ts_describe_rexpert_rollout", "ts_describe_rexpert_labels")


class RexpertCfg(C.Structure):
    """ts_rexpert_cfg: a rollout's steps, mode and stream, and the reach table it reads."""
    _fields_ = [("steps", C.c_int32), ("mode", C.c_uint32), ("write_state", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64),
                ("step_index", C.c_int64), ("board_offset", C.c_int64), ("explore_threshold", C.c_uint64), ("table", C.c_void_p),
                ("slots", C.c_int64), ("count", C.c_void_p), ("n_rows", C.c_int64), ("rows", C.c_void_p)]


class RexpertLabelsIn(C.Structure):
    """ts_rexpert_labels_in: ts_labels_in with (table, count, slots) of a reach table in place of the dense pointer."""
    _fields_ = [("first", C.c_void_p), ("pos_log", C.c_void_p), ("table", C.c_void_p), ("count", C.c_void_p), ("rows", C.c_void_p),
                ("slots", C.c_int64), ("n_rows", C.c_int64), ("steps", C.c_int32), ("reserved", C.c_int32)]


class RexpertDesc(Desc):
    """ts_rexpert_desc: what one ts_rexpert_rollout or ts_rexpert_labels would launch."""
    _fields_ = [("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32), ("blocks", C.c_int64), ("waves", C.c_int64),
                ("samples", C.c_int64), ("bytes", C.c_int64), ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP, CP = C.c_void_p, C.POINTER(Dims), C.POINTER(State), C.POINTER(RexpertCfg)
    L.ts_rexpert_supported.argtypes = [DP]
    L.ts_rexpert_supported.restype = C.c_int32
    L.ts_rexpert_rollout.argtypes = [DP, SP, CP, C.POINTER(RolloutOut), P]
    L.ts_rexpert_rollout.restype = C.c_int32
    L.ts_rexpert_labels.argtypes = [DP, SP, C.POINTER(RexpertLabelsIn), C.POINTER(LabelsOut), P]
    L.ts_rexpert_labels.restype = C.c_int32
    L.ts_describe_rexpert_rollout.argtypes = [DP, CP, C.c_uint32, C.POINTER(RexpertDesc)]
    L.ts_describe_rexpert_rollout.restype = C.c_int32
    L.ts_describe_rexpert_labels.argtypes = [DP, C.c_int32, C.c_uint32, C.POINTER(RexpertDesc)]
    L.ts_describe_rexpert_labels.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def rexpert_supported(dims):
    """ts_rexpert_supported(dims) as a bool; raises for invalid dims.  No GPU needed."""
    rc = lib().ts_rexpert_supported(C.byref(dims))
    if rc < 0:
        check(int(rc), "ts_rexpert_supported")
    return rc == 1


def describe_rexpert_rollout(dims, cfg, out_mask=0):
    """dict of ts_describe_rexpert_rollout(dims, cfg, out_mask): the launch ts_rexpert_rollout would make.  No GPU needed."""
    desc = RexpertDesc()
    check(lib().ts_describe_rexpert_rollout(C.byref(dims), C.byref(cfg), int(out_mask), C.byref(desc)), "ts_describe_rexpert_rollout")
    return desc.as_dict()


def describe_rexpert_labels(dims, steps, what=LABELS_OUT_MOVES | LABELS_OUT_BEST | LABELS_OUT_ACTION):
    """dict of ts_describe_rexpert_labels(dims, steps, what): the launch ts_rexpert_labels would make.  No GPU needed."""
    desc = RexpertDesc()
    check(lib().ts_describe_rexpert_labels(C.byref(dims), int(steps), int(what), C.byref(desc)), "ts_describe_rexpert_labels")
    return desc.as_dict()
