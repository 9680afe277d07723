"""ctypes binding of lib/libtiler_slider_targets.so — the trajectory targets' C-ABI declared in include/tiler_slider_targets.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES, which says why it is a library of its own.  There is no CPU fallback: if the library is missing or does
not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi, _train_cabi
from ._cabi import Desc, Dims, State

SRC = os.path.join(_cabi._PKG, "csrc", "ts_targets.hip")
HEADERS = _train_cabi.HEADERS + [os.path.join(_cabi.ROOT, "include", "tiler_slider_targets.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_targets.so")
HEADER, PREFIX, LABEL = "tiler_slider_targets.h", "ts_targets_", "targets "

ABI_VERSION = 1
MIN_KERNELS = 16  # k_traj_returns<1 .. 8> and k_traj_labels<1 .. 8>: what compile_guarded must find

RETURNS, LABELS = 0, 1
RETURNS_OUT_REWARD, RETURNS_OUT_ADV, RETURNS_OUT_RET, RETURNS_OUT_MASK = 0x01, 0x02, 0x04, 0x08
RETURNS_IN_CELLS, RETURNS_IN_FIRST, RETURNS_IN_VALUES, RETURNS_IN_LAST_VALUE = 0x10, 0x20, 0x40, 0x80
LABELS_OUT_MOVES, LABELS_OUT_BEST, LABELS_OUT_ACTION = 0x01, 0x02, 0x04

EXPORTS = ("ts_targets_abi_version", "ts_targets_last_hip_error", "ts_targets_supported", "ts_traj_returns", "ts_traj_labels",
           "ts_describe_traj_returns", "ts_describe_traj_labels")


class ReturnsIn(C.Structure):
    """ts_returns_in: the log (c[0] = first, the cells after step k = pos_log[k], flags_log), the values, gamma, lambda and the
    six reward weights."""
    _fields_ = [("first", C.c_void_p), ("pos_log", C.c_void_p), ("flags_log", C.c_void_p), ("values", C.c_void_p),
                ("last_value", C.c_void_p), ("steps", C.c_int32), ("value_stride", C.c_int32), ("gamma", C.c_float), ("lam", C.c_float),
                ("w_step", C.c_float), ("w_win", C.c_float), ("w_timeout", C.c_float), ("w_invalid", C.c_float), ("w_dist", C.c_float),
                ("w_progress", C.c_float)]


class ReturnsOut(C.Structure):
    """ts_returns_out: float32 [K][N] reward, adv, ret and uint8 [K][N] mask; each optional."""
    _fields_ = [("reward", C.c_void_p), ("adv", C.c_void_p), ("ret", C.c_void_p), ("mask", C.c_void_p)]


class LabelsIn(C.Structure):
    """ts_labels_in: the cells of the samples, the table and its rows."""
    _fields_ = [("first", C.c_void_p), ("pos_log", C.c_void_p), ("table", C.c_void_p), ("rows", C.c_void_p), ("n_rows", C.c_int64),
                ("steps", C.c_int32), ("reserved", C.c_int32)]


class LabelsOut(C.Structure):
    """ts_labels_out: int16 moves, uint8 best, uint8 action, each [K][N] and optional."""
    _fields_ = [("moves", C.c_void_p), ("best", C.c_void_p), ("action", C.c_void_p)]


class TargetsDesc(Desc):
    """ts_targets_desc: what one ts_traj_returns / ts_traj_labels would launch."""
    _fields_ = [("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32), ("chunk_steps", C.c_int32), ("reserved", C.c_int32),
                ("blocks", C.c_int64), ("samples", C.c_int64), ("bytes_read", C.c_int64), ("bytes_written", C.c_int64),
                ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_targets_supported.argtypes = [DP, C.c_int32]
    L.ts_targets_supported.restype = C.c_int32
    L.ts_traj_returns.argtypes = [DP, SP, C.POINTER(ReturnsIn), C.POINTER(ReturnsOut), P]
    L.ts_traj_returns.restype = C.c_int32
    L.ts_traj_labels.argtypes = [DP, SP, C.POINTER(LabelsIn), C.POINTER(LabelsOut), P]
    L.ts_traj_labels.restype = C.c_int32
    for name in ("ts_describe_traj_returns", "ts_describe_traj_labels"):
        fn = getattr(L, name)
        fn.argtypes = [DP, C.c_int32, C.c_uint32, C.POINTER(TargetsDesc)]
        fn.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def targets_supported(dims, which):
    """ts_targets_supported(dims, RETURNS or LABELS) as a bool; raises for invalid dims.  No GPU needed."""
    rc = lib().ts_targets_supported(C.byref(dims), int(which))
    if rc < 0:
        check(rc, "ts_targets_supported")
    return rc == 1


def _describe(name, dims, steps, what):
    desc = TargetsDesc()
    check(getattr(lib(), name)(C.byref(dims), int(steps), int(what), C.byref(desc)), name)
    return desc.as_dict()


def describe_traj_returns(dims, steps=1, what=RETURNS_OUT_REWARD | RETURNS_OUT_ADV | RETURNS_OUT_RET | RETURNS_OUT_MASK):
    """dict of ts_describe_traj_returns: the launch ts_traj_returns would make for the outputs and inputs of `what`.  No GPU needed."""
    return _describe("ts_describe_traj_returns", dims, steps, what)


def describe_traj_labels(dims, steps=1, what=LABELS_OUT_MOVES | LABELS_OUT_BEST | LABELS_OUT_ACTION):
    """dict of ts_describe_traj_labels: the launch ts_traj_labels would make for the outputs of `what`.  No GPU needed."""
    return _describe("ts_describe_traj_labels", dims, steps, what)
