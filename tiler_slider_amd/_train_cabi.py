"""ctypes binding of lib/libtiler_slider_train.so — the trainable policies' C-ABI declared in include/tiler_slider_train.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES, which says why it is a library of its own.  There is no CPU fallback: if the library is missing or does
not load, every entry point raises.
The network it shares with the policy library is csrc/ts_mlp.h, which _policy_cabi.HEADERS lists.
"""
import ctypes as C
import os

from . import _cabi, _policy_cabi
from ._cabi import Desc, Dims, State
from ._policy_cabi import Mlp

SRC = os.path.join(_cabi._PKG, "csrc", "ts_train.hip")
HEADERS = _policy_cabi.HEADERS + [os.path.join(_cabi.ROOT, "include", "tiler_slider_train.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_train.so")
HEADER, PREFIX, LABEL = "tiler_slider_train.h", "ts_train_", "train "

ABI_VERSION = 1
MIN_KERNELS = 16  # k_train_forward<1 .. 8> and k_train_backward<1 .. 8>: what compile_guarded must find

EXPORTS = ("ts_train_abi_version", "ts_train_last_hip_error", "ts_train_supported", "ts_train_forward", "ts_train_backward",
           "ts_describe_train_forward", "ts_describe_train_backward")


class TrainIn(C.Structure):
    """ts_train_in: the cells of the samples - c[0] = first [T][N], c[k] = pos_log[k - 1] of a rollout's [K][T][N] log."""
    _fields_ = [("first", C.c_void_p), ("pos_log", C.c_void_p), ("steps", C.c_int32), ("reserved", C.c_int32)]


class MlpGrad(C.Structure):
    """ts_mlp_grad: four device buffers in the layouts of ts_mlp, added into."""
    _fields_ = [("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p)]


class TrainDesc(Desc):
    """ts_train_desc: what one ts_train_forward / ts_train_backward would launch."""
    _fields_ = [("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32), ("weights_in_lds", C.c_int32), ("grads_in_lds", C.c_int32),
                ("chunk_steps", C.c_int32), ("reserved", C.c_int32), ("blocks", C.c_int64), ("samples", C.c_int64),
                ("flush_bytes", C.c_int64), ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_train_supported.argtypes = [DP, C.c_int32]
    L.ts_train_supported.restype = C.c_int32
    L.ts_train_forward.argtypes = [DP, SP, C.POINTER(Mlp), C.POINTER(TrainIn), P, P]
    L.ts_train_forward.restype = C.c_int32
    L.ts_train_backward.argtypes = [DP, SP, C.POINTER(Mlp), C.POINTER(TrainIn), P, C.POINTER(MlpGrad), P]
    L.ts_train_backward.restype = C.c_int32
    for name in ("ts_describe_train_forward", "ts_describe_train_backward"):
        fn = getattr(L, name)
        fn.argtypes = [DP, C.c_int32, C.c_int32, C.POINTER(TrainDesc)]
        fn.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def train_supported(dims, hidden):
    """ts_train_supported(dims, hidden) as a bool; raises for invalid dims.  No GPU needed."""
    rc = lib().ts_train_supported(C.byref(dims), int(hidden))
    if rc < 0:
        check(rc, "ts_train_supported")
    return rc == 1


def _describe(name, dims, hidden, steps):
    desc = TrainDesc()
    check(getattr(lib(), name)(C.byref(dims), int(hidden), int(steps), C.byref(desc)), name)
    return desc.as_dict()


def describe_train_forward(dims, hidden, steps=1):
    """dict of ts_describe_train_forward: the launch ts_train_forward would make.  No GPU needed."""
    return _describe("ts_describe_train_forward", dims, hidden, steps)


def describe_train_backward(dims, hidden, steps=1):
    """dict of ts_describe_train_backward: the launch ts_train_backward would make.  No GPU needed."""
    return _describe("ts_describe_train_backward", dims, hidden, steps)
