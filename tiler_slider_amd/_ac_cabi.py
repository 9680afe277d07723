"""ctypes binding of lib/libtiler_slider_ac.so — the actor-critic network's C-ABI declared in include/tiler_slider_ac.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES, which says why it is a library of its own.  There is no CPU fallback: if the library is missing or does
not load, every entry point raises.
The network it shares with the policy and train libraries, value head included, is csrc/ts_mlp.h, listed through
_train_cabi.HEADERS.
"""
import ctypes as C
import os

from . import _cabi, _train_cabi
from ._cabi import Dims, State
from ._train_cabi import Mlp, MlpGrad, TrainDesc, TrainIn

SRC = os.path.join(_cabi._PKG, "csrc", "ts_ac.hip")
HEADERS = _train_cabi.HEADERS + [os.path.join(_cabi.ROOT, "include", "tiler_slider_ac.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_ac.so")
HEADER, PREFIX, LABEL = "tiler_slider_ac.h", "ts_ac_", "actor-critic "

ABI_VERSION = 1
MIN_KERNELS = 16  # k_ac_forward<1 .. 8> and k_ac_backward<1 .. 8>: what compile_guarded must find

EXPORTS = ("ts_ac_abi_version", "ts_ac_last_hip_error", "ts_ac_supported", "ts_ac_forward", "ts_ac_backward",
           "ts_describe_ac_forward", "ts_describe_ac_backward")


class ValueHead(C.Structure):
    """ts_value_head: v = bv[0] + sum_j wv[j] h_j on the hidden layer of a ts_mlp."""
    _fields_ = [("wv", C.c_void_p), ("bv", C.c_void_p)]


class ValueHeadGrad(C.Structure):
    """ts_value_head_grad: two device buffers in the layouts of ts_value_head, added into."""
    _fields_ = [("wv", C.c_void_p), ("bv", C.c_void_p)]


def _declare(L):
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_ac_supported.argtypes = [DP, C.c_int32]
    L.ts_ac_supported.restype = C.c_int32
    L.ts_ac_forward.argtypes = [DP, SP, C.POINTER(Mlp), C.POINTER(ValueHead), C.POINTER(TrainIn), P, P, P]
    L.ts_ac_forward.restype = C.c_int32
    L.ts_ac_backward.argtypes = [DP, SP, C.POINTER(Mlp), C.POINTER(ValueHead), C.POINTER(TrainIn), P, P, C.POINTER(MlpGrad),
                                 C.POINTER(ValueHeadGrad), P]
    L.ts_ac_backward.restype = C.c_int32
    for name in ("ts_describe_ac_forward", "ts_describe_ac_backward"):
        fn = getattr(L, name)
        fn.argtypes = [DP, C.c_int32, C.c_int32, C.POINTER(TrainDesc)]
        fn.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def ac_supported(dims, hidden):
    """ts_ac_supported(dims, hidden) as a bool; raises for invalid dims.  No GPU needed."""
    rc = lib().ts_ac_supported(C.byref(dims), int(hidden))
    if rc < 0:
        check(rc, "ts_ac_supported")
    return rc == 1


def _describe(name, dims, hidden, steps):
    desc = TrainDesc()
    check(getattr(lib(), name)(C.byref(dims), int(hidden), int(steps), C.byref(desc)), name)
    return desc.as_dict()


def describe_ac_forward(dims, hidden, steps=1):
    """dict of ts_describe_ac_forward: the launch ts_ac_forward would make.  No GPU needed."""
    return _describe("ts_describe_ac_forward", dims, hidden, steps)


def describe_ac_backward(dims, hidden, steps=1):
    """dict of ts_describe_ac_backward: the launch ts_ac_backward would make.  No GPU needed."""
    return _describe("ts_describe_ac_backward", dims, hidden, steps)
