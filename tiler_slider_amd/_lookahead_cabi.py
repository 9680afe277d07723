"""ctypes binding of lib/libtiler_slider_lookahead.so — the lookahead's C-ABI declared in include/tiler_slider_lookahead.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES; it is an entry of _libraries.SINCE, which says why it is not one of LIBRARIES.  There is no CPU fallback:
if the library is missing or does not load, every entry point raises.
The network it shares with the policy, train and actor-critic libraries, value head included, is csrc/ts_mlp.h, listed through
_ac_cabi.HEADERS.
"""
import ctypes as C
import os

from . import _ac_cabi, _cabi
from ._ac_cabi import ValueHead
from ._cabi import Desc, Dims, State
from ._train_cabi import Mlp, TrainIn

SRC = os.path.join(_cabi._PKG, "csrc", "ts_lookahead.hip")
HEADERS = _ac_cabi.HEADERS + [os.path.join(_cabi.ROOT, "include", "tiler_slider_lookahead.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_lookahead.so")
HEADER, PREFIX, LABEL = "tiler_slider_lookahead.h", "ts_lookahead_", "lookahead "

ABI_VERSION = 1
MAX_DEPTH = 4
NO_ACTION = 255
LEAVES = {"zero": 0, "value": 1, "qmax": 2}
MIN_KERNELS = 32  # k_lookahead<1 .. 8, 1 .. 4>: what compile_guarded must find

EXPORTS = ("ts_lookahead_abi_version", "ts_lookahead_last_hip_error", "ts_lookahead_supported", "ts_lookahead", "ts_describe_lookahead")


class LookaheadCfg(C.Structure):
    """ts_lookahead_cfg: the depth, the leaf kind, the discount and the three reward weights of one search."""
    _fields_ = [("depth", C.c_int32), ("leaf", C.c_int32), ("gamma", C.c_float), ("w_step", C.c_float), ("w_win", C.c_float),
                ("w_invalid", C.c_float), ("reserved", C.c_int32 * 2)]


class LookaheadOut(C.Structure):
    """ts_lookahead_out: four device buffers, each optional but not all."""
    _fields_ = [("q", C.c_void_p), ("value", C.c_void_p), ("best", C.c_void_p), ("win_in", C.c_void_p)]


OUT_FIELDS = tuple(f for f, _ in LookaheadOut._fields_)


class LookaheadDesc(Desc):
    """ts_lookahead_desc: what one ts_lookahead would launch."""
    _fields_ = [("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32), ("weights_in_lds", C.c_int32), ("leaf_is_template", C.c_int32),
                ("depth", C.c_int32), ("reserved", C.c_int32), ("blocks", C.c_int64), ("samples", C.c_int64), ("leaves", C.c_int64),
                ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_lookahead_supported.argtypes = [DP, C.c_int32, C.c_int32]
    L.ts_lookahead_supported.restype = C.c_int32
    L.ts_lookahead.argtypes = [DP, SP, C.POINTER(Mlp), C.POINTER(ValueHead), C.POINTER(TrainIn), C.POINTER(LookaheadCfg),
                               C.POINTER(LookaheadOut), P]
    L.ts_lookahead.restype = C.c_int32
    L.ts_describe_lookahead.argtypes = [DP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(LookaheadDesc)]
    L.ts_describe_lookahead.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def lookahead_supported(dims, hidden, leaf):
    """ts_lookahead_supported(dims, hidden, leaf) as a bool, `leaf` one of LEAVES' values; raises for invalid dims or an unknown
    leaf.  No GPU needed."""
    rc = lib().ts_lookahead_supported(C.byref(dims), int(hidden), int(leaf))
    if rc < 0:
        check(rc, "ts_lookahead_supported")
    return rc == 1


def describe_lookahead(dims, hidden, steps=1, depth=2, leaf=1):
    """dict of ts_describe_lookahead: the launch ts_lookahead would make.  No GPU needed."""
    desc = LookaheadDesc()
    check(lib().ts_describe_lookahead(C.byref(dims), int(hidden), int(steps), int(depth), int(leaf), C.byref(desc)), "ts_describe_lookahead")
    return desc.as_dict()
