"""ctypes binding of lib/libtiler_slider_optim.so — the fused optimiser's C-ABI declared in include/tiler_slider_optim.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES, which says why it is a library of its own.  There is no CPU fallback: if the library is missing or does
not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Desc

SRC = os.path.join(_cabi._PKG, "csrc", "ts_optim.hip")
HEADERS = _cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi.ROOT, "include", h) for h in ("tiler_slider_search.h", "tiler_slider_optim.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_optim.so")
HEADER, PREFIX, LABEL = "tiler_slider_optim.h", "ts_optim_", "optim "

ABI_VERSION = 1
MIN_KERNELS = 4  # k_optim_one, k_optim_norm, k_optim_apply and k_optim_finish: what compile_guarded must find

MAX_TENSORS, THREADS, ONE_THREADS, CHUNK, ONE_CHUNK, MAX_BLOCKS = 32, 256, 1024, 1024, 256, 1024
FORM_NONE, FORM_ONE, FORM_MULTI, FORM_APPLY = 0, 1, 2, 3
NORM, ZERO_GRAD = 0x01, 0x02
TUNE_ONE_BLOCK_MAX = 0

EXPORTS = ("ts_optim_abi_version", "ts_optim_last_hip_error", "ts_optim_tuning", "ts_optim_workspace_bytes", "ts_adam_step",
           "ts_describe_adam_step")

_PTRS = C.c_void_p * MAX_TENSORS


class OptimTensors(C.Structure):
    """ts_optim_tensors: up to 32 tensors, each numel float32 elements in param, grad, m and v."""
    _fields_ = [("n_tensors", C.c_int32), ("reserved", C.c_int32), ("numel", C.c_int64 * MAX_TENSORS), ("param", _PTRS), ("grad", _PTRS),
                ("m", _PTRS), ("v", _PTRS)]


class AdamCfg(C.Structure):
    """ts_adam_cfg: the betas as doubles, lr by value or from the device, and what the call does besides the update."""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("lr_dev", C.c_void_p), ("lr", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("max_grad_norm", C.c_float), ("skip_nonfinite", C.c_int32), ("zero_grad", C.c_int32)]


class OptimOut(C.Structure):
    """ts_optim_out: int64 counters [2], float32 grad_norm [1] (optional) and the workspace of the partial sums."""
    _fields_ = [("counters", C.c_void_p), ("grad_norm", C.c_void_p), ("workspace", C.c_void_p)]


class OptimDesc(Desc):
    """ts_optim_desc: what one ts_adam_step would launch."""
    _fields_ = [("form", C.c_int32), ("launches", C.c_int32), ("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32),
                ("blocks", C.c_int64), ("chunks", C.c_int64), ("total_numel", C.c_int64), ("workspace_bytes", C.c_int64),
                ("bytes_read", C.c_int64), ("bytes_written", C.c_int64), ("name", C.c_char * 32), ("norm_name", C.c_char * 32),
                ("finish_name", C.c_char * 32)]

    def as_dict(self):
        d = super().as_dict()
        d["norm_name"], d["finish_name"] = self.norm_name.decode(), self.finish_name.decode()
        return d


def _declare(L):
    L.ts_optim_tuning.argtypes = [C.c_int32, C.c_int64]
    L.ts_optim_tuning.restype = C.c_int64
    L.ts_optim_workspace_bytes.argtypes = [C.c_int64]
    L.ts_optim_workspace_bytes.restype = C.c_int64
    L.ts_adam_step.argtypes = [C.POINTER(OptimTensors), C.POINTER(AdamCfg), C.POINTER(OptimOut), C.c_void_p]
    L.ts_adam_step.restype = C.c_int32
    L.ts_describe_adam_step.argtypes = [C.c_int32, C.POINTER(C.c_int64), C.c_uint32, C.POINTER(OptimDesc)]
    L.ts_describe_adam_step.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def workspace_bytes(total_numel):
    """ts_optim_workspace_bytes(total_numel); raises for a negative total.  No GPU needed."""
    n = lib().ts_optim_workspace_bytes(int(total_numel))
    if n < 0:
        check(int(n), "ts_optim_workspace_bytes")
    return n


def tuning(key, value=-1):
    """ts_optim_tuning(key, value): value >= 0 sets the knob, a negative one reads it; the value before the call."""
    return lib().ts_optim_tuning(int(key), int(value))


def describe_adam_step(numels, what=NORM):
    """dict of ts_describe_adam_step: the launches ts_adam_step would make on tensors of these sizes.  No GPU needed."""
    numels = [int(x) for x in numels]
    arr = (C.c_int64 * max(1, len(numels)))(*numels)
    desc = OptimDesc()
    check(lib().ts_describe_adam_step(len(numels), arr, int(what), C.byref(desc)), "ts_describe_adam_step")
    return desc.as_dict()
