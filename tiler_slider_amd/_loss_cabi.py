"""ctypes binding of lib/libtiler_slider_loss.so — the fused actor-critic loss' C-ABI declared in include/tiler_slider_loss.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES, which says why it is a library of its own.  There is no CPU fallback: if the library is missing or does
not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Desc

SRC = os.path.join(_cabi._PKG, "csrc", "ts_loss.hip")
HEADERS = _cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi.ROOT, "include", h) for h in ("tiler_slider_search.h", "tiler_slider_loss.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_loss.so")
HEADER, PREFIX, LABEL = "tiler_slider_loss.h", "ts_loss_", "loss "

ABI_VERSION = 1
MIN_KERNELS = 3  # k_loss_stats, k_loss_main and k_loss_finish: what compile_guarded must find

THREADS, MAX_BLOCKS, SCALARS = 256, 2048, 8
OLD_LOGITS, VALUES, ADV, MASK = 0x01, 0x02, 0x04, 0x08

EXPORTS = ("ts_loss_abi_version", "ts_loss_last_hip_error", "ts_loss_workspace_bytes", "ts_actor_critic_loss", "ts_describe_loss")


class LossIn(C.Structure):
    """ts_loss_in: the network's outputs, the old policy's, the actions or labels, the targets and the coefficients."""
    _fields_ = [("logits", C.c_void_p), ("old_logits", C.c_void_p), ("act", C.c_void_p), ("mask", C.c_void_p), ("adv", C.c_void_p),
                ("values", C.c_void_p), ("ret", C.c_void_p), ("n_samples", C.c_int64), ("clip", C.c_float), ("value_coef", C.c_float),
                ("entropy_coef", C.c_float), ("normalize_adv", C.c_int32)]


class LossOut(C.Structure):
    """ts_loss_out: float32 dlogits [M][4], dvalues [M], scalars [8] and the workspace of the partial sums."""
    _fields_ = [("dlogits", C.c_void_p), ("dvalues", C.c_void_p), ("scalars", C.c_void_p), ("workspace", C.c_void_p)]


class LossDesc(Desc):
    """ts_loss_desc: what one ts_actor_critic_loss would launch."""
    _fields_ = [("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32), ("launches", C.c_int32), ("reserved", C.c_int32),
                ("blocks", C.c_int64), ("partials", C.c_int64), ("samples", C.c_int64), ("workspace_bytes", C.c_int64),
                ("bytes_read", C.c_int64), ("bytes_written", C.c_int64), ("name", C.c_char * 64), ("stats_name", C.c_char * 32),
                ("finish_name", C.c_char * 32)]

    def as_dict(self):
        d = super().as_dict()
        d["stats_name"], d["finish_name"] = self.stats_name.decode(), self.finish_name.decode()
        return d


def _declare(L):
    L.ts_loss_workspace_bytes.argtypes = [C.c_int64]
    L.ts_loss_workspace_bytes.restype = C.c_int64
    L.ts_actor_critic_loss.argtypes = [C.POINTER(LossIn), C.POINTER(LossOut), C.c_void_p]
    L.ts_actor_critic_loss.restype = C.c_int32
    L.ts_describe_loss.argtypes = [C.c_int64, C.c_uint32, C.POINTER(LossDesc)]
    L.ts_describe_loss.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def workspace_bytes(n_samples):
    """ts_loss_workspace_bytes(n_samples); raises for a negative count.  No GPU needed."""
    n = lib().ts_loss_workspace_bytes(int(n_samples))
    if n < 0:
        check(int(n), "ts_loss_workspace_bytes")
    return n


def describe_loss(n_samples, what=0):
    """dict of ts_describe_loss: the launches ts_actor_critic_loss would make for the optional inputs of `what`.  No GPU needed."""
    desc = LossDesc()
    check(lib().ts_describe_loss(int(n_samples), int(what), C.byref(desc)), "ts_describe_loss")
    return desc.as_dict()
