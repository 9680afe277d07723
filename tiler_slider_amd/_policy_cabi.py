"""ctypes binding of lib/libtiler_slider_policy.so — the neural-policy rollouts' C-ABI declared in include/tiler_slider_policy.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES, which says why it is a library of its own.  There is no CPU fallback: if the library is missing or does
not load, every entry point raises.
The network's device functions and block plans are csrc/ts_mlp.h's, shared with the train and actor-critic libraries: HEADERS
lists it, so editing it marks all of them (and the targets library, which extends the same list) stale.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Desc, Dims, State

SRC = os.path.join(_cabi._PKG, "csrc", "ts_policy.hip")
# ts_mlp.h: the network that ts_policy.hip, ts_train.hip and ts_ac.hip share (_train_cabi, _targets_cabi and _ac_cabi extend this list)
HEADERS = _cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi._PKG, "csrc", "ts_mlp.h")] + [
    os.path.join(_cabi.ROOT, "include", h) for h in ("tiler_slider_search.h", "tiler_slider_table.h", "tiler_slider_rollout.h", "tiler_slider_policy.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_policy.so")
HEADER, PREFIX, LABEL = "tiler_slider_policy.h", "ts_policy_", "policy "

ABI_VERSION = 1
POLICY_MAX_HIDDEN = 64
GREEDY, SAMPLE = 0, 1
SELECTS = {"greedy": GREEDY, "sample": SAMPLE}
OUT_LOGITS_LOG = 0x200
MIN_KERNELS = 24  # k_policy_rollout<1 .. 8, GREEDY / SAMPLE> and k_policy_logits<1 .. 8>: what compile_guarded must find

EXPORTS = ("ts_policy_abi_version", "ts_policy_last_hip_error", "ts_policy_supported", "ts_policy_logits", "ts_policy_rollout",
           "ts_describe_policy_rollout", "ts_describe_policy_logits")


class Mlp(C.Structure):
    """ts_mlp of include/tiler_slider_policy.h: device pointers in the kernel layout, w1 [D][H], b1 [H], w2 [H][4], b2 [4]."""
    _fields_ = [("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p), ("hidden", C.c_int32), ("reserved", C.c_int32)]


class PolicyCfg(C.Structure):
    """ts_policy_cfg."""
    _fields_ = [("steps", C.c_int32), ("mode", C.c_uint32), ("select", C.c_int32), ("write_state", C.c_int32), ("seed", C.c_uint64),
                ("step_index", C.c_int64), ("board_offset", C.c_int64), ("explore_threshold", C.c_uint64)]


OUT_FIELDS = ("wins", "finished", "first_win", "win_moves", "reward_sum", "flags", "act_log", "flags_log", "pos_log", "logits_log")


class PolicyOut(C.Structure):
    """ts_policy_out: ten optional device pointers - the nine of ts_rollout_out in the order of their OUT_* bits, and logits_log."""
    _fields_ = [(name, C.c_void_p) for name in OUT_FIELDS]


class PolicyDesc(Desc):
    """ts_policy_desc: what one ts_policy_rollout / ts_policy_logits would launch."""
    _fields_ = [("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32), ("weights_in_lds", C.c_int32), ("reserved", C.c_int32),
                ("blocks", C.c_int64), ("logged_bytes", C.c_int64), ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_policy_supported.argtypes = [DP, C.c_int32]
    L.ts_policy_supported.restype = C.c_int32
    L.ts_policy_logits.argtypes = [DP, SP, C.POINTER(Mlp), P, P]
    L.ts_policy_logits.restype = C.c_int32
    L.ts_policy_rollout.argtypes = [DP, SP, C.POINTER(Mlp), C.POINTER(PolicyCfg), C.POINTER(PolicyOut), P]
    L.ts_policy_rollout.restype = C.c_int32
    L.ts_describe_policy_rollout.argtypes = [DP, C.c_int32, C.POINTER(PolicyCfg), C.c_uint32, C.POINTER(PolicyDesc)]
    L.ts_describe_policy_rollout.restype = C.c_int32
    L.ts_describe_policy_logits.argtypes = [DP, C.c_int32, C.POINTER(PolicyDesc)]
    L.ts_describe_policy_logits.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def policy_supported(dims, hidden):
    """ts_policy_supported(dims, hidden) as a bool; raises for invalid dims.  No GPU needed."""
    rc = lib().ts_policy_supported(C.byref(dims), int(hidden))
    if rc < 0:
        check(rc, "ts_policy_supported")
    return rc == 1


def describe_policy_rollout(dims, hidden, cfg, out_mask=0):
    """dict of ts_describe_policy_rollout: the launch ts_policy_rollout would make.  No GPU needed."""
    desc = PolicyDesc()
    check(lib().ts_describe_policy_rollout(C.byref(dims), int(hidden), C.byref(cfg), int(out_mask), C.byref(desc)), "ts_describe_policy_rollout")
    return desc.as_dict()


def describe_policy_logits(dims, hidden):
    """dict of ts_describe_policy_logits: the launch ts_policy_logits would make.  No GPU needed."""
    desc = PolicyDesc()
    check(lib().ts_describe_policy_logits(C.byref(dims), int(hidden), C.byref(desc)), "ts_describe_policy_logits")
    return desc.as_dict()
