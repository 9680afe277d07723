"""ctypes binding of lib/libtiler_slider_rollout.so — the fused rollouts' C-ABI declared in include/tiler_slider_rollout.h.

Built through _cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding) like every entry of
_libraries.LIBRARIES, which says why it is a library of its own.  There is no CPU fallback: if the library is missing or does
not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Desc, Dims, State

SRC = os.path.join(_cabi._PKG, "csrc", "ts_rollout.hip")
HEADERS = _cabi.HEADERS + _cabi.SHARED_HEADERS + [os.path.join(_cabi.ROOT, "include", h) for h in ("tiler_slider_search.h", "tiler_slider_table.h", "tiler_slider_rollout.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_rollout.so")
HEADER, PREFIX, LABEL = "tiler_slider_rollout.h", "ts_rollout_", "rollout "

ABI_VERSION = 1
ROLLOUT_MAX_STEPS, ROLLOUT_MAX_SIZE, ROLLOUT_MAX_TILES = 65535, 8, 8
GIVEN, RANDOM, TABLE = 0, 1, 2
POLICIES = {"given": GIVEN, "random": RANDOM, "table": TABLE}
OUT_WINS, OUT_FINISHED, OUT_FIRST_WIN, OUT_WIN_MOVES, OUT_REWARD_SUM = 0x001, 0x002, 0x004, 0x008, 0x010
OUT_FLAGS, OUT_ACT_LOG, OUT_FLAGS_LOG, OUT_POS_LOG = 0x020, 0x040, 0x080, 0x100
MIN_KERNELS = 24  # k_rollout<1 .. 8, GIVEN / RANDOM / TABLE>: what compile_guarded must find in the device assembly

EXPORTS = ("ts_rollout_abi_version", "ts_rollout_last_hip_error", "ts_rollout_supported", "ts_rollout", "ts_describe_rollout")


class RolloutCfg(C.Structure):
    """ts_rollout_cfg of include/tiler_slider_rollout.h."""
    _fields_ = [("steps", C.c_int32), ("mode", C.c_uint32), ("policy", C.c_int32), ("write_state", C.c_int32), ("actions", C.c_void_p),
                ("seed", C.c_uint64), ("step_index", C.c_int64), ("board_offset", C.c_int64), ("explore_threshold", C.c_uint64),
                ("table", C.c_void_p), ("n_rows", C.c_int64), ("rows", C.c_void_p)]


OUT_FIELDS = ("wins", "finished", "first_win", "win_moves", "reward_sum", "flags", "act_log", "flags_log", "pos_log")


class RolloutOut(C.Structure):
    """ts_rollout_out: nine optional device pointers, in the order of the OUT_* bits."""
    _fields_ = [(name, C.c_void_p) for name in OUT_FIELDS]


class RolloutDesc(Desc):
    """ts_rollout_desc: what one ts_rollout would launch."""
    _fields_ = [("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32), ("blocks", C.c_int64), ("logged_bytes", C.c_int64),
                ("name", C.c_char * 64)]


def _declare(L):
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_rollout_supported.argtypes = [DP, C.c_int32]
    L.ts_rollout_supported.restype = C.c_int32
    L.ts_rollout.argtypes = [DP, SP, C.POINTER(RolloutCfg), C.POINTER(RolloutOut), P]
    L.ts_rollout.restype = C.c_int32
    L.ts_describe_rollout.argtypes = [DP, C.POINTER(RolloutCfg), C.c_uint32, C.POINTER(RolloutDesc)]
    L.ts_describe_rollout.restype = C.c_int32


_lib = None
build_library, lib, check = _cabi.bind(__name__, _declare)


def rollout_supported(dims, policy):
    """ts_rollout_supported(dims, policy) as a bool; raises for invalid dims or an unknown policy.  No GPU needed."""
    rc = lib().ts_rollout_supported(C.byref(dims), int(policy))
    if rc < 0:
        check(rc, "ts_rollout_supported")
    return rc == 1


def describe_rollout(dims, cfg, out_mask=0):
    """dict of ts_describe_rollout(dims, cfg, out_mask): the launch ts_rollout would make.  No GPU needed."""
    desc = RolloutDesc()
    check(lib().ts_describe_rollout(C.byref(dims), C.byref(cfg), int(out_mask), C.byref(desc)), "ts_describe_rollout")
    return desc.as_dict()
