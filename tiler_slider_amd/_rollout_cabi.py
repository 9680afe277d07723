"""ctypes binding of lib/libtiler_slider_rollout.so — the fused rollouts' C-ABI declared in include/tiler_slider_rollout.h.

A fourth library beside libtiler_slider_hip.so, libtiler_slider_search.so and libtiler_slider_table.so (all three are pinned
symbol by symbol and kernel by kernel, so the rollout kernels live in their own).  Same rules as _cabi.py: built through
_cabi.compile_guarded (hipcc --offload-arch=gfx950, VGPR hazard scan and padding), and there is no CPU fallback: if the library
is missing or does not load, every entry point raises.
"""
import ctypes as C
import os

from . import _cabi
from ._cabi import Dims, State, TilerSliderLibraryError

SRC = os.path.join(_cabi._PKG, "csrc", "ts_rollout.hip")
HEADERS = _cabi.HEADERS + [os.path.join(_cabi.ROOT, "include", h) for h in ("tiler_slider_search.h", "tiler_slider_table.h", "tiler_slider_rollout.h")]
LIB_PATH = os.path.join(_cabi._PKG, "lib", "libtiler_slider_rollout.so")

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


class RolloutDesc(C.Structure):
    """ts_rollout_desc: what one ts_rollout would launch."""
    _fields_ = [("threads_per_block", C.c_int32), ("lds_bytes", C.c_int32), ("blocks", C.c_int64), ("logged_bytes", C.c_int64),
                ("name", C.c_char * 64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["name"] = self.name.decode()
        return d


def _stale():
    if not os.path.exists(LIB_PATH):
        return True
    built = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(p) > built for p in [SRC] + HEADERS)


def build_library(force=False, verbose=False):
    """Compile the rollout kernels for gfx950 in-tree, through the same guarded steps as the other three libraries."""
    if not force and not _stale():
        return LIB_PATH
    _cabi.compile_guarded(SRC, LIB_PATH, verbose=verbose, keep_asm=os.environ.get("TS_KEEP_ASM") == "1", min_kernels=MIN_KERNELS)
    return LIB_PATH


_lib = None


def lib():
    """The loaded rollout library; raises (never falls back) when it is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TilerSliderLibraryError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback.")
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:
        raise TilerSliderLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    missing = [s for s in EXPORTS if not hasattr(L, s)]
    if missing:
        raise TilerSliderLibraryError(f"{LIB_PATH} lacks symbols {missing}; rebuild it")
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_rollout_abi_version.restype = C.c_int32
    L.ts_rollout_last_hip_error.restype = C.c_int32
    L.ts_rollout_supported.argtypes = [DP, C.c_int32]
    L.ts_rollout_supported.restype = C.c_int32
    L.ts_rollout.argtypes = [DP, SP, C.POINTER(RolloutCfg), C.POINTER(RolloutOut), P]
    L.ts_rollout.restype = C.c_int32
    L.ts_describe_rollout.argtypes = [DP, C.POINTER(RolloutCfg), C.c_uint32, C.POINTER(RolloutDesc)]
    L.ts_describe_rollout.restype = C.c_int32
    if L.ts_rollout_abi_version() != ABI_VERSION:
        raise TilerSliderLibraryError(f"rollout ABI version {L.ts_rollout_abi_version()} != {ABI_VERSION}; rebuild the library")
    _lib = L
    return L


def check(rc, what):
    if rc != _cabi.OK:
        msg = _cabi.lib().ts_status_string(rc).decode()  # the status codes are the step library's
        extra = f" (hipError {lib().ts_rollout_last_hip_error()})" if rc == _cabi.ERR_HIP else ""
        raise TilerSliderLibraryError(f"{what}: {msg}{extra}")


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
