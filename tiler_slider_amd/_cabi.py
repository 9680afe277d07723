"""ctypes binding of lib/libtiler_slider_hip.so — the C-ABI declared in include/tiler_slider.h.

There is no CPU fallback: if the shared library is missing or does not load, every entry
point raises.  Build it with `python -c "import __graft_entry__ as g; g.build()"` or
`tiler_slider_amd.build_library()` (hipcc --offload-arch=gfx950).
"""
import ctypes as C
import os
import shutil
import subprocess
import sys

_PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_PKG)
SRC = os.path.join(_PKG, "csrc", "ts_kernels.hip")
HEADERS = [os.path.join(_PKG, "csrc", "ts_core.h"), os.path.join(ROOT, "include", "tiler_slider.h")]
LIB_PATH = os.path.join(_PKG, "lib", "libtiler_slider_hip.so")
# what every other library's source shares beyond ts_core.h: the index space and the host side of a launch
SHARED_HEADERS = [os.path.join(_PKG, "csrc", h) for h in ("ts_index.h", "ts_launch.h")]

HEADER, PREFIX, LABEL = "tiler_slider.h", "ts_", ""  # the public header, the symbol prefix, the library's name in the ABI-mismatch message
ABI_VERSION = 6
MIN_KERNELS = None  # hundreds of kernels: compile_guarded recognises a parse failure by "no kernel fills its allocation"
OK, ERR_NULL, ERR_DIMS, ERR_LIMIT, ERR_HIP, ERR_ARG = 0, -1, -2, -3, -4, -5
FLAG_IS_WON, FLAG_INVALID_MOVE, FLAG_SUCCESS, FLAG_TIMEOUT = 0x01, 0x02, 0x04, 0x08
FLAG_STEPPED_DONE, FLAG_AUTORESET, FLAG_BAD_ACTION = 0x10, 0x20, 0x40
MODE_STRICT, MODE_AUTORESET = 0, 1
TUNE_MULTI_MIN_BOARDS, TUNE_NT_THRESHOLD_BYTES, TUNE_LINES_LANES, TUNE_LINES_BPW, TUNE_EMIT_EDGES, TUNE_XCD_PIECE = 0, 1, 2, 3, 4, 5
TUNE_DEAL, TUNE_MT_WINDOW, TUNE_SMALL_BPW, TUNE_CACHED_EVERY, TUNE_STATE_ONLY, TUNE_LINES_WAVES, TUNE_SMALL_WAVES = 6, 7, 8, 9, 10, 11, 12

EXPORTS = ("ts_abi_version", "ts_limits", "ts_status_string", "ts_last_hip_error", "ts_blk_words", "ts_cell_bytes",
           "ts_onehot_channels", "ts_check_dims", "ts_reset", "ts_step", "ts_valid_moves", "ts_is_won", "ts_encode",
           "ts_encode_u8", "ts_expand_u8", "ts_encode_onehot", "ts_reward", "ts_generate", "ts_fill_actions",
           "ts_lines_words", "ts_prepare", "ts_generate_mt19937", "ts_tuning", "ts_valid_moves4", "ts_describe_launch",
           "ts_handoff_layout", "ts_pack_handoff", "ts_unpack_handoff")


class Dims(C.Structure):
    _fields_ = [("n_boards", C.c_int64), ("size", C.c_int32), ("n_tiles", C.c_int32), ("n_targets", C.c_int32),
                ("multi_color", C.c_int32), ("max_steps", C.c_int32), ("launch_hint", C.c_int32), ("emit_edges", C.c_int32),
                ("lines_lanes", C.c_int32), ("xcd_piece", C.c_int32), ("ring_bytes", C.c_int64)]


class State(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("init", C.c_void_p), ("tgt", C.c_void_p), ("blk", C.c_void_p),
                ("step_count", C.c_void_p), ("done", C.c_void_p), ("lines", C.c_void_p)]


class StepOut(C.Structure):
    _fields_ = [("flags", C.c_void_p), ("obs", C.c_void_p), ("reward", C.c_void_p), ("onehot", C.c_void_p),
                ("valid", C.c_void_p), ("obs_u8", C.c_void_p), ("valid4", C.c_void_p)]


OP_STEP, OP_RESET, OP_OBSERVE = 0, 1, 2
HANDOFF_CELLS, HANDOFF_REWARD, HANDOFF_STEP_COUNT = 0x1, 0x2, 0x4
OUT_OBS, OUT_REWARD, OUT_ONEHOT, OUT_VALID, OUT_OBS_U8, OUT_VALID4, OUT_FLAGS = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40
KERNEL_NAMES = {0: "none", 1: "k_small", 2: "k_multi", 3: "k_deal", 4: "k_lines", 5: "k_state", 6: "k_step_update"}


class Desc(C.Structure):
    """A ts_*_desc: what one call would launch, as_dict() for the describe_* functions."""

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["name"] = self.name.decode()
        return d


class LaunchDesc(Desc):
    """ts_launch_desc of include/tiler_slider.h: what one call of the hot path would launch."""
    _fields_ = [("kernel", C.c_int32), ("out_of_cache", C.c_int32), ("lanes_per_board", C.c_int32), ("boards_per_lane", C.c_int32),
                ("boards_per_wave", C.c_int32), ("tiles_per_lane", C.c_int32), ("extras", C.c_int32), ("wide", C.c_int32),
                ("cached_every", C.c_int32), ("emit_edges", C.c_int32), ("xcd_piece", C.c_int32), ("waves_per_block", C.c_int32),
                ("blocks_per_cu", C.c_int32), ("lds_bytes_block", C.c_int32), ("lds_bytes_used", C.c_int32), ("reserved", C.c_int32),
                ("blocks", C.c_int64), ("output_bytes", C.c_int64), ("resident_bytes", C.c_int64), ("name", C.c_char * 64)]


def describe_launch(dims, op=OP_STEP, outputs=OUT_OBS):
    """dict of ts_describe_launch(dims, op, outputs): the launch ts_step / ts_reset / ts_encode ... would make.  No GPU needed.
    A Dims object that an environment has marked `step_in_place` (VecTilerSliderEnv(obs_update=...): its steps go through
    ts_step_update) answers OP_STEP with ts_describe_step_update's record instead: the kernel that actually runs."""
    if op == OP_STEP and getattr(dims, "step_in_place", False):
        from . import _update_cabi
        return _update_cabi.describe_step_update(dims, outputs & ~OUT_FLAGS)
    desc = LaunchDesc()
    check(lib().ts_describe_launch(C.byref(dims), op, outputs, C.byref(desc)), "ts_describe_launch")
    return desc.as_dict()


class TilerSliderLibraryError(RuntimeError):
    pass


_LLVM_BIN = "/opt/rocm/lib/llvm/bin"


def pad_vgpr_allocations(asm, hits=None):
    """(patched assembly, number of kernels padded): see _vgpr_guard.pad_vgpr_allocations."""
    from . import _vgpr_guard
    try:
        out, padded = _vgpr_guard.pad_vgpr_allocations(asm, hits)
    except ValueError as e:
        raise TilerSliderLibraryError(str(e)) from e
    return out, len(padded)


def _run(cmd, verbose):
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise TilerSliderLibraryError(f"build step failed ({res.returncode}): {' '.join(cmd)}")


def compile_guarded(src, out_lib, defines=(), work=None, verbose=False, keep_asm=False, min_kernels=None):
    """hipcc's own steps (`hipcc -###`) taken apart so that the device assembly can be post-processed between compiler
    and assembler:  device code -> assembly -> [scan the unpadded object, pad VGPR allocations] -> object -> code object
    -> [scan again: any finding fails the build] -> fat binary -> host compile.  The gfx950 hazard and the padding policy
    are described in _vgpr_guard.py.  `defines`: extra -D flags (tools/variant_bench.py builds its A/B variants through
    this function, so that no variant runs without the guard).  `min_kernels`: how a parse failure of the kernel metadata
    is recognised.  None (the step library, hundreds of kernels): no kernel at all fills its register allocation.  A code
    object of a handful of kernels can honestly have none that does; for such a library pass the number of kernels it
    must hold at least: fewer parsed, or one parsed without registers, is the failure.  Returns the guard's report (also
    written next to the intermediate files: vgpr_guard.json, or <library>.gfx950.vgpr_guard.json with min_kernels)."""
    import json
    from . import _vgpr_guard as guard
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise TilerSliderLibraryError(f"hipcc not found: cannot build {os.path.basename(out_lib)}")
    work = work or os.path.join(ROOT, "build", "lib")
    os.makedirs(work, exist_ok=True)
    os.makedirs(os.path.dirname(out_lib), exist_ok=True)
    base = os.path.join(work, os.path.splitext(os.path.basename(out_lib))[0] + ".gfx950")
    common = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", *defines]

    def assemble(asm_path, tag):
        _run([f"{_LLVM_BIN}/clang", "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c", asm_path, "-o", base + tag + ".o"], verbose)
        _run([f"{_LLVM_BIN}/lld", "-flavor", "gnu", "-m", "elf64_amdgpu", "--no-undefined", "-shared", "-o", base + tag + ".hsaco", base + tag + ".o"], verbose)
        return base + tag + ".hsaco"

    _run([hipcc, *common, "-S", "--cuda-device-only", "-o", base + ".raw.s", src], verbose)
    raw = open(base + ".raw.s").read()
    a0, b0, counts0 = guard.scan_code_object(assemble(base + ".raw.s", ".raw"))
    hits = {k for k, _ in a0} | {k for k, _ in b0}
    try:
        asm, padded = guard.pad_vgpr_allocations(raw, hits)
    except ValueError as e:
        raise TilerSliderLibraryError(str(e)) from e
    open(base + ".s", "w").write(asm)
    hsaco = assemble(base + ".s", "")
    a1, b1, counts1 = guard.scan_code_object(hsaco)
    full = sorted(k for k, (n, ag) in counts0.items() if n and (n + ag) % guard.GRANULE == 0 and ag == 0)
    report = {
        "kernels": len(counts0), "allocation_full": len(full), "padded": len(padded),
        "padded_free_below_64": sum(1 for n, r in padded.values() if r == "free"),
        "hits_in_unpadded_object": {"class_a": len(a0), "class_b": len(b0), "kernels": sorted(hits)},
        # kernels at or above 64 registers whose count fills the allocation: a granule more costs a wave per SIMD there
        "at_or_above_64": [{"kernel": k, "vgprs": counts0[k][0], "padded": k in padded,
                            "waves_per_simd": guard.waves_per_simd(counts0[k][0]),
                            "waves_per_simd_if_padded": guard.waves_per_simd(counts0[k][0] + 1)}
                           for k in full if counts0[k][0] >= guard.FREE_BELOW],
        "hits_in_final_object": {"class_a": len(a1), "class_b": len(b1)},
        # kernels that use accumulation registers are not scanned (their last VGPR is an AGPR): reported, so that one appearing is seen
        "kernels_with_agprs": sorted(k for k, (n, ag) in counts0.items() if ag > 0),
    }
    report_name = "vgpr_guard.json" if min_kernels is None else os.path.basename(base) + ".vgpr_guard.json"
    json.dump(report, open(os.path.join(work, report_name), "w"), indent=1)
    if a1 or b1:
        raise TilerSliderLibraryError(f"VGPR hazard guard: the padded code object still has {len(a1)} class A / {len(b1)} class B "
                                      f"reads of a last allocated VGPR: {(a1 + b1)[:3]}")
    parsed = bool(full) if min_kernels is None else len(counts0) >= min_kernels and all(n > 0 for n, _ in counts0.values())
    if not parsed:
        raise TilerSliderLibraryError("VGPR hazard guard: no kernel metadata was parsed from the device assembly")
    _run([f"{_LLVM_BIN}/clang-offload-bundler", "-type=o", "-bundle-align=4096",
          "-targets=host-x86_64-unknown-linux-gnu,hipv4-amdgcn-amd-amdhsa--gfx950", "-input=/dev/null", f"-input={hsaco}",
          f"-output={base}.hipfb"], verbose)
    tmp = out_lib + ".tmp"
    _run([hipcc, *common, "--cuda-host-only", "-Xclang", "-fcuda-include-gpubinary", "-Xclang", base + ".hipfb", "-shared", "-fPIC",
          "-o", tmp, src], verbose)
    os.replace(tmp, out_lib)
    for ext in (".raw.s", ".raw.o", ".raw.hsaco", ".o", ".hsaco", ".hipfb") + (() if keep_asm else (".s",)):
        if os.path.exists(base + ext):
            os.remove(base + ext)
    if verbose:
        print(f"VGPR guard: {report['padded']} of {report['allocation_full']} full allocations padded "
              f"({report['padded_free_below_64']} at no cost in waves per SIMD, {len(hits)} on a scanner hit); "
              f"{sum(1 for e in report['at_or_above_64'] if not e['padded'])} at or above 64 left alone (no 64-bit read of the last register)")
    return report


def bind(module, declare):
    """(build_library, lib, check) of a binding module - this one or any other of _libraries.LIBRARIES.  The module keeps SRC,
    HEADERS, LIB_PATH, EXPORTS, ABI_VERSION, MIN_KERNELS and _lib as its own attributes, read when a function is called, and
    beside them HEADER (its public header's file name), PREFIX (of its <prefix>abi_version and <prefix>last_hip_error symbols)
    and LABEL (the library's name in the ABI-mismatch message); declare(L): the prototypes of its entry points."""
    m = sys.modules[module]
    label, prefix = m.LABEL, m.PREFIX

    def build_library(force=False, verbose=False):
        """Compile the library for gfx950 in-tree (hipcc cross-compiles without a GPU), through compile_guarded, if it is older
        than its source or a header it includes."""
        stale = not os.path.exists(m.LIB_PATH) or any(os.path.getmtime(p) > os.path.getmtime(m.LIB_PATH) for p in [m.SRC] + m.HEADERS)
        if force or stale:
            compile_guarded(m.SRC, m.LIB_PATH, verbose=verbose, keep_asm=os.environ.get("TS_KEEP_ASM") == "1", min_kernels=m.MIN_KERNELS)
        return m.LIB_PATH

    def lib():
        """The loaded shared library; raises (never falls back) when it is unavailable."""
        if m._lib is not None:
            return m._lib
        if not os.path.exists(m.LIB_PATH):
            raise TilerSliderLibraryError(
                f"{m.LIB_PATH} is missing: the HIP extension has not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback.")
        try:
            L = C.CDLL(m.LIB_PATH)
        except OSError as e:
            raise TilerSliderLibraryError(f"cannot load {m.LIB_PATH}: {e}") from e
        missing = [s for s in m.EXPORTS if not hasattr(L, s)]
        if missing:
            raise TilerSliderLibraryError(f"{m.LIB_PATH} lacks symbols {missing}; rebuild it")
        version, last_error = getattr(L, prefix + "abi_version"), getattr(L, prefix + "last_hip_error")
        version.restype = last_error.restype = C.c_int32
        declare(L)
        if version() != m.ABI_VERSION:
            raise TilerSliderLibraryError(f"{label}ABI version {version()} != {m.ABI_VERSION}; rebuild the library")
        m._lib = L
        return L

    def check(rc, what):
        if rc != OK:
            msg = _status_string(rc)
            extra = f" (hipError {getattr(lib(), prefix + 'last_hip_error')()})" if rc == ERR_HIP else ""
            raise TilerSliderLibraryError(f"{what}: {msg}{extra}")

    return build_library, lib, check


def _declare(L):
    P, DP, SP = C.c_void_p, C.POINTER(Dims), C.POINTER(State)
    L.ts_limits.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.ts_limits.restype = None
    L.ts_status_string.argtypes = [C.c_int32]
    L.ts_status_string.restype = C.c_char_p
    L.ts_blk_words.argtypes = [C.c_int32]
    L.ts_blk_words.restype = C.c_int32
    L.ts_cell_bytes.argtypes = [C.c_int32]
    L.ts_cell_bytes.restype = C.c_int32
    L.ts_lines_words.argtypes = [C.c_int32]
    L.ts_lines_words.restype = C.c_int32
    L.ts_tuning.argtypes = [C.c_int32, C.c_int64]
    L.ts_tuning.restype = C.c_int64
    L.ts_onehot_channels.argtypes = [DP]
    L.ts_onehot_channels.restype = C.c_int32
    L.ts_check_dims.argtypes = [DP]
    L.ts_check_dims.restype = C.c_int32
    L.ts_describe_launch.argtypes = [DP, C.c_uint32, C.c_uint32, C.POINTER(LaunchDesc)]
    L.ts_describe_launch.restype = C.c_int32
    L.ts_handoff_layout.argtypes = [DP, C.c_int64, C.c_uint32, C.POINTER(C.c_int64 * 4)]
    L.ts_handoff_layout.restype = C.c_int64
    for name, args in (("ts_pack_handoff", [DP, SP, P, P, C.c_int64, C.c_uint32, P, P]),
                       ("ts_unpack_handoff", [DP, C.c_int64, C.c_uint32, C.c_int32, P, P, C.c_int64, P, P, P, P, P]),
                       ("ts_reset", [DP, SP, P, P]),
                       ("ts_step", [DP, SP, P, C.c_uint32, C.POINTER(StepOut), P]),
                       ("ts_valid_moves", [DP, SP, P, P]), ("ts_valid_moves4", [DP, SP, P, P]), ("ts_is_won", [DP, SP, P, P]), ("ts_prepare", [DP, SP, P, P]),
                       ("ts_encode", [DP, SP, P, P]), ("ts_encode_u8", [DP, SP, P, P]),
                       ("ts_encode_onehot", [DP, SP, P, P]), ("ts_reward", [DP, SP, P, P]),
                       ("ts_generate", [DP, SP, C.c_uint64, C.c_int64, C.c_int32, P]),
                       ("ts_generate_mt19937", [DP, SP, P, C.c_int32, P]),
                       ("ts_fill_actions", [C.c_int64, C.c_uint64, C.c_int64, C.c_int64, P, P]),
                       ("ts_expand_u8", [P, P, C.c_int64, P])):
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int32


_lib = None
build_library, lib, check = bind(__name__, _declare)


def _status_string(rc):
    """The text of a status code: the codes of every library are the step library's."""
    return lib().ts_status_string(rc).decode()


def limits():
    a, b = C.c_int32(), C.c_int32()
    lib().ts_limits(C.byref(a), C.byref(b))
    return a.value, b.value
