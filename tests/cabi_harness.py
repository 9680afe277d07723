"""What the CPU tests of the C-ABI libraries share: the symbols a header declares and a library exports, the fields of a header's
struct, a ts_dims, the kernels of a code object with their metadata and instruction counts, the hazard scan."""
import os
import re
import subprocess
import sys
import tempfile

from conftest import ROOT

# what _kernel_metadata reads of every kernel's note: a kernel that lacks one fails the parse
_METADATA_KEYS = ("vgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "uses_dynamic_stack")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", text)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if re.search(r" T ts_", l))


def _struct_fields(header_text, struct):
    """The field names of `typedef struct <struct> { ... } <struct>;` in declaration order: "float gamma, lam" declares two,
    "void *param[TS_OPTIM_MAX_TENSORS]" and "char name[64]" one each."""
    body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header_text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s*(?:\[\w+\]\s*)*[,;]", body)


def _dims(S, T, mc=0, n=8, Tt=None):
    from tiler_slider_amd import _cabi
    return _cabi.Dims(n, S, T, T if Tt is None else Tt, mc, 100, 0)


def _kernel_names(lib_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_recipes_tool", os.path.join(ROOT, "tools", "kernel_recipes.py"))  # (tests/ has a table of that name)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.kernel_names(lib_path)


def _code_object_text(lib_path, *tool):
    """stdout of an LLVM tool (llvm-readelf --notes, llvm-objdump -d ...) run on the gfx950 code object inside a built library."""
    from tiler_slider_amd import _vgpr_guard as guard
    with tempfile.TemporaryDirectory() as wd:
        return subprocess.run([f"{guard.LLVM}/{tool[0]}", *tool[1:], guard.unbundle(lib_path, wd)], check=True, capture_output=True, text=True).stdout


def _kernel_metadata(lib_path):
    """One record per kernel of the library's code object, each parsed from that kernel's own entry of the metadata note: name
    and _METADATA_KEYS (integers; uses_dynamic_stack a bool).  An entry without a name or without one of the keys raises."""
    notes = _code_object_text(lib_path, "llvm-readelf", "--notes")
    kernels = re.search(r"^amdhsa\.kernels:\s*\n(.*?)(?=^amdhsa\.|\Z)", notes, flags=re.S | re.M).group(1)
    records = []
    for entry in re.split(r"^  - ", kernels, flags=re.M)[1:]:   # the list's own items: nested lists (.args) are indented deeper
        rec = {}
        for key in ("name",) + _METADATA_KEYS:
            found = re.findall(rf"^(?:    )?\.{key}:\s+(\S.*?)\s*$", entry, flags=re.M)
            if len(found) != 1:
                raise ValueError(f"{lib_path}: kernel entry with {len(found)} .{key} lines:\n{entry[:400]}")
            rec[key] = found[0].strip("'\"") if key == "name" else found[0] == "true" if key == "uses_dynamic_stack" else int(found[0])
        records.append(rec)
    return records


def _instruction_counts(lib_path, patterns):
    """kernel symbol -> [lines of its disassembly that match each of `patterns`]."""
    counts, kernel = {}, None
    for line in _code_object_text(lib_path, "llvm-objdump", "-d", "--no-show-raw-insn").splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            kernel = m.group(1)
            counts.setdefault(kernel, [0] * len(patterns))
        elif kernel:
            for i, pat in enumerate(patterns):
                counts[kernel][i] += bool(re.search(pat, line))
    return counts


def _scan_last_vgpr(lib_path):
    """tools/scan_last_vgpr.py's scan of a built library: (class A findings, class B findings, number of kernels parsed)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scan_last_vgpr
    return scan_last_vgpr.scan(lib_path)


def _bindings():
    from tiler_slider_amd._libraries import LIBRARIES
    return LIBRARIES


def _assert_build_goes_through_the_guard(binding, monkeypatch):
    """build_library(force=True) of `binding` is one call of _cabi.compile_guarded with the binding's own source, library and
    kernel count (None for the step library: compile_guarded's default)."""
    from tiler_slider_amd import _cabi
    calls = []
    monkeypatch.setattr(_cabi, "compile_guarded", lambda *a, **kw: calls.append((a, kw)))
    assert binding.build_library(force=True) == binding.LIB_PATH
    assert len(calls) == 1
    (args, kw), = calls
    assert args == (binding.SRC, binding.LIB_PATH) and kw["min_kernels"] == binding.MIN_KERNELS
    assert (binding.MIN_KERNELS is None) == (binding is _cabi)
