"""What the CPU tests of the four C-ABI libraries share: the symbols a header declares and a library exports, a ts_dims,
the kernels of a code object."""
import os
import re
import subprocess

from conftest import ROOT


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ts_[a-z0-9_]+)\s*\(", text)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if re.search(r" T ts_", l))


def _dims(S, T, mc=0, n=8, Tt=None):
    from tiler_slider_amd import _cabi
    return _cabi.Dims(n, S, T, T if Tt is None else Tt, mc, 100, 0)


def _kernel_names(lib_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_recipes_tool", os.path.join(ROOT, "tools", "kernel_recipes.py"))  # (tests/ has a table of that name)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.kernel_names(lib_path)


def _bindings():
    from tiler_slider_amd import _cabi, _rollout_cabi, _search_cabi, _table_cabi
    return _cabi, _search_cabi, _table_cabi, _rollout_cabi


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
