"""What tests/test_libraries_cpu.py checks for every entry of tiler_slider_amd._libraries.LIBRARIES, for every entry of LATER - the
libraries added since that file pinned the table at its twelve names: header, exports and ABI version agree, no symbol is shared
with any other library, the shipped code object passes the gfx950 hazard scan, the build goes through the guard, the binding lists
every header its source reaches - and __graft_entry__.build() builds them after the twelve and the oracle, on lines of their own."""
import itertools
import os
import re
import types

import pytest

from cabi_harness import _assert_build_goes_through_the_guard, _declared, _exported, _kernel_metadata, _scan_last_vgpr
from conftest import ROOT
from tiler_slider_amd import _cabi, _libraries
from tiler_slider_amd._libraries import LATER, LIBRARIES

# the ABI version every later library is pinned at, in the order the libraries were added
PINNED_ABI = {"ptable": 1}
NAMES = [_libraries.name(b) for b in LATER]
every_later_library = pytest.mark.parametrize("binding", LATER, ids=NAMES)


def test_the_table_still_has_its_twelve_names_and_the_later_ones_follow():
    assert [_libraries.name(b) for b in LIBRARIES] == ["step", "search", "table", "rollout", "policy", "train", "targets", "ac", "update",
                                                       "loss", "optim", "starts"]
    assert NAMES == list(PINNED_ABI) and not set(LATER) & set(LIBRARIES)
    every = LIBRARIES + LATER
    assert len({b.LIB_PATH for b in every}) == len({b.SRC for b in every}) == len({b.PREFIX for b in every}) == len(every)


@every_later_library
def test_header_exports_and_abi_version_agree(binding):
    assert _exported(binding.LIB_PATH) == _declared(binding.HEADER) == sorted(binding.EXPORTS)
    assert os.path.join(ROOT, "include", binding.HEADER) in binding.HEADERS
    assert {binding.PREFIX + "abi_version", binding.PREFIX + "last_hip_error"} <= set(binding.EXPORTS)
    header = open(os.path.join(ROOT, "include", binding.HEADER)).read()
    defined = int(re.search(rf"#define {binding.PREFIX.upper()}ABI_VERSION (\d+)", header).group(1))
    assert getattr(binding.lib(), binding.PREFIX + "abi_version")() == binding.ABI_VERSION == defined == PINNED_ABI[_libraries.name(binding)]


def test_no_later_library_exports_a_symbol_of_any_other():
    for a, b in itertools.combinations(LIBRARIES + LATER, 2):
        if a in LATER or b in LATER:
            assert not set(a.EXPORTS) & set(b.EXPORTS), (a.__name__, b.__name__)
            assert not set(_exported(a.LIB_PATH)) & set(_exported(b.LIB_PATH)), (a.__name__, b.__name__)


@every_later_library
def test_no_64bit_read_of_the_last_allocated_vgpr(binding):
    class_a, class_b, n_kernels = _scan_last_vgpr(binding.LIB_PATH)
    assert n_kernels == len(_kernel_metadata(binding.LIB_PATH)) >= binding.MIN_KERNELS
    assert class_a == [] and class_b == []


@every_later_library
def test_the_build_goes_through_the_guard(binding, monkeypatch):
    _assert_build_goes_through_the_guard(binding, monkeypatch)


@every_later_library
def test_the_binding_lists_the_headers_its_source_includes(binding):
    """The walk of tests/test_cabi_and_host_logic.py: every quoted #include of SRC, followed through the headers it reaches, is in
    [SRC] + HEADERS - for the policy tables that includes ts_mlp.h, the network they share with the policy library."""
    csrc = os.path.dirname(os.path.realpath(_cabi.SRC))
    listed = {os.path.realpath(p) for p in [binding.SRC] + binding.HEADERS}
    seen, todo = set(), [os.path.realpath(binding.SRC)]
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M):
            todo.append(os.path.realpath(os.path.join(os.path.dirname(path), inc)))
    assert seen <= listed, (binding.__name__, sorted(seen - listed))
    assert {os.path.join(csrc, h) for h in ("ts_core.h", "ts_index.h", "ts_launch.h")} <= seen
    if _libraries.name(binding) == "ptable":
        assert os.path.join(csrc, "ts_mlp.h") in seen and os.path.join(ROOT, "include", "tiler_slider_policy.h") in seen


def test_build_builds_the_later_libraries_after_the_twelve_and_the_oracle(monkeypatch, capsys):
    """__graft_entry__.build() with every build_library and the oracle's build replaced by recorders."""
    import __graft_entry__ as entry
    from oracle import binding as oracle_binding
    fake = types.SimpleNamespace(__name__="tiler_slider_amd._fake_cabi", PREFIX="ts_fake_", ABI_VERSION=7, LIB_PATH="/nowhere/libtiler_slider_fake.so",
                                 lib=lambda: types.SimpleNamespace(ts_fake_abi_version=lambda: 7))
    later = LATER + (fake,)
    monkeypatch.setattr(_libraries, "LATER", later)
    events = []
    for binding in LIBRARIES + later:
        monkeypatch.setattr(binding, "build_library", lambda force=False, verbose=False, b=binding: events.append((b, force)), raising=False)
    monkeypatch.setattr(oracle_binding, "build", lambda *a, **kw: events.append(("oracle", a, kw)))
    monkeypatch.delenv("TS_FORCE_REBUILD", raising=False)
    entry.build()
    assert events == [(b, False) for b in LIBRARIES] + [("oracle", (), {})] + [(b, False) for b in later]
    lines = capsys.readouterr().out.splitlines()
    assert [l for l in lines if l.startswith("later: built ")] == [f"later: built {b.LIB_PATH} (abi {b.ABI_VERSION})" for b in later]
    assert len([l for l in lines if l.startswith("built ")]) == len(LIBRARIES)
    assert lines.index(f"later: built {later[0].LIB_PATH} (abi {later[0].ABI_VERSION})") > max(i for i, l in enumerate(lines) if l.startswith("built "))


def test_smoke_runs_a_smoke_function_of_every_later_library():
    import inspect
    import __graft_entry__ as entry
    body = inspect.getsource(entry.smoke)
    for name in NAMES:
        assert inspect.isfunction(getattr(entry, f"_smoke_{name}")) and f"_smoke_{name}(" in body, name
