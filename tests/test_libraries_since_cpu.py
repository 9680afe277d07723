"""What tests/test_libraries_added_cpu.py checks for the entries of ADDED, for every entry of tiler_slider_amd._libraries.SINCE - the
libraries added since tests/test_rexpert_cpu.py pinned ADDED at its three names: header, exports and ABI version agree, no symbol
is shared with any other library, the shipped code object passes the gfx950 hazard scan, the build goes through the guard, the
binding lists every header its source reaches, __graft_entry__.build() builds them last on lines of their own, and smoke() runs
a _smoke_<name> of each.

This file pins NEITHER names NOR a length: it iterates over SINCE, and each library's ABI number is pinned in its own
tests/test_<name>_cpu.py.  The next library is one more entry of SINCE and one more such file."""
import inspect
import itertools
import os
import re
import types

import pytest

from cabi_harness import _assert_build_goes_through_the_guard, _declared, _exported, _kernel_metadata, _scan_last_vgpr
from conftest import ROOT
from tiler_slider_amd import _cabi, _libraries
from tiler_slider_amd._libraries import ADDED, LATER, LIBRARIES, SINCE

EARLIER = LIBRARIES + LATER + ADDED
NAMES = [_libraries.name(b) for b in SINCE]
every_library_since = pytest.mark.parametrize("binding", SINCE, ids=NAMES)


def test_the_libraries_since_follow_the_frozen_tuples():
    assert SINCE and len(set(NAMES)) == len(NAMES)
    assert not set(SINCE) & set(EARLIER)
    every = EARLIER + SINCE
    assert len({b.LIB_PATH for b in every}) == len({b.SRC for b in every}) == len({b.PREFIX for b in every}) == len(every)
    for name in NAMES:   # the file that pins the library's ABI number
        assert os.path.exists(os.path.join(ROOT, "tests", f"test_{name}_cpu.py")), name
    assert callable(_libraries.build_since)


@every_library_since
def test_header_exports_and_abi_version_agree(binding):
    assert _exported(binding.LIB_PATH) == _declared(binding.HEADER) == sorted(binding.EXPORTS)
    assert os.path.join(ROOT, "include", binding.HEADER) in binding.HEADERS
    assert {binding.PREFIX + "abi_version", binding.PREFIX + "last_hip_error"} <= set(binding.EXPORTS)
    header = open(os.path.join(ROOT, "include", binding.HEADER)).read()
    defined = int(re.search(rf"#define {binding.PREFIX.upper()}ABI_VERSION (\d+)", header).group(1))
    assert getattr(binding.lib(), binding.PREFIX + "abi_version")() == binding.ABI_VERSION == defined


def test_no_library_since_exports_a_symbol_of_any_other():
    for a, b in itertools.combinations(EARLIER + SINCE, 2):
        if a in SINCE or b in SINCE:
            assert not set(a.EXPORTS) & set(b.EXPORTS), (a.__name__, b.__name__)
            assert not set(_exported(a.LIB_PATH)) & set(_exported(b.LIB_PATH)), (a.__name__, b.__name__)


@every_library_since
def test_no_64bit_read_of_the_last_allocated_vgpr(binding):
    class_a, class_b, n_kernels = _scan_last_vgpr(binding.LIB_PATH)
    assert n_kernels == len(_kernel_metadata(binding.LIB_PATH)) >= binding.MIN_KERNELS
    assert class_a == [] and class_b == []


@every_library_since
def test_the_build_goes_through_the_guard(binding, monkeypatch):
    _assert_build_goes_through_the_guard(binding, monkeypatch)


@every_library_since
def test_the_binding_lists_the_headers_its_source_includes(binding):
    """The walk of tests/test_cabi_and_host_logic.py: every quoted #include of SRC, followed through the headers it reaches, is in
    [SRC] + HEADERS, its own public header among them."""
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
    assert os.path.join(csrc, "ts_core.h") in seen and os.path.join(ROOT, "include", binding.HEADER) in seen


def test_build_builds_the_libraries_since_last_on_lines_of_their_own(monkeypatch, capsys):
    """__graft_entry__.build() with every build_library and the oracle's build replaced by recorders, and one more entry appended
    to SINCE: a new library is one entry."""
    import __graft_entry__ as entry
    from oracle import binding as oracle_binding
    fake = types.SimpleNamespace(__name__="tiler_slider_amd._fake_cabi", PREFIX="ts_fake_", ABI_VERSION=7, LIB_PATH="/nowhere/libtiler_slider_fake.so",
                                 lib=lambda: types.SimpleNamespace(ts_fake_abi_version=lambda: 7))
    since = SINCE + (fake,)
    monkeypatch.setattr(_libraries, "SINCE", since)
    events = []
    for binding in EARLIER + since:
        monkeypatch.setattr(binding, "build_library", lambda force=False, verbose=False, b=binding: events.append((b, force)), raising=False)
    monkeypatch.setattr(oracle_binding, "build", lambda *a, **kw: events.append(("oracle", a, kw)))
    monkeypatch.delenv("TS_FORCE_REBUILD", raising=False)
    entry.build()
    assert events == [(b, False) for b in LIBRARIES] + [("oracle", (), {})] + [(b, False) for b in LATER + ADDED + since]
    lines = capsys.readouterr().out.splitlines()
    mine = [l for l in lines if l.startswith("since: built ")]
    assert mine == [f"since: built {b.LIB_PATH} (abi {b.ABI_VERSION})" for b in since]
    # the counts of the three earlier files: no line of these begins "built ", "later: built " or "added: built "
    assert len([l for l in lines if l.startswith("built ")]) == len(LIBRARIES)
    assert len([l for l in lines if l.startswith("later: built ")]) == len(LATER)
    assert len([l for l in lines if l.startswith("added: built ")]) == len(ADDED)
    assert lines.index(mine[0]) > max(i for i, l in enumerate(lines) if l.startswith("added: built "))
    monkeypatch.setenv("TS_FORCE_REBUILD", "1")
    del events[:]
    entry.build()
    assert events[-len(since):] == [(b, True) for b in since]


def test_smoke_runs_a_smoke_function_of_every_library_since():
    import __graft_entry__ as entry
    body = inspect.getsource(entry.smoke)
    for name in NAMES:
        assert inspect.isfunction(getattr(entry, f"_smoke_{name}")) and f"_smoke_{name}(" in body, name
