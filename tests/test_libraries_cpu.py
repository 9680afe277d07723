"""What holds for every C-ABI library alike, once, over tiler_slider_amd._libraries.LIBRARIES: header, exports and ABI version
agree, no two libraries share a symbol, the shipped code object passes the gfx950 hazard scan, the build goes through the guard -
and __graft_entry__.build() visits exactly the entries of the table.  What is particular to a library (struct layouts, refusals,
launch plans, its code object's properties) is in its own tests/test_<name>_cpu.py."""
import inspect
import itertools
import os
import re
import types

import pytest

from cabi_harness import _assert_build_goes_through_the_guard, _declared, _exported, _kernel_metadata, _scan_last_vgpr
from conftest import ROOT
from tiler_slider_amd import _cabi, _libraries
from tiler_slider_amd._libraries import LIBRARIES

# the ABI version every library is pinned at, in the order the libraries were added: the one place the numbers are written
PINNED_ABI = {"step": 6, "search": 1, "table": 1, "rollout": 1, "policy": 1, "train": 1, "targets": 1, "ac": 1, "update": 1, "loss": 1,
              "optim": 1, "starts": 1}
NAMES = [_libraries.name(b) for b in LIBRARIES]
every_library = pytest.mark.parametrize("binding", LIBRARIES, ids=NAMES)


def test_the_table_lists_the_libraries_in_the_order_they_were_added():
    assert NAMES == list(PINNED_ABI)
    assert len({b.LIB_PATH for b in LIBRARIES}) == len({b.SRC for b in LIBRARIES}) == len({b.PREFIX for b in LIBRARIES}) == len(LIBRARIES)


@every_library
def test_header_exports_and_abi_version_agree(binding):
    assert _exported(binding.LIB_PATH) == _declared(binding.HEADER) == sorted(binding.EXPORTS)
    assert os.path.join(ROOT, "include", binding.HEADER) in binding.HEADERS
    assert {binding.PREFIX + "abi_version", binding.PREFIX + "last_hip_error"} <= set(binding.EXPORTS)
    header = open(os.path.join(ROOT, "include", binding.HEADER)).read()
    defined = int(re.search(rf"#define {binding.PREFIX.upper()}ABI_VERSION (\d+)", header).group(1))
    assert getattr(binding.lib(), binding.PREFIX + "abi_version")() == binding.ABI_VERSION == defined == PINNED_ABI[_libraries.name(binding)]


def test_no_two_libraries_export_the_same_symbol():
    for a, b in itertools.combinations(LIBRARIES, 2):
        assert not set(a.EXPORTS) & set(b.EXPORTS), (a.__name__, b.__name__)


@every_library
def test_no_64bit_read_of_the_last_allocated_vgpr(binding):
    """gfx950: a 64-bit shift whose shift amount sits in the LAST register of the wave's VGPR allocation occasionally
    reads v0 instead (profiles/r03_wrong_slide_isa.md).  The build scans the unpadded object, pads allocations (always
    below 64 registers, from 64 on only on a scanner hit), scans again and fails on a hit; this re-checks every shipped
    code object instruction by instruction."""
    class_a, class_b, n_kernels = _scan_last_vgpr(binding.LIB_PATH)
    # the metadata was found and parsed: every kernel the code object holds, hundreds of them in the step library
    assert n_kernels == len(_kernel_metadata(binding.LIB_PATH))
    assert n_kernels > 300 if binding is _cabi else n_kernels >= binding.MIN_KERNELS
    assert class_a == [] and class_b == []


@every_library
def test_the_build_goes_through_the_guard(binding, monkeypatch):
    _assert_build_goes_through_the_guard(binding, monkeypatch)


@pytest.mark.parametrize("force", (False, True))
def test_build_visits_every_entry_of_the_table_once_in_order_then_the_oracle(force, monkeypatch, capsys):
    """__graft_entry__.build() with every build_library and the oracle's build replaced by recorders, and a thirteenth entry
    appended to the table: a new library is one entry."""
    import __graft_entry__ as entry
    from oracle import binding as oracle_binding
    fake = types.SimpleNamespace(__name__="tiler_slider_amd._fake_cabi", PREFIX="ts_fake_", ABI_VERSION=7, LIB_PATH="/nowhere/libtiler_slider_fake.so",
                                 lib=lambda: types.SimpleNamespace(ts_fake_abi_version=lambda: 7))
    table = LIBRARIES + (fake,)
    monkeypatch.setattr(_libraries, "LIBRARIES", table)
    events = []
    for binding in table:
        monkeypatch.setattr(binding, "build_library", lambda force=False, verbose=False, b=binding: events.append((b, force)), raising=False)
    monkeypatch.setattr(oracle_binding, "build", lambda *a, **kw: events.append(("oracle", a, kw)))
    if force:
        monkeypatch.setenv("TS_FORCE_REBUILD", "1")
    else:
        monkeypatch.delenv("TS_FORCE_REBUILD", raising=False)
    entry.build()
    assert events == [(b, force) for b in table] + [("oracle", (), {})]
    built = [line for line in capsys.readouterr().out.splitlines() if line.startswith("built ")]
    assert built == [f"built {b.LIB_PATH} (abi {b.ABI_VERSION}{', limits (32, 255)' if b is _cabi else ''})" for b in table]


def test_smoke_runs_a_smoke_function_of_every_feature_library():
    import __graft_entry__ as entry
    body = inspect.getsource(entry.smoke)
    for name in ("policy", "train", "targets", "ac", "update", "loss", "optim", "starts"):
        assert name in NAMES and inspect.isfunction(getattr(entry, f"_smoke_{name}")) and f"_smoke_{name}(" in body, name
