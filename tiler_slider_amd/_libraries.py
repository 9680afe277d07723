"""The C-ABI libraries of the package, in the order they were added: the one place that lists them.

Every feature is a shared library of its own - its own .hip source, public header, binding module and lib/libtiler_slider_*.so -
and stays one: a code object that is never recompiled with new neighbours keeps every kernel of every earlier feature byte for
byte what was tested and measured (section 23 says what a binding module defines and how one is added).
An entry is the binding module itself, so nothing a binding knows is restated here; __graft_entry__.build() and the CPU tests
iterate over this tuple.
"""
from . import (_ac_cabi, _cabi, _lookahead_cabi, _loss_cabi, _mixed_cabi, _optim_cabi, _policy_cabi, _ptable_cabi, _reach_cabi, _rexpert_cabi, _rollout_cabi,
               _rptable_cabi, _rstarts_cabi, _rtable_cabi, _search_cabi, _starts_cabi, _table_cabi, _targets_cabi, _train_cabi, _update_cabi,
               _vtrace_cabi)

LIBRARIES = (_cabi, _search_cabi, _table_cabi, _rollout_cabi, _policy_cabi, _train_cabi, _targets_cabi, _ac_cabi, _update_cabi,
             _loss_cabi, _optim_cabi, _starts_cabi)
# Libraries added since tests/test_libraries_cpu.py and tests/test_cabi_and_host_logic.py pinned LIBRARIES at its twelve names:
# the same kind of entry, built and checked the same way (build_later, tests/test_libraries_later_cpu.py), and reported by
# __graft_entry__.build() on lines of their own.  Whoever next touches those two tests folds this tuple into LIBRARIES
# (DESIGN.md section 23).
LATER = (_ptable_cabi,)
# tests/test_libraries_later_cpu.py pins LATER at its one name and the lines build() prints for it, so LATER is frozen as well.
# The three libraries after that are the entries here: built by build_added after build_later, reported on lines that begin
# "added: built", checked by tests/test_libraries_added_cpu.py, which iterates over this tuple and pins no list of names.
ADDED = (_reach_cabi, _rtable_cabi, _rexpert_cabi)
# tests/test_rexpert_cpu.py pins ADDED at its three names, so ADDED is frozen too, whatever this comment once hoped.  Every
# library since then is an entry here: built by build_since after build_added, reported on lines that begin "since: built",
# checked by tests/test_libraries_since_cpu.py, which iterates over this tuple.  No test pins its length, and none may: a
# library's own tests check that it is an entry, never how many there are - the next library is one more entry (DESIGN.md
# section 23).  tests/test_rptable_cpu.py does assert that the reach policy tables are the LAST entry, so a new library goes in
# front of _rptable_cabi: the order inside this tuple is the order of build() and nothing else.
SINCE = (_rstarts_cabi, _lookahead_cabi, _mixed_cabi, _vtrace_cabi, _rptable_cabi)


def name(binding):
    """step, search, table, ...: _cabi is the step library's binding, _<name>_cabi every other's."""
    return binding.__name__.rsplit(".", 1)[-1][1:-len("_cabi")] or "step"


def build_all(force=False, verbose=False):
    """build_library() of every entry, in order: each compiles only if it is stale (or `force`)."""
    return [binding.build_library(force=force, verbose=verbose) for binding in LIBRARIES]


def build_later(force=False, verbose=False):
    """build_all() for the entries of LATER."""
    return [binding.build_library(force=force, verbose=verbose) for binding in LATER]


def build_added(force=False, verbose=False):
    """build_all() for the entries of ADDED."""
    return [binding.build_library(force=force, verbose=verbose) for binding in ADDED]


def build_since(force=False, verbose=False):
    """build_all() for the entries of SINCE."""
    return [binding.build_library(force=force, verbose=verbose) for binding in SINCE]
