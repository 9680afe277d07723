"""The priority schedule of the in-place step (csrc/ts_update.hip: kLoadsFirst; profiles/update_requests.md, section 7) without a
GPU: what the shipped code object holds of it, followed along the branches of every kernel, and the build-time knobs."""
import os
import re
import subprocess
import tempfile

import pytest

from cabi_harness import _kernel_metadata
from conftest import ROOT

FLAGSHIP = "k_step_update<4, 2, false>"
# The kernels whose waves raise their priority over their loads, and the raised level: kLoadsFirst and kPrioLevel of the source.
# The kernels with a measured row on which the schedule won (profiles/update_requests.md, section 7).
SHIPPED = tuple(f"k_step_update<{S}, 2, {u8}>" for S in (4, 5, 8) for u8 in ("false", "true")) + ("k_step_update<8, 8, false>",)
LEVEL = 1
KNOBS = ("TS_UPDATE_PRIO_OFF", "TS_UPDATE_PRIO_ALL", "TS_UPDATE_PRIO_LEVEL", "TS_UPDATE_PRIO_UNTIL", "TS_UPDATE_PRIO_STORES")
ALL_KERNELS = [f"k_step_update<{S}, {tmax}, {u8}>" for S in range(1, 9) for tmax in (2, 8) for u8 in ("false", "true")]


def disassemble(library):
    """kernel name -> (instructions, labels): mnemonic and operands in address order, branch targets as the disassembler's own
    labels (--symbolize-operands), and label -> index of the instruction it stands in front of."""
    from tiler_slider_amd import _vgpr_guard as guard
    with tempfile.TemporaryDirectory() as wd:
        co = guard.unbundle(library, wd)
        dis = subprocess.run([f"{guard.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--symbolize-operands", "--demangle", co],
                             check=True, capture_output=True, text=True).stdout
    kernels, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m and re.fullmatch(r"L\d+", m.group(1)):
            kernels[name][1][m.group(1)] = len(kernels[name][0])
        elif m:
            name = re.sub(r"^.*(k_step_update<[^>]*>).*$", r"\1", m.group(1))
            kernels[name] = ([], {})
        elif name and line.strip() and not line.strip().startswith("//"):
            kernels[name][0].append(line.split("//")[0].strip())
    return kernels


def priorities(text, labels):
    """The priorities a wave can hold in front of every instruction: s_setprio followed from the entry (priority 0) along the
    fall-through and both ways of every branch."""
    at = [set() for _ in text]
    work = [(0, 0)]
    while work:
        i, prio = work.pop()
        if i >= len(text) or prio in at[i]:
            continue
        at[i].add(prio)
        op, _, arg = text[i].partition(" ")
        assert not re.match(r"s_(setpc|swappc|call|rfe|trap)", op), text[i]
        if op == "s_endpgm":
            continue
        if op == "s_setprio":
            prio = int(arg, 0)
        if op == "s_branch" or op.startswith("s_cbranch_"):
            work.append((labels[arg.strip()], prio))
            if op == "s_branch":
                continue
        work.append((i + 1, prio))
    return at


@pytest.fixture(scope="module")
def shipped_library():
    from tiler_slider_amd import _update_cabi as uc
    kernels = disassemble(uc.LIB_PATH)
    assert sorted(kernels) == sorted(ALL_KERNELS), sorted(set(kernels) ^ set(ALL_KERNELS))
    return kernels


def check_schedule(name, text, labels, level):
    """A kernel with the schedule: one raise a body, every load issued raised, every store and every end at priority 0."""
    at = priorities(text, labels)
    bodies = 2 if ", 2, " in name and not name.startswith("k_step_update<1,") else 1
    raises = [i for i, t in enumerate(text) if t == f"s_setprio {level}"]
    drops = [i for i, t in enumerate(text) if t == "s_setprio 0"]
    assert len(raises) == bodies and len(drops) >= bodies, (name, raises, drops)
    assert len(raises) + len(drops) == sum(1 for t in text if t.startswith("s_setprio")), (name, "another level")
    for i in raises:
        assert at[i] == {0}, (name, i, "a raise on a raised wave")
    for i in drops:
        assert at[i] == {level}, (name, i, "a drop that a wave can reach at priority 0")
    loads = [i for i, t in enumerate(text) if t.startswith("global_load_")]
    stores = [i for i, t in enumerate(text) if t.startswith("global_store_")]
    assert loads and stores
    for i in loads:
        assert at[i] == {level}, (name, i, text[i], "a load outside the raised region")
    for i in stores:
        assert at[i] == {0}, (name, i, text[i], "a store inside the raised region")
    for i, t in enumerate(text):
        if t == "s_endpgm":
            assert at[i] <= {0}, (name, i, "a wave ends raised")


def test_the_walk_sees_a_raise_a_drop_and_what_lies_between():
    """The checker on four hand-written kernels: the schedule as it should be, a store in the raised region, a load behind the
    drop, and a path that goes round the drop."""
    good = ["s_cbranch_scc1 L1", "s_setprio 2", "global_load_dword v1, v1, s[0:1]", "s_cbranch_vccz L0", "global_load_ubyte v2, v2, s[0:1]",
            "s_setprio 0", "global_store_dword v1, v2, s[2:3]", "s_endpgm", "global_load_ubyte v3, v3, s[0:1]", "s_branch L2", "s_endpgm"]
    labels = {"L0": 8, "L2": 5, "L1": 10}  # the second load of the other path lies behind the end, as a compiler lays it out
    check_schedule("k_step_update<1, 2, false>", good, labels, 2)
    for bad, where in ((good[:2] + ["global_store_byte v1, v2, s[2:3]"] + good[2:], {"L0": 9, "L2": 6, "L1": 11}),
                       (good[:6] + ["global_load_ubyte v4, v4, s[0:1]"] + good[6:], {"L0": 9, "L2": 5, "L1": 11}),
                       (good, {"L0": 8, "L2": 6, "L1": 10})):
        with pytest.raises(AssertionError):
            check_schedule("k_step_update<1, 2, false>", bad, where, 2)


def test_the_schedule_is_in_the_kernels_that_ship_it_and_nowhere_else(shipped_library):
    """Every kernel of SHIPPED: each body raises to LEVEL in front of its first load and drops to 0 behind its last - the initial
    cells of a resetting wave among them - with no store in between and no s_setprio elsewhere.  Every other kernel of the 32
    has no s_setprio at all; with nothing shipped that is every kernel."""
    assert set(SHIPPED) <= set(ALL_KERNELS)
    for name in ALL_KERNELS:
        text, labels = shipped_library[name]
        if name in SHIPPED:
            check_schedule(name, text, labels, LEVEL)
        else:
            assert not [t for t in text if t.startswith("s_setprio")], name


def test_the_flagship_keeps_its_loads_its_stores_and_its_registers(shipped_library):
    """k_step_update<4, 2, false>: 24 loads, eight written-through stores, and a VGPR count within 28 .. 64 (eight waves a SIMD)."""
    from tiler_slider_amd import _update_cabi as uc
    text, _ = shipped_library[FLAGSHIP]
    assert sum(1 for t in text if t.startswith("global_load_")) == 24
    assert sum(1 for t in text if t.startswith("global_store_") and t.endswith(" sc1")) == 8
    meta = [k for k in _kernel_metadata(uc.LIB_PATH) if "k_step_updateILi4ELi2ELb0E" in k["name"]]
    assert len(meta) == 1 and 28 <= meta[0]["vgpr_count"] <= 64, meta


def test_the_knobs_are_asked_for_and_never_set():
    """Every knob of the schedule appears as defined(...) in the source and is never #defined there, and tools/update_ab.py and
    tools/update_timeline.py name them; the constant, its level and the three places of the drop are in the source."""
    from tiler_slider_amd import _update_cabi as uc
    src = open(uc.SRC).read()
    tool = open(os.path.join(ROOT, "tools", "update_ab.py")).read()
    for knob in KNOBS:
        assert f"defined({knob})" in src and not re.search(rf"#\s*define\s+{knob}\b", src), knob
        assert knob in tool, knob
    assert "TS_UPDATE_PRIO_OFF" in open(os.path.join(ROOT, "tools", "update_timeline.py")).read()
    assert re.search(r"template <int S, int TMAX, bool U8>\n#if defined\(TS_UPDATE_PRIO_OFF\)\nconstexpr bool kLoadsFirst = false;", src)
    assert f"constexpr int kPrioLevel = {LEVEL};" in src
    assert "enum PrioUntil { kUntil_issued, kUntil_loaded, kUntil_store };" in src
    shipped_rule = re.search(r"#else\nconstexpr bool kLoadsFirst = (.+);\n#endif", src).group(1)
    assert (shipped_rule == "false") == (not SHIPPED), shipped_rule
