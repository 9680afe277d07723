#!/usr/bin/env python3
"""Recipe table of the step kernels: one call per compiled template form that makes the library launch exactly that form.

    python tools/kernel_recipes.py            # search, print the counts, rewrite tests/kernel_recipes.py
    python tools/kernel_recipes.py --check    # search and print only; exit code 1 when the table on disk differs

The gfx950 code object holds one compiled kernel per template form of k_small / k_multi / k_deal / k_lines / k_state, each with
its own register allocation.  This tool lists them (kernel_names: the code object's metadata, demangled), then walks the space
of ts_describe_launch - board size 1 .. 32, tile and target counts (equal, unequal, no targets, more targets than cells), both
colour modes, ts_step / ts_reset / the observation entry points with the output sets the host binds, and the tuning knobs that
select a form (TS_TUNE_NT_THRESHOLD_BYTES, _DEAL, _LINES_LANES, _MULTI_MIN_BOARDS, _STATE_ONLY) - and keeps the first recipe
found for every name: fewest knobs first, the smallest board, tile counts in count_pairs' order, the richest outputs.  An
out-of-cache form counts only where the NT threshold knob selects it (not by the size of a search batch), so that recipes stay
small at any batch size.  The walk stops once every compiled form has a recipe (~10 s); a form it cannot reach is reported after
the whole walk (under a minute): plan_launch never launches it, so it should not be compiled - or it is listed, with the reason,
in the table's hand-kept UNREACHABLE.  tests/test_kernel_instantiations.py checks the table against the built library and runs
every recipe on the GPU.
"""
import ctypes as C
import itertools
import os
import pprint
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, "tests", "kernel_recipes.py")
STEP_FAMILIES = ("k_small", "k_multi", "k_deal", "k_lines", "k_state")

# ts_tuning knobs a recipe may set (name -> value); the search tries each non-default value
KNOB_VALUES = {"NT_THRESHOLD_BYTES": (0,), "MULTI_MIN_BOARDS": (0,), "DEAL": (0,), "LINES_LANES": (4, 8, 16, 32), "STATE_ONLY": (0,)}
# output sets the host binds, richest first: ts_step (VecTilerSliderEnv: flags always; float32, uint8 or no observation; reward,
# one-hot planes and the legality mask in both forms optional), ts_reset (observation or none) and the entry points of one output
STEP_MASKS = ("FLAGS|OBS|REWARD|ONEHOT|VALID|VALID4", "FLAGS|OBS|REWARD|VALID|VALID4", "FLAGS|OBS", "FLAGS|REWARD|VALID|VALID4",
              "FLAGS|VALID|VALID4", "FLAGS", "FLAGS|OBS_U8|REWARD|ONEHOT|VALID|VALID4", "FLAGS|OBS_U8", "FLAGS|ONEHOT")
RESET_MASKS = ("OBS", "")
OBSERVE_MASKS = ("OBS", "OBS_U8", "ONEHOT", "REWARD", "VALID", "VALID4", "FLAGS")
SEARCH_N = 322  # even (k_multi) and small: every launch is cache-resident unless a knob says otherwise


def mask_bits(mask):
    from tiler_slider_amd import _cabi
    bits = 0
    for part in filter(None, mask.split("|")):
        bits |= getattr(_cabi, "OUT_" + part)
    return bits


def kernel_names(lib_path):
    """Every kernel of the library's gfx950 code object, in the ts_launch_desc.name form ("k_small<5, 2, true, true>",
    "k_expand_tail"): the kernel symbols of the metadata note, demangled through the symbol table."""
    from tiler_slider_amd import _vgpr_guard as guard
    with tempfile.TemporaryDirectory() as wd:
        co = guard.unbundle(lib_path, wd)
        notes = subprocess.run([f"{guard.LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        syms = subprocess.run([f"{guard.LLVM}/llvm-readelf", "--symbols", co], check=True, capture_output=True, text=True).stdout
        demangled = subprocess.run([f"{guard.LLVM}/llvm-readelf", "--symbols", "--demangle", co], check=True, capture_output=True,
                                   text=True).stdout
    mangled = [l.split(":", 1)[1].strip() for l in notes.splitlines() if l.strip().startswith(".name:")]
    # the two symbol listings hold the same rows in the same order: column 8 on is the name
    plain, pretty = syms.splitlines(), demangled.splitlines()
    assert len(plain) == len(pretty)
    table = {}
    for a, b in zip(plain, pretty):
        fa, fb = a.split(None, 7), b.split(None, 7)
        if len(fa) == 8 and fa[3] == "FUNC":
            table[fa[7]] = fb[7]
    names = []
    for m in mangled:
        d = table[m]  # "void (anonymous namespace)::k_small<5, 2, true, true>((anonymous namespace)::KArgs)"
        d = re.sub(r"^void ", "", d).replace("(anonymous namespace)::", "")
        depth, end = 0, len(d)
        for i, ch in enumerate(d):
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                end = i
                break
        names.append(d[:end])
    assert len(set(names)) == len(names), "two kernels demangle to one name"
    return sorted(names)


def step_kernel_names(names):
    return sorted(n for n in names if n.split("<")[0] in STEP_FAMILIES and "<" in n)


def knob_settings():
    """Every combination of knob values, fewest non-default knobs first (a stable order)."""
    keys = list(KNOB_VALUES)
    combos = []
    for k in range(len(keys) + 1):
        for chosen in itertools.combinations(keys, k):
            for values in itertools.product(*(KNOB_VALUES[c] for c in chosen)):
                combos.append(dict(zip(chosen, values)))
    return combos


def set_knobs(knobs):
    """Applies `knobs` (name -> value, the others at their defaults); returns the values they replaced."""
    from tiler_slider_amd import _cabi
    L = _cabi.lib()
    return {k: L.ts_tuning(getattr(_cabi, "TUNE_" + k), v) for k, v in knobs.items()}


def tile_counts(C_):
    """Tile counts that reach every form: none, 1 .. 65 (register forms, tiles per lane of k_deal / k_lines), the k_lines
    tiles-per-lane cliffs beyond."""
    return [t for t in list(range(0, 66)) + [100, 128, 129, 200, 255] if t <= C_]


def count_pairs(S):
    """(tiles, targets) of a board size in the order the search tries them.  Targets: as many as tiles, none, one more, eight
    or sixteen more, eight more than the board has cells (targets repeat).  Preferred: boards with tiles that can still move
    (at most 3/4 of the cells) and targets, then the fewest tiles or targets a lane deals with (max(T, Tt)), equal counts, the
    most tiles."""
    C_ = S * S
    pairs = {(T, Tt) for T in tile_counts(C_) for Tt in (T, 0, T + 1, T + 8, T + 16, C_ + 8) if Tt <= 255}
    return sorted(pairs, key=lambda p: (p[0] == 0 or 4 * p[0] > 3 * C_, p[1] == 0, max(p), p[0] != p[1], -p[0]))


def search(wanted, verbose=True):
    """name -> (S, T, Tt, multi_color, op, mask, knobs) for every name of `wanted` that some call reaches (the first found)."""
    from tiler_slider_amd import _cabi
    L = _cabi.lib()
    ops = (("STEP", _cabi.OP_STEP, STEP_MASKS), ("RESET", _cabi.OP_RESET, RESET_MASKS), ("OBSERVE", _cabi.OP_OBSERVE, OBSERVE_MASKS))
    bits = {m: mask_bits(m) for _, _, masks in ops for m in masks}
    desc = _cabi.LaunchDesc()
    found, left = {}, set(wanted)
    for knobs in knob_settings():
        if not left:
            break
        before = set_knobs(knobs)
        try:
            for S in range(1, 33):
                for T, Tt in count_pairs(S):
                    for mc in (False, True):
                        d = _cabi.Dims(SEARCH_N, S, T, Tt, int(mc), 2**30, 0)
                        for op_name, op, masks in ops:
                            for m in masks:
                                if L.ts_describe_launch(C.byref(d), op, bits[m], C.byref(desc)) != _cabi.OK:
                                    continue
                                if desc.out_of_cache and "NT_THRESHOLD_BYTES" not in knobs:
                                    continue  # beyond the cache by its size alone: the knob reaches the form with small outputs
                                name = desc.name.decode()
                                if name and name not in found:
                                    found[name] = (S, T, Tt, mc, op_name, m, dict(knobs))
                                    left.discard(name)
        finally:
            assert set_knobs(before) == knobs
        if verbose:
            print(f"  knobs {knobs or '{}'}: {len(found)} forms found, {len(left)} left", file=sys.stderr)
    return found


def render(recipes, unreachable):
    lines = ['"""Recipe table of the step-kernel instantiations: GENERATED by tools/kernel_recipes.py - rerun it, do not edit by hand.',
             "",
             "name (ts_launch_desc.name, the demangled kernel symbol) -> (S, T, Tt, multi_color, op, outputs, knobs): a batch of S x S",
             "boards with T tiles and Tt targets, the call op (ts_step / ts_reset / an OBSERVE entry point) with the outputs bound",
             "(ts_describe_launch's mask, OUT_* names), and the ts_tuning knobs (TUNE_* names) that select the form.  Each one makes",
             "the library launch exactly that compiled kernel (tests/test_kernel_instantiations.py)."]
    lines += ['"""', "", "RECIPES = {"]
    for name in sorted(recipes):
        lines.append(f"    {name!r}: {recipes[name]!r},")
    lines += ["}", "", "# compiled forms no call reaches -> the reason they stay compiled (kept by hand; the search confirms each)"]
    lines.append("UNREACHABLE = " + pprint.pformat(unreachable))
    return "\n".join(lines) + "\n"


def main():
    import runpy
    from tiler_slider_amd import _cabi
    check = "--check" in sys.argv[1:]
    t0 = time.time()
    names = kernel_names(_cabi.LIB_PATH)
    steps = step_kernel_names(names)
    found = search(steps)
    recipes = {n: found[n] for n in steps if n in found}
    # UNREACHABLE is kept by hand (form -> the reason it stays compiled); the search must confirm that no call reaches it
    listed = runpy.run_path(TABLE).get("UNREACHABLE", {}) if os.path.exists(TABLE) else {}
    unreachable = sorted(set(steps) - set(found))
    by_family = {f: sum(1 for n in steps if n.startswith(f + "<")) for f in STEP_FAMILIES}
    print(f"{len(names)} kernels in the code object: {len(steps)} step-kernel instantiations {by_family}, "
          f"{len(names) - len(steps)} utility kernels")
    print(f"{len(recipes)} with a recipe, {len(unreachable)} unreachable; search {time.time() - t0:.1f} s")
    errors = [f"unreachable and not in UNREACHABLE: {n}" for n in unreachable if n not in listed]
    errors += [f"in UNREACHABLE but reached by {found[n]}: {n}" for n in listed if n in found]
    errors += [f"named by ts_describe_launch but not in the code object: {n}" for n in sorted(set(found) - set(steps))]
    for e in errors:
        print("  " + e)
    text = render(recipes, {n: listed[n] for n in unreachable if n in listed})
    if check:
        same = os.path.exists(TABLE) and open(TABLE).read() == text
        print(f"{TABLE}: {'up to date' if same else 'DIFFERS'}")
        return 0 if same and not errors else 1
    if errors:
        print("table not written: remove unreachable forms from the dispatch tables (or list them in UNREACHABLE with a reason)")
        return 1
    open(TABLE, "w").write(text)
    print(f"wrote {TABLE}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
