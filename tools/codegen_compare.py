#!/usr/bin/env python3
"""Per-kernel code generation of two builds, as the table of profiles/shared_core_codegen.md and profiles/mlp_core_codegen.md.

Build both trees with TS_KEEP_ASM=1 (the padded device assembly stays in build/lib/<library>.gfx950.s), then

    python tools/codegen_compare.py PARENT/build/lib BRANCH/build/lib policy train ac

prints a summary line and one row per kernel, every cell `parent / branch`: VGPRs, SGPRs, scratch and static LDS bytes from the
kernel's metadata, the number of instructions, waves per SIMD (_vgpr_guard.waves_per_simd of the VGPR count), and whether the
instruction text between the kernel's entry and the end of its section is the same once comments are stripped and the
compiler's block labels are numbered in order of appearance.  Plain text comparison: nothing is compiled, loaded or run.
Exit status 0 whatever the outcome; --require-identical makes a difference an error."""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tiler_slider_amd._vgpr_guard import waves_per_simd  # noqa: E402

_LABEL = re.compile(r"\.LBB\d+_\d+")
_META = {"vgprs": ".vgpr_count:", "sgprs": ".sgpr_count:", "scratch": ".private_segment_fixed_size:", "lds": ".group_segment_fixed_size:"}


def kernels_of(path):
    """mangled kernel name -> dict(vgprs, sgprs, scratch, lds, text): metadata and the normalised instruction text."""
    lines = open(path).read().split("\n")
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    out, wanted = {}, set(names)
    i = 0
    while i < len(lines):
        name = lines[i].split(":")[0]
        if name in wanted and lines[i].startswith(name + ":"):
            text, labels = [], {}
            i += 1
            while not lines[i].startswith("\t.section"):
                t = lines[i].split(";")[0].strip()
                if t and not (t.startswith(".") and not t.endswith(":")):  # instructions and labels, no directives
                    text.append(_LABEL.sub(lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), t))
                i += 1
            out[name] = {"text": text, "instructions": sum(1 for t in text if not t.endswith(":"))}
        i += 1
    meta = "\n".join(lines[lines.index("amdhsa.kernels:"):])
    for entry in re.split(r"\n  - ", meta)[1:]:
        fields = {ln.split(":")[0].strip(): ln.split(":", 1)[1].strip() for ln in entry.split("\n") if ":" in ln}
        if ".name" not in fields:  # the entries of amdhsa.version, behind the kernels
            continue
        k = out[fields[".name"]]
        for key, tag in _META.items():
            k[key] = int(fields[tag.rstrip(":")])
    return out


def short_name(mangled):
    """_ZN12_GLOBAL__N_115k_train_forwardILi1EEEvNS_5TArgsE -> k_train_forward<1>: the kernels here are templates over integers in an
    unnamed namespace, which needs no demangler."""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", mangled)
    if not m:
        return mangled
    start = m.end()
    name, rest = mangled[start:start + int(m.group(1))], mangled[start + int(m.group(1)):]
    args = re.match(r"I((?:L[ib]\d+E)+)E", rest)
    return name + ("<" + ", ".join(re.findall(r"L[ib](\d+)E", args.group(1))) + ">" if args else "")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent"), ap.add_argument("branch")
    ap.add_argument("libraries", nargs="+", help="policy -> libtiler_slider_policy.gfx950.s")
    ap.add_argument("--require-identical", action="store_true")
    args = ap.parse_args()
    rows, same, per_lib = [], 0, []
    for lib in args.libraries:
        a, b = (kernels_of(os.path.join(d, f"libtiler_slider_{lib}.gfx950.s")) for d in (args.parent, args.branch))
        if set(a) != set(b):
            sys.exit(f"{lib}: the kernel sets differ: {sorted(set(a) ^ set(b))}")
        pretty = {n: short_name(n) for n in a}
        n_same = 0
        for name in sorted(a, key=lambda n: pretty[n]):
            p, q = a[name], b[name]
            identical = p["text"] == q["text"]
            n_same += identical
            cells = [f"{p[k]} / {q[k]}" for k in ("vgprs", "sgprs", "scratch", "lds", "instructions")]
            cells.append(f"{waves_per_simd(p['vgprs'])} / {waves_per_simd(q['vgprs'])}")
            rows.append(f"| {lib} | `{pretty[name]}` | " + " | ".join(cells) + f" | {'yes' if identical else 'no'} |")
        same += n_same
        per_lib.append(f"{n_same} of {len(a)} {lib}")
    print(f"Summary: {same} of {len(rows)} kernels are identical ({', '.join(per_lib)}).\n")
    print("| library | kernel | VGPRs | SGPRs | scratch | LDS | instructions | waves/SIMD | identical |")
    print("|---|---|---|---|---|---|---|---|---|")
    print("\n".join(rows))
    if args.require_identical and same != len(rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
