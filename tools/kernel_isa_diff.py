#!/usr/bin/env python3
"""Compare the GPU code of two builds kernel by kernel: the proof that a source refactor left the device code alone.

    python tools/kernel_isa_diff.py --old OLD.s [OLD2.s ...] --new NEW.s [NEW2.s ...] [--rename OLDSYM=NEWSYM ...]

Each side is one or more outputs of `hipcc -S --cuda-device-only` (the Makefile's flags for that translation unit); a side's
files are pooled, so one old file can be compared against the files it was split into.  Per kernel symbol two things are
compared: the instruction lines from the symbol's label to the end of the function (comments dropped; the function index n
of `.LBB<n>_<m>` / `.Lfunc_end<n>` labels, which only counts the functions in front of it in the file, normalised away) and
the `.amdhsa_*` kernel descriptor (registers, LDS, scratch, every enable bit).  One line per kernel: identical, or the first
line that differs.  --rename: a kernel whose symbol changed without its code (one that became a template instantiation) is compared under
its old name.  Exit status 1 if any kernel differs or exists on one side only.  Profiles built this way: profiles/*_isa.md.
"""
import argparse
import re
import sys

_LABEL_INDEX = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI|Ltmp)\d+")


def _code_lines(lines):
    out = []
    for l in lines:
        l = _LABEL_INDEX.sub(r".\1", l.split(";")[0]).strip()
        if l:
            out.append(" ".join(l.split()))
    return out


def kernels(paths):
    """{symbol: (instruction lines, descriptor lines)} of every kernel in the files."""
    found = {}
    for path in paths:
        text = open(path).read()
        for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, flags=re.M | re.S):
            name, desc = m.group(1), _code_lines(m.group(2).splitlines())
            label = re.search(r"^%s:.*$" % re.escape(name), text, flags=re.M)
            if not label:
                sys.exit(f"{path}: kernel {name} has a descriptor but no body")
            end = re.compile(r"^\.Lfunc_end\d+:", flags=re.M).search(text, label.end())
            body = _code_lines(text[label.end():end.start()].splitlines())
            if "s_endpgm" not in body:
                sys.exit(f"{path}: no s_endpgm in the body of {name}")
            if name in found:
                sys.exit(f"{path}: kernel {name} appears twice on one side")
            found[name] = (body, desc)
    return found


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"line {i + 1}: `{x}` -> `{y}`"
    return None if len(a) == len(b) else f"{len(a)} -> {len(b)} lines (one is a prefix of the other)"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--rename", nargs="*", default=[], metavar="OLD=NEW",
                    help="a kernel that became a template instantiation: compare old symbol OLD with new symbol NEW (every "
                         "occurrence of either name inside the code is normalised to OLD)")
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    for pair in args.rename:
        o, n = pair.split("=")
        if n not in new:
            sys.exit(f"--rename: {n} is not a kernel of the new side")
        new[o] = tuple([l.replace(n, o) for l in part] for part in new.pop(n))
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            verdict = "ONLY IN " + ("old" if name in old else "new")
        else:
            d_body = first_difference(old[name][0], new[name][0])
            d_desc = first_difference(old[name][1], new[name][1])
            if d_body or d_desc:
                verdict = "DIFFERS  " + "; ".join(f"{what} {d}" for what, d in (("code", d_body), ("descriptor", d_desc)) if d)
            else:
                desc = dict(l.split(None, 1) for l in new[name][1] if " " in l)
                verdict = "identical  %d instruction lines, next_free_vgpr %s, accum_offset %s, lds %s, scratch %s" % (
                    len(new[name][0]), desc.get(".amdhsa_next_free_vgpr"), desc.get(".amdhsa_accum_offset"),
                    desc.get(".amdhsa_group_segment_fixed_size"), desc.get(".amdhsa_private_segment_fixed_size"))
        bad += not verdict.startswith("identical")
        print(f"{name}: {verdict}")
    print(f"{len(set(old) | set(new))} kernels, {bad} not identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
