#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.

    tools/isa_diff.py OLD_DIR NEW_DIR [--removed FILE] [--md OUT.md]

Each directory holds device assembly (.s) emitted with the Makefile's HIPFLAGS
plus `--cuda-device-only -S`, one file per translation unit.  A kernel is a
symbol with an `.amdhsa_kernel` block; its text is everything from its label to
its function-end label, comments stripped and local labels (.LBB0_3,
.Lfunc_end0, ...) renumbered in order of appearance, so that neither the
kernel's position in its file nor the file it lives in matters (a kernel may
move between translation units).  Required: the
same set of kernels on both sides (but for the symbols listed in --removed,
which must be absent from NEW_DIR), identical text, identical
`.amdhsa_kernel ... .end_amdhsa_kernel` block.  Exit status 1 on any difference.
"""
import argparse
import difflib
import glob
import os
import re
import sys

LOCAL = re.compile(r"\.L[A-Za-z_$]*\d+(?:_\d+)?")


def strip(line):
    return line.split(";", 1)[0].rstrip()


def normalise(lines):
    names = {}
    out = []
    for ln in lines:
        ln = strip(ln)
        if not ln.strip():
            continue
        out.append(LOCAL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), ln))
    return out


def kernels(directory):
    """symbol -> (file, text lines, descriptor lines)"""
    found = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        desc = {}
        i = 0
        while i < len(lines):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
            if m:
                j = i
                while ".end_amdhsa_kernel" not in lines[j]:
                    j += 1
                desc[m.group(1)] = [strip(l).strip() for l in lines[i:j + 1]]
                i = j
            i += 1
        label = {ln[:-1]: n for n, ln in enumerate(map(strip, lines)) if ln.endswith(":") and ln[:-1] in desc}
        for sym, d in desc.items():
            start = label[sym]
            end = start
            while not re.match(r"\.Lfunc_end\d+:", lines[end]):
                end += 1
            if sym in found:
                raise SystemExit("%s: kernel %s is also defined in %s" % (path, sym, found[sym][0]))
            found[sym] = (os.path.basename(path), normalise(lines[start:end + 1]), d)
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--removed", help="file of kernel symbols deleted on purpose, one per line")
    ap.add_argument("--md", help="write the result as markdown")
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    removed = set()
    if args.removed:
        removed = {l.strip() for l in open(args.removed) if l.strip() and not l.startswith("#")}
    report = []
    bad = 0
    for sym in sorted(removed):
        if sym not in old or sym in new:
            bad += 1
            report.append("listed as removed but %s: `%s`" % ("still present" if sym in new else "not in the old build", sym))
    for sym in sorted(set(old) - set(new) - removed):
        bad += 1
        report.append("missing from the new build: `%s` (was in %s)" % (sym, old[sym][0]))
    for sym in sorted(set(new) - set(old)):
        bad += 1
        report.append("only in the new build: `%s` (%s)" % (sym, new[sym][0]))
    same = 0
    for sym in sorted(set(old) & set(new)):
        ok = True
        for what, a, b in (("text", old[sym][1], new[sym][1]), ("descriptor", old[sym][2], new[sym][2])):
            if a != b:
                ok = False
                diff = list(difflib.unified_diff(a, b, old[sym][0], new[sym][0], lineterm="", n=1))
                report.append("%s differs: `%s`\n```\n%s\n```" % (what, sym, "\n".join(diff[:60])))
        same += ok
        bad += not ok
    files = {}
    for sym in set(old) & set(new):
        files[new[sym][0]] = files.get(new[sym][0], 0) + 1
    head = ["kernels: %d old, %d new, %d removed on purpose" % (len(old), len(new), len(removed)),
            "identical text and descriptor: %d of %d common kernels" % (same, len(set(old) & set(new))),
            "differences: %d" % bad]
    per_file = ["| %s | %d |" % kv for kv in sorted(files.items())]
    print("\n".join(head + report))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(["# Device code comparison", ""] + ["- " + h for h in head] + ["", "| new file | kernels |", "|---|---|"] +
                              per_file + [""] + (["## Removed on purpose", ""] + ["- `%s`" % s for s in sorted(removed)] + [""] if removed else []) +
                              (["## Differences", ""] + report + [""] if report else [])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
