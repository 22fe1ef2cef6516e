#!/usr/bin/env python3
"""Compare two `hipcc -S` device listings of one translation unit kernel by kernel (e.g. the parent commit's and this one's):
     python tools/isa_same.py parent.s this.s [--changed NAME ...]
A kernel is `same` when its instruction stream is identical after comments, .loc / .file / .cfi lines and the numbers of .LBB / .Ltmp
labels are stripped.  For a kernel that differs, the per-opcode counts of its floating-point instructions (v_*_f32, v_pk_*_f32,
v_fma* / v_fmac*, v_exp / v_log / v_rcp / v_sqrt; the _e32 / _e64 encoding suffix ignored) are compared as well: `fp equal` means
the arithmetic is the same and only its schedule or register allocation moved.
--changed NAME: the kernels (substring of the demangled name) that are ALLOWED to differ or to be new.  Exit status 1 when any other kernel
differs, appears or disappears, or when an allowed kernel's floating-point counts differ."""
import re
import subprocess
import sys
from collections import Counter


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        s = line.split(";")[0].strip()
        if name is None:
            m = re.match(r"^(_Z\w+):$", s)
            if m:
                name, body = m.group(1), []
            continue
        if s.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        if not s or s.startswith((".loc", ".file", ".cfi")):
            continue
        body.append(re.sub(r"\.(LBB|Ltmp)[0-9_]+", r".\1", s))
    return out


def fp_counts(body):
    c = Counter()
    for s in body:
        op = re.sub(r"_e(32|64)\b", "", s.split()[0])
        if op.startswith("v_") and ("_f32" in op or op.startswith(("v_fma", "v_exp", "v_log", "v_rcp", "v_sqrt"))):
            c[op] += 1
    return c


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {n: re.sub(r"\(.*\)$", "", d).replace("void cfnerf::", "") for n, d in zip(names, r)}


def main():
    args = sys.argv[1:]
    allowed = []
    while "--changed" in args:
        i = args.index("--changed")
        allowed.append(args[i + 1])
        del args[i:i + 2]
    a, b = kernels(args[0]), kernels(args[1])
    names = sorted(set(a) | set(b))
    dem = demangle(names)
    bad = same = 0
    for n in names:
        ok = any(x in dem[n] for x in allowed)
        if n not in a or n not in b:
            print(f"{'only in ' + (args[0] if n in a else args[1]):28s} {dem[n]}")
            bad += 0 if (ok and n in b) else 1          # (a NEW kernel named by --changed is expected)
        elif a[n] == b[n]:
            same += 1
        else:
            fa, fb = fp_counts(a[n]), fp_counts(b[n])
            diff = {op: (fa[op], fb[op]) for op in sorted(set(fa) | set(fb)) if fa[op] != fb[op]}
            print(f"{'differs' if ok else 'DIFFERS (not allowed)':28s} {dem[n]}: {len(a[n])} -> {len(b[n])} instructions, "
                  f"fp {'equal (%d)' % sum(fa.values()) if not diff else 'DIFFERENT ' + str(diff)}")
            if not ok or diff:
                bad += 1
    print(f"{same} of {len(names)} kernels identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
