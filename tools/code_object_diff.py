#!/usr/bin/env python3
"""Did a change of the sources change the machine code?  Compares the gfx950 kernels of two builds of libdcn_hip.so (or of
two device-only code objects, `hipcc --cuda-device-only --no-gpu-bundle-output -c`), kernel by kernel:

    python tools/code_object_diff.py OLD.so NEW.so [--all] [--limit=N]

Per kernel name it reports whether
  * the resource row is equal (registers, spills, scratch, LDS: tools/kernel_resources.py),
  * the disassembly is equal once addresses and encodings are stripped,
  * the schedule fingerprint is equal: the ordered list of the instructions whose mnemonic starts with one of FINGERPRINT
    (matrix instructions, LDS reads, buffer loads, waits, barriers, priorities), operands included,
and for a kernel whose disassembly differs, how many lines differ per mnemonic (removed / added) and the differing lines
themselves (--limit N: the first N of them per kernel).  Where the fingerprint differs it also says whether it is equal once
register NUMBERS are left out (v12 -> v, s[4:7] -> s[]): the same instructions in the same order on other registers.  Kernels
that are equal in everything are counted, and listed with --all.  A hand tool, like kernel_resources.py."""
import argparse
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr   # noqa: E402

FINGERPRINT = ("v_mfma_", "ds_read", "buffer_load", "s_waitcnt", "s_barrier", "s_setprio")
RESOURCES = [f[1:] for f in kr.FIELDS[1:]]


def disassembly(lib):
    """{kernel name: [instruction text, ...]} over every gfx950 code object of the file (labels kept, addresses not)"""
    out = {}
    with tempfile.TemporaryDirectory() as wd:
        try:
            objs = kr.code_objects(lib, wd)
        except subprocess.CalledProcessError:
            objs = []
        for co in objs or [lib]:   # (no fat binary inside: the file is a code object itself)
            text = subprocess.run([os.path.join(kr.LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True,
                                  text=True, check=True).stdout
            cur = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = out.setdefault(m.group(1), [])
                elif cur is not None and line.strip():
                    cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return out


def resources(lib):
    try:
        return {r["name"]: tuple(r[k] for k in RESOURCES) for r in kr.kernels(lib)}
    except subprocess.CalledProcessError:
        return {}   # (a bare code object: no fat binary to cut the notes out of)


def fingerprint(lines):
    return [l for l in lines if l.startswith(FINGERPRINT)]


def unnumbered(lines):
    return [re.sub(r"\b([vsa])(\[\d+:\d+\]|\d+)\b", lambda m: m.group(1) + ("[]" if "[" in m.group(2) else ""), l) for l in lines]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--all", action="store_true", help="list the identical kernels too")
    ap.add_argument("--limit", type=int, default=None, help="differing lines printed per kernel (default: all)")
    a = ap.parse_args()
    paths, show_all, limit = [a.old, a.new], a.all, a.limit
    old_d, new_d = disassembly(paths[0]), disassembly(paths[1])
    old_r, new_r = resources(paths[0]), resources(paths[1])
    names = sorted(set(old_r) | set(new_r) | set(old_d) | set(new_d))
    dem = dict(zip(names, kr.demangle(names)))
    same = 0
    bad_fp = []
    print("old: %s\nnew: %s\nresources: %s" % (paths[0], paths[1], " ".join(RESOURCES)))
    for n in names:
        if n not in old_d or n not in new_d:
            print("\n%s\n  only in %s" % (dem[n], "old" if n in old_d else "new"))
            bad_fp.append(n)
            continue
        res_eq = old_r.get(n) == new_r.get(n)
        dis_eq = old_d[n] == new_d[n]
        fo, fn = fingerprint(old_d[n]), fingerprint(new_d[n])
        fp_eq = fo == fn
        if res_eq and dis_eq and fp_eq:
            same += 1
            if not show_all:
                continue
        print("\n%s\n  resources %s   disassembly %s (%d instructions)   fingerprint %s (%d instructions)"
              % (dem[n], "equal" if res_eq else "DIFFER", "equal" if dis_eq else "DIFFER", len(new_d[n]),
                 "equal" if fp_eq else "DIFFER", len(fn)))
        if not res_eq:
            print("    old %s\n    new %s" % (old_r.get(n), new_r.get(n)))
        if not fp_eq:
            bad_fp.append(n)
            fl = [l for l in difflib.unified_diff(fo, fn, n=0, lineterm="") if l[0] in "+-" and not l.startswith(("---", "+++"))]
            print("    fingerprint lines that differ (%d); without register numbers the fingerprint is %s:"
                  % (len(fl), "equal" if unnumbered(fo) == unnumbered(fn) else "DIFFERENT"))
            for l in fl[:limit]:
                print("      " + l)
        if not dis_eq:
            lines = [l for l in difflib.unified_diff(old_d[n], new_d[n], "old", "new", n=0, lineterm="")
                     if not l.startswith(("---", "+++"))]
            tally = collections.Counter(l[0] + l[1:].split()[0] for l in lines if l[0] in "+-")
            print("    differing lines per mnemonic (-old / +new): " + ", ".join(
                "%s %d / %d" % (m, tally["-" + m], tally["+" + m]) for m in sorted({k[1:] for k in tally})))
            for l in lines[:limit]:
                print("    " + l)
            if limit is not None and len(lines) > limit:
                print("    ... %d more lines (run without --limit)" % (len(lines) - limit))
    print("\n%d kernels; %d identical in resources, disassembly and fingerprint; %d with a different fingerprint"
          % (len(names), same, len(bad_fp)))
    return 1 if bad_fp else 0


if __name__ == "__main__":
    sys.exit(main())
