#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.

    kernel_diff.py A B [make arguments, e.g. TUNING=1]

A and B are each a directory of device-only assembly (*.s) or a csrc directory with the Makefile;
a csrc directory is compiled first (every compile line of `make -n -B`, turned into
--offload-device-only -S) into <dir>/kdiff[_<args>]/.  Kernels are matched by symbol over all
units: the instruction text and the kernel descriptor must be equal once label numbers are
normalised and comment, .loc and .file lines are dropped.  Exit status 1 on any difference.
"""
import pathlib
import re
import shlex
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

LABEL = re.compile(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end|LJTI)\d+")


def build(csrc, margs):
    out = csrc / ("kdiff" + "".join("_" + re.sub(r"\W", "", a) for a in margs))
    out.mkdir(exist_ok=True)
    plan = subprocess.run(["make", "-C", str(csrc), "-n", "-B", *margs], check=True, capture_output=True, text=True).stdout
    cmds = []
    for line in plan.splitlines():
        w = shlex.split(line)
        if "-c" not in w or not w[w.index("-c") + 1].endswith(".hip"):
            continue
        src = w[w.index("-c") + 1]
        w[w.index("-o") + 1] = str(out / (pathlib.Path(src).name + ".s"))
        w[w.index("-c"):w.index("-c") + 1] = ["--offload-device-only", "-S"]
        cmds.append(w)
    with ThreadPoolExecutor(8) as ex:
        for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), cmds):
            if r.returncode:
                sys.exit(r.stderr)
    return out


def kernels(d):
    """symbol -> (unit, normalised text) of every kernel in the *.s files of d"""
    res, twice = {}, 0
    for f in sorted(d.glob("*.s")):
        text = f.read_text()
        for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
            # from the symbol's label to the end of the function: the code, then the descriptor
            body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(sym), text, re.M | re.S).group(1)
            lines = []
            for ln in body.splitlines():
                ln = LABEL.sub(r".\1", ln.split(";")[0]).strip()
                if ln and not ln.startswith((".loc", ".file")):
                    lines.append(ln)
            if sym in res:
                print("twice in %s: %s (%s, %s)" % (d, sym, res[sym][0], f.name))
                twice += 1
            res[sym] = (f.name, "\n".join(lines))
    return res, twice


def main():
    a, b = (pathlib.Path(p).resolve() for p in sys.argv[1:3])
    (ka, ta), (kb, tb) = (kernels(build(p, sys.argv[3:]) if (p / "Makefile").exists() else p) for p in (a, b))
    bad = ta + tb + (0 if ka and kb else 1)          # a symbol defined twice, or a side without kernels
    for sym in sorted(set(ka) | set(kb)):
        if sym not in ka or sym not in kb:
            print("only in %s: %s (%s)" % (a if sym in ka else b, sym, (ka.get(sym) or kb[sym])[0]))
        elif ka[sym][1] != kb[sym][1]:
            print("differs: %s (%s -> %s)" % (sym, ka[sym][0], kb[sym][0]))
        else:
            continue
        bad += 1
    moved = sum(1 for s in ka if s in kb and ka[s][0] != kb[s][0])
    print("%d kernels in A, %d in B, %d in another unit, %d differ or are unmatched" % (len(ka), len(kb), moved, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
