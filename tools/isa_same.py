#!/usr/bin/env python3
"""(here, no GPU) Is the device code of two trees the same?  tools/isa_same.py <tree A> <tree B>
Every gel_kernels*.hip of each tree is compiled to device-only assembly with the flags its own Makefile gives the unit (`make -s
print-flags TU=<unit>`; a tree from before that target: the recipe `make -n` prints), the text is cut per function -- from
`.type <sym>,@function` to `.size <sym>`, and a kernel's `.amdhsa_kernel` block -- and compared per symbol, whichever unit holds it
(the ordinal of a function in its unit appears in its local labels: `.LBB<k>_` is rewritten to `.LBB_`, and so on).  Units whose
symbol set is the same on both sides are also compared as whole files.  A text comparison: it knows nothing about particular instructions.
Exit status 0: every function of A exists in B and is identical."""
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile


def compile_line(csrc, unit):
    r = subprocess.run(["make", "-s", "print-flags", "TU=" + unit], cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(["make", "-n", "-B", unit + ".o"], cwd=csrc, capture_output=True, text=True, check=True)
    line = [l for l in r.stdout.split("\n") if " -c " in l][0]
    return line.split(" -c ")[0].split()


def assembly(tree, out):
    """{unit: path of its device-only assembly}"""
    csrc = os.path.join(tree, "gelato_amd", "csrc")
    units = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(csrc, "gel_kernels*.hip")))
    os.makedirs(out)

    def one(u):
        s = os.path.join(out, u + ".s")
        subprocess.run(compile_line(csrc, u) + ["--offload-device-only", "-S", "-o", s, u + ".hip"], cwd=csrc, check=True, capture_output=True)
        return u, s
    with concurrent.futures.ThreadPoolExecutor(os.cpu_count() or 4) as ex:
        return dict(ex.map(one, units))


def normal(text):
    """without what depends on a function's ordinal in its unit or on the unit's path: the ordinal in local labels (and the width of
    the gap it leaves in front of a label's comment), the compilation unit's id"""
    text = re.sub(r"(BB|JTI|CPI)\d+_(?=\d)", r"\1_", text)   # .LBB<k>_<n>, and BB<k>_<n> in the loop comments
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", text)
    return re.sub(r"[ \t]+;", " ;", text)


def functions(path):
    """{symbol: its text} and the set of kernels among them"""
    text = normal(open(path).read())
    fn = {m.group(1): m.group(0) for m in re.finditer(r"^\t\.type\t(\S+),@function\n.*?^\t\.size\t\1,.*?$", text, re.S | re.M)}
    kernels = set()
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel$", text, re.S | re.M):
        fn[m.group(1)] += "\n" + m.group(0)
        kernels.add(m.group(1))
    return fn, kernels


def main(a, b):
    with tempfile.TemporaryDirectory() as tmp:
        sa, sb = assembly(a, os.path.join(tmp, "a")), assembly(b, os.path.join(tmp, "b"))
        fa, fb = {u: functions(p) for u, p in sa.items()}, {u: functions(p) for u, p in sb.items()}
        where_b = {sym: u for u, (fn, _) in fb.items() for sym in fn}
        bad = 0
        print("%-26s %8s %9s %9s %8s  %s" % ("unit of A", "kernels", "identical", "different", "missing", "whole file"))
        for u, (fn, kernels) in sorted(fa.items()):
            same = [s for s in fn if s in where_b and fb[where_b[s]][0][s] == fn[s]]
            missing = [s for s in fn if s not in where_b]
            differ = [s for s in fn if s in where_b and s not in same]
            whole = "-"
            if u in fb and set(fb[u][0]) == set(fn):
                whole = "same" if normal(open(sa[u]).read()) == normal(open(sb[u]).read()) else "DIFFERENT"
            bad += len(missing) + len(differ) + (whole == "DIFFERENT")
            print("%-26s %8d %9d %9d %8d  %s" % (u, len(kernels), len(kernels & set(same)), len(differ), len(missing), whole))
            for s in differ + missing:
                print("    %s %s" % ("differs:" if s in differ else "missing in B:", s))
        extra = sorted(s for s in where_b if not any(s in fn for fn, _ in fa.values()))
        for s in extra:
            print("only in B (%s): %s" % (where_b[s], s))
        print("device code %s" % ("IDENTICAL" if not bad else "DIFFERS"))
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
