"""Compare the instruction sequences of the kernels two `hipcc -S` outputs share.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S csrc/score.hip -o new.s   (and the same on the other tree)
    python tools/isa_kernel_diff.py old.s new.s [--match k_sweep_f32]

A kernel is the text between its label and its .Lfunc_end; comments, directives and blank lines are dropped and the function
ordinal inside local labels (.LBB12_3) is masked, since it moves when a kernel is added to the file.  Prints one line per
kernel and a summary; exit status 1 if a shared kernel differs.
"""
import argparse
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        t = line.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.endswith(":")):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--match", default="")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    same = diff = 0
    for k in sorted(old):
        if a.match not in k or k not in new:
            continue
        eq = old[k] == new[k]
        same, diff = same + eq, diff + (not eq)
        print(("same " if eq else "DIFF ") + f"{len(old[k]):6d} {len(new[k]):6d}  {k}")
    added = [k for k in new if a.match in k and k not in old]
    print(f"{same} identical, {diff} different, {len(added)} only in the new file")
    sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()
