#!/usr/bin/env python3
"""List the compiler-written `s_waitcnt vmcnt(N)` of a kernel per barrier-delimited segment of its ISA.

The fused layer kernels wait for their global loads and LDS-DMA pieces by hand-counted waits inside inline asm.  A wait the
COMPILER writes (outside #ASMSTART / #ASMEND) stands in front of a vector memory operation it tracks itself -- a plain load,
a store it must order, a scratch reload -- and, vector memory operations retiring in order, it also waits for everything the
inline asm issued in front of it.  A chain of such waits is a chain of dependent memory round trips: sixteen `vmcnt(0)` in
front of sixteen stores are fifteen store acknowledgements waited for one at a time.  This tool cuts a kernel at its
`s_barrier`s and prints, per segment, the compiler-written vmcnt waits (and how many of them are vmcnt(0)), the
`global_store_dwordx4`, the global loads and the scratch instructions, so that such chains are visible per phase.  An
unconditional branch (or the program's end) cuts a segment too: what the compiler lays out behind it belongs to another path
(the tail of the idle waves' loop stands in front of the live prologue in the sequence-resident kernel).

usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -Iinclude influentialrs_amd/csrc/decoder.hip -o dec.s
       tools/isa_vm_drain_scan.py dec.s <mangled-kernel-name-prefix> [...]"""
import re
import sys



def kernel_lines(lines, prefix):
    """the kernel's whole function, up to its .Lfunc_end (a kernel may hold more than one s_endpgm)"""
    i = next(k for k, l in enumerate(lines) if l.startswith(prefix) and ":" in l.split()[0])
    j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
    return lines[i:j]


def segments(lines):
    """One dict per segment between two s_barrier / unconditional branches (segment 0 = up to the first one): `line` = the segment's first line in
    `lines`, `waits` = the N of every compiler-written s_waitcnt vmcnt(N), `asm_waits` = of those inside inline asm,
    `st128` = global_store_dwordx4, `gld` = global loads into registers, `dma` = LDS-DMA loads, `scratch` = scratch
    instructions."""
    def new(i):
        return {"line": i, "waits": [], "asm_waits": [], "st128": 0, "gld": 0, "dma": 0, "scratch": 0}
    segs, in_asm = [new(0)], False
    for i, l in enumerate(lines):
        t = l.strip()
        if t.startswith(";;#ASMSTART"):
            in_asm = True
        elif t.startswith(";;#ASMEND"):
            in_asm = False
        if not t or t[0] in ";.":
            continue
        op = t.split(None, 1)[0]
        s = segs[-1]
        if op in ("s_barrier", "s_branch", "s_endpgm", "s_setpc_b64"):
            segs.append(new(i + 1))  # (behind an unconditional branch: code of another path, laid out here by the compiler)
        elif op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", t)
            if m:
                s["asm_waits" if in_asm else "waits"].append(int(m.group(1)))
        elif op.startswith("global_store_dwordx4"):
            s["st128"] += 1
        elif op.startswith("global_load_lds"):
            s["dma"] += 1
        elif op.startswith("global_load"):
            s["gld"] += 1
        elif op.startswith("scratch_"):
            s["scratch"] += 1
    return segs


def main():
    lines = open(sys.argv[1]).read().split("\n")
    for prefix in sys.argv[2:]:
        k = kernel_lines(lines, prefix)
        segs = segments(k)
        print(f"{prefix}: {len(k)} lines, {len(segs)} segments, {sum(len(s['waits']) for s in segs)} compiler-written vmcnt waits")
        for n, s in enumerate(segs):
            if s["waits"] or s["st128"]:
                print(f"  segment {n:3d} (line {s['line']:6d}): {len(s['waits']):2d} compiler vmcnt waits ({s['waits'].count(0)} x vmcnt(0)), "
                      f"{len(s['asm_waits'])} in asm, {s['st128']} global_store_dwordx4, {s['gld']} global loads, {s['dma']} DMA, {s['scratch']} scratch")


if __name__ == "__main__":
    main()
