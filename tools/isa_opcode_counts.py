"""Instruction and opcode counts of chosen kernels in a `hipcc -S` output, and their registers from the resource remarks.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
        influentialrs_amd/csrc/decoder.hip -o new.s 2> new.res
    python tools/isa_opcode_counts.py new.s [--res new.res] --kernel k_block_x6ILi3ELi8ELb0ELi4ELi2ELb1E [--kernel ..] \
        [--op v_cvt_f16_f32 --op v_fma_mix ..]

Per kernel: instructions, vector instructions that are no MFMA, MFMAs, barriers, each --op prefix's count, and VGPRs / spilled
VGPRs / scratch bytes.  (Code bytes: llvm-nm --print-size on the device object of `hipcc -c --cuda-device-only`.)
"""
import argparse
import re
import sys

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.abspath(__file__)))
from isa_kernel_diff import kernels  # noqa: E402

OPS = ["v_cvt_f16_f32", "v_cvt_pk_f16_f32", "v_cvt_f32_f16", "v_sub_f32", "v_pk_add_f32", "v_fma_mix", "v_exp_f32", "v_cndmask"]


def resources(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(Function Name|VGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
            out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--res", default=None)
    ap.add_argument("--kernel", action="append", required=True, help="substring of the mangled name")
    ap.add_argument("--op", action="append", default=None, help="opcode prefix to count (default: the plane-split family)")
    a = ap.parse_args()
    ks, res = kernels(a.asm), resources(a.res) if a.res else {}
    for want in a.kernel:
        for name, body in ks.items():
            if want not in name:
                continue
            ins = [t.split()[0] for t in body if not t.endswith(":")]
            vec = [o for o in ins if o.startswith("v_") and not o.startswith("v_mfma")]
            row = {"instructions": len(ins), "vector": len(vec), "mfma": sum(o.startswith("v_mfma") for o in ins),
                   "barriers": ins.count("s_barrier")}
            for p in (a.op or OPS):
                row[p] = sum(o.startswith(p) for o in ins)
            r = res.get(name, {})
            row.update(vgpr=r.get("VGPRs"), spilled=r.get("VGPRs Spill"), scratch=r.get("ScratchSize [bytes/lane]"))
            print(name)
            print("   " + "  ".join(f"{k}={v}" for k, v in row.items()))


if __name__ == "__main__":
    main()
