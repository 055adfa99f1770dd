#!/usr/bin/env python3
"""Lab: where k_plan_seq (the one-workgroup plan of the sequence-resident decoder launch) spends its time.  Needs a stamped build
of the library (tools/seq_lab.sh plan_stamp -> tools/seqlab_plan_stamp.so: -DIRS_LAB -DPLAN_STAMP, s_memtime of thread 0 at the
kernel's boundaries and of every wave at its end).  usage: IRS_LAB_LIB=tools/seqlab_plan_stamp.so python tools/plan_stamps.py [users=4096]
Layout of the 32 stamps: [0] start, [1] histogram and class starts done, [2] thread 0's counting done (behind its barrier),
[3] pull pass done (behind its barrier), [16 + w] end of wave w.  A library of the range-list form of the kernel (the first version; profiles/step_front_tail/README.md)
fills [3] order table done, [4] end, [5 .. 7] sums over the classes of thread 0's section in front of the placement, the placement
with its two barriers, thread 0's section behind it, [8] classes."""
import ctypes, os, sys
sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np, torch
from influentialrs_amd import _lib
_lib.LIB_PATH = os.path.abspath(os.environ["IRS_LAB_LIB"])
import bench
from influentialrs_amd import synth
from gpu_util import make_engine

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
dev = torch.device("cuda:0")
cfg = synth.make_config("c2")
eng = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=B, max_seqs=B)
lib = ctypes.CDLL(_lib.LIB_PATH)
lib.irs_lab_plan_stamps.restype = ctypes.c_void_p
ptr = lib.irs_lab_plan_stamps()
hip = ctypes.CDLL("libamdhip64.so")
users = torch.randint(0, cfg.n_user, (B,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
pos = torch.full((B,), cfg.max_len - 2, dtype=torch.int32, device=dev)
eng.decoder_seq = True
rows = []
for seed in range(3, 11):  # eight batches of bench windows, the first is the warm-up
    seqs = bench.gpu_windows(B, cfg.max_len, cfg.n_item, dev, seed=seed)
    eng.decode(seqs, users, want_x=False, pos=pos)
    torch.cuda.synchronize()
    buf = torch.empty(32, dtype=torch.int64, device=dev)
    hip.hipMemcpy(ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(32 * 8), ctypes.c_int(3))
    rows.append(buf.cpu().numpy().astype(np.float64))
t = np.stack(rows[1:])  # s_memtime ticks
us = lambda a: "%.0f (%.0f - %.0f)" % (a.mean(), a.min(), a.max())
print("%d users, %d batches; s_memtime ticks, mean (min - max)" % (B, len(t)))
print("  histogram + class starts     ", us(t[:, 1] - t[:, 0]))
print("  thread 0: tail-rule counting ", us(t[:, 2] - t[:, 1]))
if t[:, 4].any():  # the range-list form
    print("  order table                  ", us(t[:, 3] - t[:, 2]))
    print("  class loop                   ", us(t[:, 4] - t[:, 3]), " over %.0f classes" % t[:, 8].mean())
    print("    thread 0 in front of the placements", us(t[:, 5]))
    print("    placements + 2 barriers each       ", us(t[:, 6]))
    print("    thread 0 behind the placements     ", us(t[:, 7]))
    print("  whole kernel (thread 0)      ", us(t[:, 4] - t[:, 0]))
else:
    end = t[:, 16:32]
    print("  pull pass over the classes   ", us(t[:, 3] - t[:, 2]))
    print("  own sequences, slowest wave  ", us(end.max(1) - t[:, 3]))
    print("  whole kernel (slowest wave)  ", us(end.max(1) - t[:, 0]))
