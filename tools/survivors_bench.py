"""Time the exact-candidates pass (irs_topk_ensure_survivors, irs_bind_survivor_scratch).

    python tools/survivors_bench.py [--batch 4096] [--steps 20] [--rounds 5] [--catalog 1000000,128] [--starved 1,64]
                                    [--reps 20] [--out F]

1. loop: irs_generate_paths at the C2 shape (n_item 3415, d 128, L 200, 6 layers; --batch users, --steps steps, random
   windows and targets, so no row is starved) with the survivor scratch unbound and bound, in ONE process on one engine: the
   two alternate over --rounds rounds (a warm-up call of each first), every round is reported, the medians are the figures.
   ms per step = host clock around a call that ends in a device synchronise, divided by the steps.  The difference is the
   price of the flag pass (a 4-byte memset, the flag kernel and two launches that return at once).  `rescued` counts the
   users with IRS_ROW_RESCUED in the bound runs (0 on these inputs) and the paths of the two are compared.
2. pass: one call of irs_topk_ensure_survivors on lists of irs_score_topk (k = 100, want = 1) at the --catalog shape
   (items, d), with the windows of the first s rows holding those rows' 100 candidates (s in --starved; the other rows have
   an empty window) -- ms per call as the median of --reps calls timed by events, lists restored between calls.
One JSON line per row."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from influentialrs_amd import synth  # noqa: E402
from influentialrs_amd._lib import IRS_MASK_IRN, IRS_ROW_RESCUED, IRS_SWEEP_BF16  # noqa: E402
from influentialrs_amd.engine import Engine  # noqa: E402

DEV = "cuda:0"


def _engine(cfg, sd, rows, seqs, max_k=100):
    eng = Engine(n_item=cfg.n_item, n_user=cfg.n_user, d=cfg.emb_dim, max_len=cfg.max_len, n_heads=cfg.n_heads,
                 ffn_dim=cfg.ffn_dim, n_layers=cfg.n_layers, u_dim=cfg.u_emb_dim, mask_mode=IRS_MASK_IRN, device=torch.device(DEV),
                 max_rows=rows, max_seqs=seqs, max_k=max_k)
    eng.bind_state_dict({k: (v if torch.is_tensor(v) else torch.from_numpy(v)).to(DEV) for k, v in sd.items()})
    return eng


def run_loop(B, steps, rounds):
    cfg = synth.make_config("c2")
    eng = _engine(cfg, synth.irn_state_dict(cfg, 1234), B, B)
    seq0 = torch.from_numpy(synth.random_windows(B, cfg.max_len, cfg.n_item, seed=5)).to(DEV)
    users = (torch.arange(B, device=DEV) % cfg.n_user).to(torch.int64)
    hep0 = torch.full((B,), cfg.max_len - 2, dtype=torch.int32, device=DEV)
    paths = torch.zeros((B, steps), dtype=torch.float32, device=DEV)
    status = torch.zeros(B, dtype=torch.int32, device=DEV)
    seq, hep = seq0.clone(), hep0.clone()

    def call(bound):
        seq.copy_(seq0)
        hep.copy_(hep0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.generate_paths(seq, users, hep, steps, k=100, sweep=IRS_SWEEP_BF16, paths=paths, status=status, exact_candidates=bound)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    ms = {False: [], True: []}
    out = {}
    for bound in (False, True):
        call(bound)
        out[bound] = paths.clone()
    rescued = int((status & IRS_ROW_RESCUED).ne(0).sum().item())
    for _ in range(rounds):
        for bound in (False, True):
            ms[bound].append(call(bound))
    med = {b: sorted(v)[len(v) // 2] for b, v in ms.items()}
    return dict(bench="generate_paths", config="c2", B=B, steps=steps, k=100, rounds_ms_unbound=[round(v, 4) for v in ms[False]],
                rounds_ms_bound=[round(v, 4) for v in ms[True]], ms_per_step_unbound=round(med[False], 4),
                ms_per_step_bound=round(med[True], 4), flag_pass_ms_per_step=round(med[True] - med[False], 4), rescued=rescued,
                same_paths=bool(torch.equal(out[False], out[True])), device=torch.cuda.get_device_name(0))


def run_pass(n_item, d, starved, reps, M=64, k=100, L=200):
    nh = d // 32 if d % 32 == 0 else 1
    cfg = synth.make_config("tiny", n_item=n_item, emb_dim=d, n_heads=nh, n_layers=1, max_len=L, ffn_dim=8, n_user=2)
    g = torch.Generator(device=DEV)
    g.manual_seed(n_item + d)
    sd = dict(synth.irn_state_dict(cfg, seed=1))
    sd["item_embedder.weight"] = torch.zeros((n_item + 1, d))  # (not used by the pass: spare the host the random table)
    sd["project.weight"] = (torch.rand((n_item, d), generator=g, device=DEV) * 2 - 1) * d ** -0.5
    sd["project.bias"] = torch.randn((n_item,), generator=g, device=DEV) * 0.1
    eng = _engine(cfg, sd, M, 1)
    x = torch.randn((M, d), generator=g, device=DEV)
    val0, ids0, _ = eng.score_topk(x, k, IRS_SWEEP_BF16)
    scratch = torch.empty(eng.survivor_scratch_bytes(M, 1), dtype=torch.uint8, device=DEV)
    rows = []
    for s in starved:
        seq = torch.zeros((M, L), dtype=torch.int64, device=DEV)
        hep = torch.full((M,), -1, dtype=torch.int32, device=DEV)
        seq[:s, :k] = ids0[:s] + 1
        hep[:s] = k - 1
        val, ids = val0.clone(), ids0.clone()
        status = torch.zeros(M, dtype=torch.int32, device=DEV)
        times = []
        for i in range(reps + 3):
            val.copy_(val0)
            ids.copy_(ids0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.ensure_survivors(x, seq, hep, val, ids, status, want=1, scratch=scratch)
            b.record()
            torch.cuda.synchronize()
            if i >= 3:
                times.append(a.elapsed_time(b))
        n = int((status & IRS_ROW_RESCUED).ne(0).sum().item())
        rows.append(dict(bench="ensure_survivors", n_item=n_item, d=d, M=M, k=k, want=1, starved=s, rescued=n,
                         ms_per_call=round(float(np.median(times)), 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4),
                         reps=reps, scratch_mib=round(scratch.numel() / 2 ** 20, 2), device=torch.cuda.get_device_name(0)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--catalog", default="1000000,128", help="items,d of the pass timing ('' skips it)")
    ap.add_argument("--starved", default="1,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    if not a.no_loop:
        rows.append(run_loop(a.batch, a.steps, a.rounds))
        print(json.dumps(rows[-1]), flush=True)
    if a.catalog:
        n_item, d = (int(v) for v in a.catalog.split(","))
        for r in run_pass(n_item, d, [int(v) for v in a.starved.split(",")], a.reps):
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
