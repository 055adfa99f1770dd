"""Time the C2 search step with and without a bound guide (irs_bind_guide: the Rec2Inf choice rule).

    python tools/guided_bench.py --case unbound|bound [--tree DIR] [--batch 4096] [--steps 20] [--rounds 5] [--out F]

irs_generate_paths at the C2 shape (n_item 3415, d 128, L 200, 6 layers; --batch users, --steps steps, random windows and
targets, k = 100).  ms per step = host clock around a call that ends in a device synchronise, divided by the steps; a warm-up
call first, then --rounds calls, every one reported, the median is the figure.  One process measures ONE side, so that the
sides can alternate as processes:

  --case unbound   nothing bound.  --tree DIR takes the package (and its built library) from another checkout: the parent
                   commit's tree gives the figure this commit's unbound run must not differ from.
  --case bound     two guides, each bound once before its calls (the binding's launch is not in the figures):
                   an 18-bit binary table (ml-1m's genre vectors have 18 bits; random bits here) with k_c = 5, and a float
                   table with F = 128 and k_c = 32 (one lane per survivor, 32 x 512 bytes of table rows per user and step).
                   paths_moved is the share of path entries that differ from the unbound run's.
One JSON line per row."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

DEV = "cuda:0"


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("unbound", "bound"), required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from influentialrs_amd import synth
    from influentialrs_amd._lib import IRS_MASK_IRN, IRS_SWEEP_BF16
    from influentialrs_amd.engine import Engine

    B, steps = a.batch, a.steps
    cfg = synth.make_config("c2")
    eng = Engine(n_item=cfg.n_item, n_user=cfg.n_user, d=cfg.emb_dim, max_len=cfg.max_len, n_heads=cfg.n_heads,
                 ffn_dim=cfg.ffn_dim, n_layers=cfg.n_layers, u_dim=cfg.u_emb_dim, mask_mode=IRS_MASK_IRN, device=torch.device(DEV),
                 max_rows=B, max_seqs=B, max_k=100)
    eng.bind_state_dict({k: torch.from_numpy(v).to(DEV) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    seq0 = torch.from_numpy(synth.random_windows(B, cfg.max_len, cfg.n_item, seed=5)).to(DEV)
    users = (torch.arange(B, device=DEV) % cfg.n_user).to(torch.int64)
    hep0 = torch.full((B,), cfg.max_len - 2, dtype=torch.int32, device=DEV)
    paths = torch.zeros((B, steps), dtype=torch.float32, device=DEV)
    status = torch.zeros(B, dtype=torch.int32, device=DEV)
    seq, hep = seq0.clone(), hep0.clone()

    def call():
        seq.copy_(seq0)
        hep.copy_(hep0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.generate_paths(seq, users, hep, steps, k=100, sweep=IRS_SWEEP_BF16, paths=paths, status=status)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    def timed():
        call()
        ms = [call() for _ in range(a.rounds)]
        return ms, int(paths.to(torch.float64).sum().item())

    base = dict(bench="generate_paths", config="c2", B=B, steps=steps, k=100, label=a.label or a.case,
                device=torch.cuda.get_device_name(0))
    rows = []
    ms, chk = timed()
    unbound = paths.clone()
    rows.append(dict(base, case="unbound", rounds_ms=[round(v, 4) for v in ms], ms_per_step=round(_median(ms), 4), paths_sum=chk))
    if a.case == "bound":
        g = np.random.default_rng(18)
        guides = (("binary F=18 k_c=5", torch.from_numpy(g.integers(0, 2, size=(cfg.n_item + 1, 18)).astype(np.uint8)), 5),
                  ("float F=128 k_c=32", torch.from_numpy(g.standard_normal((cfg.n_item + 1, 128)).astype(np.float32)), 32))
        for name, table, k_c in guides:
            held = eng.bind_guide(table.to(DEV), k_c)
            try:
                ms, chk = timed()
                rows.append(dict(base, case=name, k_c=k_c, F=table.shape[1], rounds_ms=[round(v, 4) for v in ms],
                                 ms_per_step=round(_median(ms), 4), paths_sum=chk,
                                 paths_moved=round(float((paths != unbound).float().mean().item()), 4)))
            finally:
                torch.cuda.synchronize()
                eng.unbind_guide()
            del held
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
