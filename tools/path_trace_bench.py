"""Time the search step with and without a bound path trace (irs_bind_path_trace).

    python tools/path_trace_bench.py --case unbound|bound [--tree DIR] [--config c2|c3] [--batch 4096] [--steps 20]
                                     [--rounds 5] [--label L] [--out F]

irs_generate_paths at the C2 shape (n_item 3415, d 128, L 200, 6 layers) or the C3 shape (n_item 1,000,000, same decoder);
--batch users, --steps steps, random windows and targets, k = 100.  ms per step = host clock around a call that ends in a device
synchronise, divided by the steps; a warm-up call first, then --rounds calls, every one reported, the median is the figure.  One
process measures ONE side, so that the sides can alternate as processes:

  --case unbound   nothing bound.  --tree DIR takes the package (and its built library) from another checkout: the parent
                   commit's tree gives the figure this commit's unbound run must not differ from.
  --case bound     the trace bound once before the calls (three [batch, steps] arrays and the scratch): every step then runs the
                   target sweep (one more pass over the float32 catalog) and the record kernel.  The row also carries sums of
                   the three arrays, so that two runs can be told to have computed the same thing.
One JSON line per row."""
import argparse
import json
import os
import sys
import time

import torch

DEV = "cuda:0"


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("unbound", "bound"), required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--config", choices=("c2", "c3"), default="c2")
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
    cfg = synth.make_config(a.config)
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
        return [call() for _ in range(a.rounds)]

    row = dict(bench="generate_paths", config=a.config, n_item=cfg.n_item, B=B, steps=steps, k=100, label=a.label or a.case,
               case=a.case, device=torch.cuda.get_device_name(0))
    if a.case == "unbound":
        ms = timed()
    else:
        lp_item, lp_target, rank, scratch = eng.bind_path_trace(B, steps)
        try:
            ms = timed()
            torch.cuda.synchronize()
            row.update(scratch_kib=round(scratch.numel() / 1024, 1), lp_item_sum=float(lp_item.double().sum().item()),
                       lp_target_sum=float(lp_target.double().sum().item()), rank_sum=int(rank.to(torch.int64).sum().item()),
                       rank_min=int(rank.min().item()))
        finally:
            eng.unbind_path_trace()
    row.update(rounds_ms=[round(v, 4) for v in ms], ms_per_step=round(_median(ms), 4),
               paths_sum=int(paths.to(torch.float64).sum().item()))
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
