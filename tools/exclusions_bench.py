"""Time the C2 search step with and without bound exclusions (irs_bind_exclusions).

    python tools/exclusions_bench.py --case unbound|bound [--tree DIR] [--batch 4096] [--steps 20] [--rounds 5] [--out F]

irs_generate_paths at the C2 shape (n_item 3415, d 128, L 200, 6 layers; --batch users, --steps steps, random windows and
targets, k = 100).  ms per step = host clock around a call that ends in a device synchronise, divided by the steps; a warm-up
call first, then --rounds calls, every one reported, the median is the figure.  One process measures ONE side, so that the
sides can alternate as processes:

  --case unbound   nothing bound.  --tree DIR takes the package (and its built library) from another checkout: the parent
                   commit's tree gives the figure this commit's unbound run must not differ from.
  --case bound     per-user lists of ml-1m-shaped histories (synth.user_histories: median 95 ids, at most 2276), bound once
                   before the calls; timed without and with a survivor scratch (exact_candidates), with no_repeat on.  The
                   share of starved users is the share with IRS_ROW_NO_CANDIDATE (no scratch) or IRS_ROW_RESCUED (scratch) in
                   their status word after the 20 steps.
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
    from influentialrs_amd._lib import IRS_MASK_IRN, IRS_ROW_NO_CANDIDATE, IRS_ROW_RESCUED, IRS_SWEEP_BF16
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

    def call(**kw):
        seq.copy_(seq0)
        hep.copy_(hep0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.generate_paths(seq, users, hep, steps, k=100, sweep=IRS_SWEEP_BF16, paths=paths, status=status, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    def timed(**kw):
        call(**kw)
        ms = [call(**kw) for _ in range(a.rounds)]
        return ms, int(paths.to(torch.float64).sum().item())

    base = dict(bench="generate_paths", config="c2", B=B, steps=steps, k=100, label=a.label or a.case,
                device=torch.cuda.get_device_name(0))
    rows = []
    if a.case == "unbound":
        ms, chk = timed()
        rows.append(dict(base, case="unbound", rounds_ms=[round(v, 4) for v in ms], ms_per_step=round(_median(ms), 4), paths_sum=chk))
    else:
        hists = synth.user_histories(B, cfg.n_item, seed=7)
        n_excl = max(len(h) for h in hists)
        excl = np.full((B, n_excl), -1, dtype=np.int64)
        for b, h in enumerate(hists):
            excl[b, :len(h)] = np.asarray(h, dtype=np.int64) - 1
        lens = [len(h) for h in hists]
        scratch = eng.bind_exclusions(torch.from_numpy(excl).to(DEV), no_repeat=True)
        try:
            for exact in (False, True):
                ms, chk = timed(exact_candidates=exact)
                bit = IRS_ROW_RESCUED if exact else IRS_ROW_NO_CANDIDATE
                rows.append(dict(base, case="bound+scratch" if exact else "bound", n_excl=n_excl, list_len_median=int(np.median(lens)),
                                 list_len_max=int(max(lens)), no_repeat=True, scratch_mib=round(scratch.numel() / 2 ** 20, 1),
                                 rounds_ms=[round(v, 4) for v in ms], ms_per_step=round(_median(ms), 4),
                                 starved_share=round(float((status & bit).ne(0).float().mean().item()), 4), paths_sum=chk))
        finally:
            torch.cuda.synchronize()
            eng.unbind_exclusions()
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
