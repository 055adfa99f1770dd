"""Time irs_recommend against the calls it is built on and the formulation it replaces.

    python tools/recommend_bench.py --shape c2|1m [--rows R] [--n 20] [--k 100] [--rounds 5] [--out F]

One catalog, one set of decoder-shaped rows (random, seeded), windows of max_len - 1 random items.  Four things are timed on the
same rows, alternating inside every round:

  topk_lse        Engine.score_topk_lse(rows, k)                  -- what irs_recommend starts with
  recommend       Engine.recommend(rows, n, windows, k)           -- + flag pass, (strips, merge,) take
  sort_mask       Engine.score_dense, torch.sort(descending), drop what the window holds, cut n   -- the reference's formulation
  mask_topk       Engine.score_dense, masked_fill(-inf), torch.topk(n)                            -- its cheapest torch form

with no short row (random windows hide almost nothing of a row's top k) and with 1 % of the rows short (their windows hold their
own top 120 items, so the strips and the merge run for them).  ms per call = host clock around `reps` calls that end in one
device synchronise, divided by reps; a warm-up of every variant first; every round is reported, the median is the figure.
The slates of `recommend` are compared with `mask_topk`'s on the spot (ids_equal: rows whose n ids are the same in order; scores
that tie may swap in torch's order).  One JSON line per variant."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

DEV = "cuda:0"
SHAPES = {"c2": dict(n_item=3415, d=128, L=200, rows=4096), "1m": dict(n_item=1_000_000, d=128, L=200, rows=1024)}


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from influentialrs_amd import synth
    from influentialrs_amd._lib import IRS_MASK_IRN, IRS_ROW_RESCUED, IRS_SWEEP_BF16
    from influentialrs_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("recommend_bench: no GPU: a timing taken anywhere else says nothing")
    sh = SHAPES[a.shape]
    N, d, L, M = sh["n_item"], sh["d"], sh["L"], a.rows or sh["rows"]
    n, k = a.n, a.k
    cfg = synth.make_config("tiny", n_item=N, emb_dim=d, n_heads=4, n_layers=1, max_len=L, ffn_dim=8, n_user=2)
    eng = Engine(n_item=N, n_user=cfg.n_user, d=d, max_len=L, n_heads=4, ffn_dim=8, n_layers=1, u_dim=cfg.u_emb_dim,
                 mask_mode=IRS_MASK_IRN, device=torch.device(DEV), max_rows=M, max_seqs=1, max_k=k)
    sd = synth.irn_state_dict(cfg, seed=1)
    g = torch.Generator(device="cpu").manual_seed(3)
    sd["project.weight"] = ((torch.rand((N, d), generator=g) * 2 - 1) / np.sqrt(d)).numpy()
    sd["project.bias"] = (torch.randn(N, generator=g) * 0.1).numpy()
    eng.bind_state_dict({k_: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k_, v in sd.items()})
    x = torch.randn((M, d), generator=g).to(DEV)
    win_plain = torch.randint(1, N + 1, (M, L), generator=g).to(DEV)
    hep = torch.full((M,), L - 2, dtype=torch.int32, device=DEV)
    _, top_ids, _, _, _ = eng.score_topk_lse(x, k)
    n_short = max(1, M // 100)
    win_short = win_plain.clone()
    short_rows = torch.arange(0, M, M // n_short, device=DEV)[:n_short]
    full = eng.score_dense(x[short_rows])
    win_short[short_rows, :120] = torch.topk(full, 120, dim=1).indices + 1
    del full

    def hidden_of(win):
        h = torch.zeros((M, N), dtype=torch.bool, device=DEV)
        h.scatter_(1, win[:, :L - 1] - 1, True)
        return h

    def topk_lse(win):
        return eng.score_topk_lse(x, k)

    def recommend(win):
        return eng.recommend(x, n, seqs=win, hep=hep, k=k, sweep=IRS_SWEEP_BF16)

    def sort_mask(win):
        logits = eng.score_dense(x)
        val, idx = torch.sort(logits, dim=1, descending=True)
        keep = ~hidden_of(win).gather(1, idx)
        sel = keep & (keep.cumsum(1) <= n)
        return val[sel].view(M, n), idx[sel].view(M, n)

    def mask_topk(win):
        logits = eng.score_dense(x)
        return torch.topk(logits.masked_fill_(hidden_of(win), float("-inf")), n, dim=1)

    variants = [("topk_lse", topk_lse), ("recommend", recommend), ("sort_mask", sort_mask), ("mask_topk", mask_topk)]
    base = dict(bench="recommend", shape=a.shape, n_item=N, d=d, L=L, rows=M, n=n, k=k, device=torch.cuda.get_device_name(0))
    rows_out = []
    for case, win in (("no_short_row", win_plain), ("1pct_short_rows", win_short)):
        got = recommend(win)
        want = mask_topk(win)
        torch.cuda.synchronize()
        rescued = int((got[4] & IRS_ROW_RESCUED).ne(0).sum().item())
        ids_equal = int((got[1] == want.indices).all(dim=1).sum().item())
        val_equal = int((got[0] == want.values).all(dim=1).sum().item())
        del want
        reps = {}
        for name, fn in variants:  # warm-up, and the repetitions that fill about a fifth of a second
            fn(win)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(win)
            torch.cuda.synchronize()
            reps[name] = max(1, min(200, int(0.2 / max(time.perf_counter() - t0, 1e-5))))
        ms = {name: [] for name, _ in variants}
        for _ in range(a.rounds):
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps[name]):
                    fn(win)
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / reps[name])
        for name, _ in variants:
            rows_out.append(dict(base, case=case, variant=name, reps=reps[name], rounds_ms=[round(v, 4) for v in ms[name]],
                                 ms_per_call=round(_median(ms[name]), 4), rescued_rows=rescued, ids_equal_rows=ids_equal,
                                 values_equal_rows=val_equal))
    for r in rows_out:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in rows_out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
