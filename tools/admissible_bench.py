"""Time the search step with nothing bound, with a path trace, and with the admissible rank on top of it (irs_bind_trace_admissible)
under no list, ml-1m-shaped lists + no_repeat and 4096-id lists; write the tables of profiles/admissible/README.md from the rows.

    python tools/admissible_bench.py --case unbound|trace|adm|adm_ml1m|adm_4096|trace_ml1m|trace_4096 [--tree DIR] [--batch 4096] [--steps 20] [--rounds 5]
                                     [--label L] [--out F]
    python tools/admissible_bench.py --case report --rows profiles/admissible/admissible_bench.jsonl

The C2 shape (n_item 3415, d 128, L 200, 6 layers), --batch users, --steps steps, random windows and targets, k = 100, everything
bound once before the calls.  ms per step = host clock around one irs_generate_paths call that ends in a device synchronise,
divided by the steps; a warm-up call first, then --rounds calls, every one reported, the median is the figure.  One process
measures ONE side, so that the sides can alternate as processes:

  --case unbound   nothing bound.  --tree DIR takes the package (and its built library) from another checkout: the parent
                   commit's tree gives the figure this commit's unbound run must not differ from.
  --case trace     the path trace bound.
  --case adm       trace + admissible rank, no exclusion list: H is the window, rank_adm == rank_target (the row says so).
  --case adm_ml1m  trace + admissible rank, lists shaped like ml-1m histories (log-normal lengths, median 93 ids, the longest
                   2276) and no_repeat.
  --case adm_4096  trace + admissible rank, every user's list 4096 ids wide (about 2390 distinct items of the 3415).
  --case trace_ml1m / trace_4096   the same lists under the trace alone: what the admissible rank adds on top of them.
  --case report    no GPU: the markdown tables from the rows of --rows, to stdout.
One JSON line per row."""
import argparse
import json
import os
import sys
import time

DEV = "cuda:0"


def _median(v):
    return sorted(v)[len(v) // 2]


def report(rows_path):
    rows = [json.loads(l) for l in open(rows_path) if l.strip()]
    print("| process | case | ms / step (rounds) | paths_sum | rank_sum | rank_adm_sum | list ids (median / longest) |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        ms = r["rounds_ms"]
        print(f"| {r['label']} | {r['case']} | {r['ms_per_step']:.4f} ({min(ms):.4f} – {max(ms):.4f}) | {r['paths_sum']} | "
              f"{r.get('rank_sum', '')} | {r.get('rank_adm_sum', '')} | {r.get('list_median', '')} / {r.get('list_longest', '')} |")
    by = {}
    for r in rows:
        by.setdefault(r["case"] + (":parent" if r["label"].startswith("parent") else ""), []).append(r["ms_per_step"])
    print()
    for k, v in by.items():
        print(f"- {k}: medians {', '.join(f'{x:.4f}' for x in v)} ms")


def ml1m_lengths(B, g, np):
    n = np.clip(np.round(93 * np.exp(g.standard_normal(B))).astype(np.int64), 1, 2276)
    n[0] = 2276
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("unbound", "trace", "adm", "adm_ml1m", "adm_4096", "trace_ml1m", "trace_4096", "report"), required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="profiles/admissible/admissible_bench.jsonl")
    a = ap.parse_args()
    if a.case == "report":
        return report(a.rows)
    import numpy as np
    import torch
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
        return (time.perf_counter() - t0) * 1e3

    row = dict(bench="admissible", config="c2", n_item=cfg.n_item, B=B, steps=steps, k=100, label=a.label or a.case, case=a.case,
               device=torch.cuda.get_device_name(0))
    held, trace, adm_held = [], None, None  # (what the bindings return: kept alive while bound)
    listed = a.case.endswith(("_ml1m", "_4096"))
    try:
        if listed:
            g = np.random.default_rng(7)
            if a.case.endswith("_4096"):
                ids = g.integers(0, cfg.n_item, (B, 4096)).astype(np.int64)
            else:
                n = ml1m_lengths(B, g, np)
                ids = np.full((B, int(n.max())), -1, dtype=np.int64)
                for b in range(B):
                    ids[b, :n[b]] = g.permutation(cfg.n_item)[:n[b]]
            valid = (ids >= 0).sum(axis=1)
            row.update(list_median=int(np.median(valid)), list_longest=int(valid.max()))
            held.append(eng.bind_exclusions(torch.from_numpy(ids).to(DEV), no_repeat=a.case.endswith("_ml1m")))
        if a.case != "unbound":
            trace = eng.bind_path_trace(B, steps)
        if a.case.startswith("adm"):
            adm_held = eng.bind_trace_admissible(B, steps)
        call()
        ms = [call() / steps for _ in range(a.rounds)]
        torch.cuda.synchronize()
        row.update(rounds_ms=[round(v, 4) for v in ms], ms_per_step=round(_median(ms), 4),
                   paths_sum=int(paths.to(torch.float64).sum().item()))
        if a.case != "unbound":
            rank = trace[2]
            row.update(rank_sum=int(rank.to(torch.int64).sum().item()))
        if a.case.startswith("adm"):
            adm = adm_held[0]
            row.update(rank_adm_sum=int(adm.to(torch.int64).sum().item()), adm_le_rank=bool((adm <= rank).all().item()))
    finally:
        if a.case != "unbound":
            eng.unbind_path_trace()
        if listed:
            eng.unbind_exclusions()
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
