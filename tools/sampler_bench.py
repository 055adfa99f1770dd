"""Time the search step greedy, with the stock sampled step (sample = 1, sample_k = 3) and with a bound sampler (irs_bind_sampler);
write profiles/sampler/README.md from the recorded rows.

    python tools/sampler_bench.py --case greedy|stock|bound [--tree DIR] [--batch 4096] [--steps 20] [--rounds 7] [--top-k 3]
                                  [--temperature 1] [--top-p 1] [--label L] [--out F]
    python tools/sampler_bench.py --case report --rows profiles/sampler/sampler_bench.jsonl [--readme profiles/sampler/README.md]

The C2 shape (n_item 3415, d 128, L 200, 6 layers), --batch users, --steps steps, random windows and targets, k = 100.  ms per
step = host clock around one irs_generate_paths call (stream launches) that ends in a device synchronise, divided by the steps; a
warm-up call first, then --rounds calls, every one reported, the median is the figure.  One process measures ONE side, so that
the sides can alternate as processes: compare two versions by alternating them, and trust a difference only beyond the spread of
equal sides.  --tree DIR takes the package (and its built library) from
another checkout: the parent commit's tree gives the greedy and the stock figures of the parent.
--case report needs no GPU: the README from the rows of --rows.  One JSON line per row."""
import argparse
import json
import os
import sys
import time

DEV = "cuda:0"


def _median(v):
    return sorted(v)[len(v) // 2]


def _fmt(row):
    r = row["rounds_ms"]
    return f"{row['ms_per_step']:.4f} ({min(r):.4f} – {max(r):.4f})"


def report(rows_path, readme):
    rows = [json.loads(l) for l in open(rows_path) if l.strip()]
    first = rows[0]
    out = ["# Bound sampler (`irs_bind_sampler`): what a search step costs greedy, with the stock sampled step and with the sampler bound", "",
           "Written by `python tools/sampler_bench.py --case report` from `sampler_bench.jsonl` (one process per row, the sides "
           f"alternating as processes on one MI355X, which torch names `{first['device']}`). The feature is off by default. No speed "
           "is claimed: the bound step is the greedy step plus one launch of `k_sampler_choose`, one wave per row, and these "
           "figures are all that was measured.", "",
           f"C2 shape ({first['n_item']} items, d 128, L 200, 6 layers), {first['steps']} steps, k = 100, random windows and targets. "
           "Host clock around one `irs_generate_paths` call (stream launches, no captured step) that ends in a device synchronise, "
           "divided by the steps; a warm-up call, then the rounds; the median is the figure, the range of the rounds in brackets. "
           "`parent` rows run the parent commit's package and library (`--tree`); `paths_sum` is the sum of all path entries, a "
           "check that equal sides chose equal paths.", ""]
    for B in sorted({r["B"] for r in rows}, reverse=True):
        out += [f"## B = {B}", ""]
        if B * first["steps"] < 1024:
            out += [f"A call at B = {B} times about {first['steps']} steps of launch overhead, a few milliseconds of work: this is an "
                    "overhead figure (what one more launch adds to a latency-bound step), not a throughput figure.", ""]
        out += ["| process | step | ms / step | paths_sum |", "|---|---|---|---|"]
        mine = [r for r in rows if r["B"] == B]
        for r in mine:
            what = {"greedy": "greedy", "stock": "stock sample = 1, sample_k = 3",
                    "bound": f"bound sampler top_k = {r.get('top_k')}, T = {r.get('temperature')}, top_p = {r.get('top_p')}"}[r["case"]]
            out.append(f"| {r['label']} | {what} | {_fmt(r)} | {r['paths_sum']} |")
        med = {}
        for r in mine:
            med.setdefault((r["label"].startswith("parent"), r["case"], r.get("top_k")), []).append(r["ms_per_step"])
        g = med.get((False, "greedy", None))
        if g:
            out.append("")
            for (parent, case, top_k), v in sorted(med.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2] or 0)):
                name = ("parent " if parent else "this ") + case + (f" top_k = {top_k}" if top_k else "")
                out.append(f"- {name}: medians {', '.join(f'{x:.4f}' for x in v)} ms; against this commit's greedy medians "
                           f"({min(g):.4f} – {max(g):.4f}): {min(v) - max(g):+.4f} … {max(v) - min(g):+.4f} ms per step")
        out.append("")
    with open(readme, "w") as f:
        f.write("\n".join(out))
    print(f"wrote {readme} from {len(rows)} rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("greedy", "stock", "bound", "report"), required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--top-k", type=int, default=3)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="profiles/sampler/sampler_bench.jsonl")
    ap.add_argument("--readme", default="profiles/sampler/README.md")
    a = ap.parse_args()
    if a.case == "report":
        return report(a.rows, a.readme)
    import torch
    sys.path.insert(0, os.path.abspath(a.tree))
    from influentialrs_amd import synth
    from influentialrs_amd._lib import IRS_MASK_IRN, IRS_SWEEP_BF16
    from influentialrs_amd.engine import Engine

    B, steps = a.batch, a.steps
    cfg = synth.make_config("c2")
    eng = Engine(n_item=cfg.n_item, n_user=cfg.n_user, d=cfg.emb_dim, max_len=cfg.max_len, n_heads=cfg.n_heads,
                 ffn_dim=cfg.ffn_dim, n_layers=cfg.n_layers, u_dim=cfg.u_emb_dim, mask_mode=IRS_MASK_IRN, device=torch.device(DEV),
                 max_rows=max(B, 8), max_seqs=max(B, 8), max_k=100)
    eng.bind_state_dict({k: torch.from_numpy(v).to(DEV) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    seq0 = torch.from_numpy(synth.random_windows(B, cfg.max_len, cfg.n_item, seed=5)).to(DEV)
    users = (torch.arange(B, device=DEV) % cfg.n_user).to(torch.int64)
    hep0 = torch.full((B,), cfg.max_len - 2, dtype=torch.int32, device=DEV)
    paths = torch.zeros((B, steps), dtype=torch.float32, device=DEV)
    status = torch.zeros(B, dtype=torch.int32, device=DEV)
    seq, hep = seq0.clone(), hep0.clone()
    kw = dict(sample=True, sample_k=3, seed=11) if a.case == "stock" else dict(seed=11)

    def call():
        seq.copy_(seq0)
        hep.copy_(hep0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.generate_paths(seq, users, hep, steps, k=100, sweep=IRS_SWEEP_BF16, paths=paths, status=status, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    row = dict(bench="sampler", config="c2", n_item=cfg.n_item, B=B, steps=steps, k=100, label=a.label or a.case, case=a.case,
               device=torch.cuda.get_device_name(0))
    if a.case == "bound":
        eng.bind_sampler(a.top_k, a.temperature, a.top_p)
        row.update(top_k=a.top_k, temperature=a.temperature, top_p=a.top_p)
    try:
        call()
        ms = [call() / steps for _ in range(a.rounds)]
        row.update(rounds_ms=[round(v, 4) for v in ms], ms_per_step=round(_median(ms), 4),
                   paths_sum=int(paths.to(torch.float64).sum().item()))
    finally:
        if a.case == "bound":
            torch.cuda.synchronize()
            eng.unbind_sampler()
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
