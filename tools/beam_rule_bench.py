"""Time the beam search under a bound beam trace without and with a beam rule (irs_set_beam_rule); write
profiles/beam_rule/README.md from the recorded rows.

    python tools/beam_rule_bench.py --case trace|weight|arrive [--tree DIR] [--config c2|c5] [--users N] [--beam W] [--steps P]
                                    [--rounds 5] [--label L] [--out F]
    python tools/beam_rule_bench.py --case report --rows profiles/beam_rule/beam_rule_bench.jsonl [--readme F]

The shapes of tools/beam_trace_bench.py: c2 (n_item 3415, d 128, L 200, 6 layers; 128 users, beam 8, 20 steps) and c5 (one user,
beam 32, 10 steps), random windows and targets, k = 100, stream launches (use_graph off).  ms per search = host clock around
one call that ends in a device synchronise; a warm-up call first, then --rounds calls, every one reported, the median is the
figure.  One process measures ONE side, so that the sides can alternate as processes:

  --case trace    irs_beam_search with a beam trace bound and no rule.  --tree DIR takes the package (and its built library) from
                  another checkout: the parent commit's tree gives the figure this commit's run must not differ from.
  --case weight   the same with the rule (0, off, lambda 0.5): ranking only, no beam is ever offered its target.
  --case arrive   the same with the rule (rank_max = n_item / 4, off, lambda 0.5): beams are offered their targets.
  --case report   no GPU: the README from the rows of --rows (and of bench_ab.jsonl and isa.txt beside them, where they exist).
One JSON line per row."""
import argparse
import json
import os
import sys
import time

DEV = "cuda:0"
SHAPES = {"c2": (128, 8, 20), "c5": (1, 32, 10)}


def _median(v):
    return sorted(v)[len(v) // 2]


def _fmt(row):
    r = row["rounds_ms"]
    return f"{row['ms_per_search']:.3f} ({min(r):.3f} – {max(r):.3f})"


def report(rows_path, readme):
    rows = [json.loads(l) for l in open(rows_path) if l.strip()]
    here = os.path.dirname(os.path.abspath(rows_path))
    out = ["# Beam rule (`irs_set_beam_rule`): what a traced beam search costs with no rule, with a weight, and with arrivals", "",
           "Written by `python tools/beam_rule_bench.py --case report` from `beam_rule_bench.jsonl` (one process per row, the "
           f"processes alternating inside one call on one MI355X, which torch names `{rows[0]['device']}`). The feature is opt-in and "
           "off by default. **No speed is claimed.** The one claim these rows are here to support: with no rule set, a search under a "
           "bound beam trace costs what the parent commit's costs, within the run-to-run spread of the alternated runs.", "",
           "Host clock around one `irs_beam_search` that ends in a device synchronise; a warm-up call, then the rounds; the median is "
           "the figure, the range of the rounds in brackets. k = 100, random windows and targets, stream launches.", ""]
    for config in sorted({r["config"] for r in rows}):
        rs = [r for r in rows if r["config"] == config]
        f = rs[0]
        out += [f"## {config}: {f['n_item']} items, {f['users']} users, beam {f['beam']}, {f['steps']} steps", "",
                "| process | case | ms / search | paths_sum | rank_sum | offered users |", "|---|---|---|---|---|---|"]
        out += [f"| {r['label']} | {r['case']} | {_fmt(r)} | {r['paths_sum']} | {r['rank_sum']} | {r['offered_users']} |" for r in rs]
        parent = [r for r in rs if r["case"] == "trace" and r["label"].startswith("parent")]
        this = [r for r in rs if r["case"] == "trace" and not r["label"].startswith("parent")]
        if parent and this:
            pm, tm = [r["ms_per_search"] for r in parent], [r["ms_per_search"] for r in this]
            pr = [v for r in parent for v in r["rounds_ms"]]
            out += ["", f"No rule: the parent's medians span {min(pm):.3f} – {max(pm):.3f} ms, its rounds {min(pr):.3f} – {max(pr):.3f}. "
                    f"This commit's medians: {', '.join(f'{v:.3f}' for v in tm)}; {sum(1 for v in tm if v <= max(pm))} of {len(tm)} lie "
                    f"inside the parent's span of medians or below it, the highest {max(tm) - max(pm):+.3f} ms against the parent's highest "
                    "median. `paths_sum` and `rank_sum` (the recorded ranks) are the same numbers in all of these processes: same inputs, same "
                    "paths, same trace. With no rule the loop "
                    "launches what the parent launches; the host code differs by one test of the rule per step."]
        for case, what in (("weight", "lambda 0.5 and no clause: nobody is offered"), ("arrive", "rank_max = n_item / 4 and lambda 0.5")):
            cm = [r["ms_per_search"] for r in rs if r["case"] == case]
            if cm:
                out += ["", f"`{case}` ({what}): medians {', '.join(f'{v:.3f}' for v in cm)} ms. The ruled step replaces the linked step "
                        "launch for launch; it reads four more values per beam row and keeps one more double per candidate in LDS."]
        out.append("")
    if "c5" not in {r["config"] for r in rows}:
        out += ["The C5 shape (one user, beam 32, 10M items) was not measured.", ""]
    bench = os.path.join(here, "bench_ab.jsonl")
    if os.path.exists(bench):
        b = [json.loads(l) for l in open(bench) if l.strip()]
        pm = [r["row"]["ms_per_step"] for r in b if r["side"] == "parent"]
        tm = [r["row"]["ms_per_step"] for r in b if r["side"] == "this"]
        out += ["## `bench.py --gpus 1 --steps 20 --warmup 5`: parent and this commit", "",
                "Its own step assembly on `irs_decode`, `irs_score_topk`, `irs_path_step`, none of which this commit changes; one "
                "process each, alternating, the parent first (`bench_ab.jsonl`: two calls, two pairs then three), ms per "
                "step in process order:", "",
                "| parent | this |", "|---|---|"]
        out += [f"| {a:.4f} | {c:.4f} |" for a, c in zip(pm, tm)]
        out += ["", f"The parent's runs span {min(pm):.4f} – {max(pm):.4f} ms; this commit's {min(tm):.4f} – {max(tm):.4f}.", ""]
    isa = os.path.join(here, "isa.txt")
    if os.path.exists(isa):
        out += ["## Instruction sequences of the existing kernels", "",
                "`hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S` of `csrc/path.hip`, `csrc/beam_trace.hip` and "
                "`csrc/score.hip` on the parent and on this commit, compared kernel by kernel with `tools/isa_kernel_diff.py` "
                "(`isa.txt`):", "", "```"] + open(isa).read().rstrip().split("\n") + ["```", ""]
    with open(readme, "w") as f:
        f.write("\n".join(out))
    print(f"wrote {readme} from {len(rows)} rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("trace", "weight", "arrive", "report"), required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--config", choices=sorted(SHAPES), default="c2")
    ap.add_argument("--users", type=int, default=None)
    ap.add_argument("--beam", type=int, default=None)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="profiles/beam_rule/beam_rule_bench.jsonl")
    ap.add_argument("--readme", default="profiles/beam_rule/README.md")
    a = ap.parse_args()
    if a.case == "report":
        return report(a.rows, a.readme)
    import torch
    if not torch.cuda.is_available():
        sys.exit("beam_rule_bench: no GPU -- a timing is taken on the device or not at all")
    sys.path.insert(0, os.path.abspath(a.tree))
    from influentialrs_amd import synth
    from influentialrs_amd._lib import IRS_MASK_IRN, IRS_SWEEP_BF16
    from influentialrs_amd.engine import Engine

    B, W, P = (given or shape for given, shape in zip((a.users, a.beam, a.steps), SHAPES[a.config]))
    cfg = synth.make_config(a.config)
    eng = Engine(n_item=cfg.n_item, n_user=cfg.n_user, d=cfg.emb_dim, max_len=cfg.max_len, n_heads=cfg.n_heads,
                 ffn_dim=cfg.ffn_dim, n_layers=cfg.n_layers, u_dim=cfg.u_emb_dim, mask_mode=IRS_MASK_IRN, device=torch.device(DEV),
                 max_rows=B * W, max_seqs=B * W, max_k=100)
    eng.bind_state_dict({k: torch.from_numpy(v).to(DEV) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    seq0 = torch.from_numpy(synth.random_windows(B, cfg.max_len, cfg.n_item, seed=5)).to(DEV)
    users = (torch.arange(B, device=DEV) % cfg.n_user).to(torch.int64)
    hep0 = torch.full((B,), cfg.max_len - 2, dtype=torch.int32, device=DEV)
    keep = {}

    def call():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep["paths"], _, keep["status"] = eng.beam_search(seq0, users, hep0, P, W, k=100, sweep=IRS_SWEEP_BF16)[:3]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    held = eng.bind_beam_trace(B, W, P)  # (the arrays and the scratch are the caller's: kept alive while bound)
    try:
        if a.case != "trace":  # (the parent's tree has no rule to set: --tree goes with --case trace)
            eng.set_beam_rule(cfg.n_item // 4 if a.case == "arrive" else None, None, 0.5)
        call()
        ms = [call() for _ in range(a.rounds)]
    finally:
        if a.case != "trace":
            eng.set_beam_rule(None, None, 0.0)
        eng.unbind_beam_trace()
    row = dict(bench="beam_rule", config=a.config, n_item=cfg.n_item, users=B, beam=W, steps=P, k=100, label=a.label or a.case, case=a.case,
               device=torch.cuda.get_device_name(0), rounds_ms=[round(v, 3) for v in ms], ms_per_search=round(_median(ms), 3),
               paths_sum=int(keep["paths"].to(torch.float64).sum().item()), offered_users=int((keep["status"] & 16).ne(0).sum().item()),
               rank_sum=int(held[2].to(torch.int64).sum().item()))
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
