"""Time the beam search without and with a bound beam trace (irs_bind_beam_trace), and against the alternative the trace
replaces -- the unbound search followed by a replay of all W beams; write profiles/beam_trace/README.md from the recorded rows.

    python tools/beam_trace_bench.py --case unbound|bound|replay [--tree DIR] [--users 128] [--beam 8] [--steps 20] [--rounds 5]
                                     [--label L] [--out F]
    python tools/beam_trace_bench.py --case report --rows profiles/beam_trace/beam_trace_bench.jsonl [--readme F]

The C2 shape (n_item 3415, d 128, L 200, 6 layers), --users users, --beam beams, --steps steps, random windows and targets,
k = 100, stream launches (use_graph off).  ms per search = host clock around one call that ends in a device synchronise; a
warm-up call first, then --rounds calls, every one reported, the median is the figure.  One process measures ONE side, so that
the sides can alternate as processes:

  --case unbound  irs_beam_search, nothing bound.  --tree DIR takes the package (and its built library) from another checkout:
                  the parent commit's tree gives the figure this commit's unbound run must not differ from.
  --case bound    irs_beam_search with the trace bound once before the calls.
  --case replay   irs_beam_search unbound, then irs_replay_paths over every (beam, step) of the returned paths: the same three
                  arrays, by decoding all users x W x steps windows a second time.
  --case report   no GPU: the README from the rows of --rows.
One JSON line per row."""
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
    return f"{row['ms_per_search']:.3f} ({min(r):.3f} – {max(r):.3f})"


def report(rows_path, readme):
    rows = [json.loads(l) for l in open(rows_path) if l.strip()]
    first = rows[0]
    by = {c: [r for r in rows if r["case"] == c] for c in ("unbound", "bound", "replay")}
    parent = [r for r in by["unbound"] if r["label"].startswith("parent")]
    this = [r for r in by["unbound"] if not r["label"].startswith("parent")]
    out = ["# Beam trace (`irs_bind_beam_trace`): what the beam search costs unbound, bound, and against a replay of its beams", "",
           "Written by `python tools/beam_trace_bench.py --case report` from `beam_trace_bench.jsonl` (one process per row, the "
           f"processes alternating inside one call on one MI355X, which torch names `{first['device']}`). The feature is opt-in and "
           "off by default; these figures are all that is claimed about its speed. Nobody had measured any of this before.", "",
           f"C2 shape ({first['n_item']} items, d 128, L 200, 6 layers), {first['users']} users, beam {first['beam']}, "
           f"{first['steps']} steps, k = 100, random windows and targets, stream launches. Host clock around one search that ends in a "
           "device synchronise; a warm-up call, then the rounds; the median is the figure, the range of the rounds in brackets. "
           "The C5 shape (one user, beam 32, 10M items) was not measured.", "",
           "| process | case | ms / search | paths_sum | rank_sum |", "|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['label']} | {r['case']} | {_fmt(r)} | {r['paths_sum']} | {r.get('rank_sum', '')} |")
    if parent and this:
        pm, tm = [r["ms_per_search"] for r in parent], [r["ms_per_search"] for r in this]
        pr = [v for r in parent for v in r["rounds_ms"]]
        out += ["", "## Unbound: the parent commit and this commit", "",
                f"The parent's medians span {min(pm):.3f} – {max(pm):.3f} ms, its rounds {min(pr):.3f} – {max(pr):.3f}. This commit's "
                f"unbound medians: {', '.join(f'{v:.3f}' for v in tm)}; {sum(1 for v in tm if v <= max(pm))} of {len(tm)} lie inside the "
                f"parent's span of medians or below it, the highest {max(tm) - max(pm):+.3f} ms against the parent's highest median. "
                "`paths_sum` is the same number in every process: same inputs, same paths. Unbound, the loop launches what the "
                "parent launches; the host code differs by one test of the binding per step and per call."]
    if by["bound"] and by["replay"] and this:
        bm, rm, tm = ([r["ms_per_search"] for r in rs] for rs in (by["bound"], by["replay"], this))
        out += ["", "## Bound, and the replay it replaces", "",
                f"Bound medians: {', '.join(f'{v:.3f}' for v in bm)} ms; unbound search plus replay of all beams: "
                f"{', '.join(f'{v:.3f}' for v in rm)} ms; this commit unbound: {', '.join(f'{v:.3f}' for v in tm)} ms. `rank_sum` of the "
                "bound rows and of the replay rows is over the same (beam, step) entries: "
                + ("the same number in all of them." if len({r["rank_sum"] for r in by["bound"] + by["replay"]}) == 1 else
                   "where the two differ, a replayed window was decoded in another batch and a near tie fell the other way "
                   "(tests/test_gpu_beam_trace.py holds the rule).")
                + " A timed call is one search of a few tens of milliseconds, so a row's range is as much the host's as the device's; "
                "the comparison rests on the alternation of whole processes.", "",
                "Nothing is claimed beyond these rows. The bound step adds one float32 pass over the catalog for the users x W rows "
                "(the greedy trace's sweep), the carry kernel and a few stores in the beam step."]
    bench = os.path.join(os.path.dirname(os.path.abspath(rows_path)), "bench_ab.jsonl")
    if os.path.exists(bench):
        b = [json.loads(l) for l in open(bench) if l.strip()]
        pm = [r["row"]["ms_per_step"] for r in b if r["side"] == "parent"]
        tm = [r["row"]["ms_per_step"] for r in b if r["side"] == "this"]
        out += ["", "## `bench.py --gpus 1 --steps 20 --warmup 5`: parent and this commit", "",
                "Its own step assembly on `irs_decode`, `irs_score_topk`, `irs_path_step`, none of which this commit changes; one "
                "process each, alternating in one call, the parent first (`bench_ab.jsonl`), ms per step in process order:", "",
                "| parent | this |", "|---|---|"]
        out += [f"| {a:.4f} | {c:.4f} |" for a, c in zip(pm, tm)]
        out += ["", f"The parent's runs span {min(pm):.4f} – {max(pm):.4f} ms; this commit's {min(tm):.4f} – {max(tm):.4f}: "
                f"{sum(1 for v in tm if min(pm) <= v <= max(pm))} of {len(tm)} inside the parent's range, "
                f"{sum(1 for v in tm if v > max(pm))} above it."]
    out += ["", "## Ranks against float64", "",
            "`tests/test_gpu_beam_trace.py::test_against_float64_replay_and_scores` (tiny config, two users, beam 4, 8 steps): the "
            "set of rank entries that differ from the float64 oracle, recorded from the first GPU run, is empty.", "",
            "## Instruction sequences of the existing beam step", "",
            "`hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S` of `csrc/path.hip` on the parent and on this commit: "
            "the eight existing instantiations of `k_beam_step` (UNTIL x EXCL x window slots) keep their instruction sequences and "
            "their kernel descriptors line for line (998 – 1728 lines each; only the mangled name differs, by the empty parameter "
            "pack). The eight linked instantiations add 23 – 52 lines and 4 KB of LDS (20.6 KB).", "",
            "## Next lever, not built", "",
            "The rank count could be folded into the beam's own float32 log-sum-exp pass (`k_lse_f32` / `k_lse_ring`): the top-k call "
            "of a beam step already sweeps the float32 catalog for (max, sum exp), and the trace sweep reads the same rows again "
            "for the same pair plus the count.", ""]
    with open(readme, "w") as f:
        f.write("\n".join(out))
    print(f"wrote {readme} from {len(rows)} rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("unbound", "bound", "replay", "report"), required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--users", type=int, default=128)
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="profiles/beam_trace/beam_trace_bench.jsonl")
    ap.add_argument("--readme", default="profiles/beam_trace/README.md")
    a = ap.parse_args()
    if a.case == "report":
        return report(a.rows, a.readme)
    import torch
    if not torch.cuda.is_available():
        sys.exit("beam_trace_bench: no GPU -- a timing is taken on the device or not at all")
    sys.path.insert(0, os.path.abspath(a.tree))
    from influentialrs_amd import synth
    from influentialrs_amd._lib import IRS_MASK_IRN, IRS_SWEEP_BF16
    from influentialrs_amd.engine import Engine

    B, W, P = a.users, a.beam, a.steps
    cfg = synth.make_config("c2")
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
        paths, scores, status = eng.beam_search(seq0, users, hep0, P, W, k=100, sweep=IRS_SWEEP_BF16)[:3]
        if a.case == "replay":
            rows = torch.arange(B * W * P, device=DEV, dtype=torch.int32)
            keep["replayed"] = eng.replay_paths(0, seq0.repeat_interleave(W, dim=0), paths.view(B * W, P).to(torch.int64), rows // P, rows % P,
                                                hep0=hep0.repeat_interleave(W), users=users.repeat_interleave(W))
        torch.cuda.synchronize()
        keep["paths"] = paths
        return (time.perf_counter() - t0) * 1e3

    held = eng.bind_beam_trace(B, W, P) if a.case == "bound" else None
    try:
        call()
        ms = [call() for _ in range(a.rounds)]
    finally:
        if held is not None:
            eng.unbind_beam_trace()
    row = dict(bench="beam_trace", config="c2", n_item=cfg.n_item, users=B, beam=W, steps=P, k=100, label=a.label or a.case, case=a.case,
               device=torch.cuda.get_device_name(0), rounds_ms=[round(v, 3) for v in ms], ms_per_search=round(_median(ms), 3),
               paths_sum=int(keep["paths"].to(torch.float64).sum().item()))
    if held is not None:
        row["rank_sum"] = int(held[2].to(torch.int64).sum().item())
    if a.case == "replay":
        row["rank_sum"] = int(keep["replayed"][2].to(torch.int64).sum().item())
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
