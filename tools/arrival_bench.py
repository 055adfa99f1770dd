"""Time the search step with a bound path trace, without and with an arrival rule (irs_set_arrival_rule), and count what the
rule saves in the until loop; write profiles/arrival/README.md from the recorded rows.

    python tools/arrival_bench.py --case off|rank1|half [--tree DIR] [--batch 4096] [--steps 20] [--rounds 5] [--label L] [--out F]
    python tools/arrival_bench.py --case report --rows profiles/arrival/arrival_bench.jsonl [--readme profiles/arrival/README.md]

The C2 shape (n_item 3415, d 128, L 200, 6 layers), --batch users, --steps steps, random windows and targets, k = 100, the trace
bound once before the calls.  ms per step = host clock around a call that ends in a device synchronise, divided by the steps; a
warm-up call first, then --rounds calls, every one reported, the median is the figure.  One process measures ONE side, so that
the sides can alternate as processes:

  --case off     irs_generate_paths, no rule.  --tree DIR takes the package (and its built library) from another checkout: the
                 parent commit's tree gives the figure this commit's rule-off run must not differ from.
  --case rank1   irs_generate_paths with rank_max = 1: on random targets the rule essentially never fires, so the difference to
                 `off` prices the added launch alone.  The row carries how many users were offered their target.
  --case half    irs_generate_paths_until without a rule, then with rank_max = the median over users of the best rank_target the
                 rule-off run recorded (about half the users arrive): steps run, row_steps and ms per call of both.
  --case report  no GPU: the README from the rows of --rows.
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
    return f"{row['ms_per_step']:.4f} ({min(r):.4f} – {max(r):.4f})"


def report(rows_path, readme):
    rows = [json.loads(l) for l in open(rows_path) if l.strip()]
    off = [r for r in rows if r["case"] == "off"]
    parent = [r for r in off if r["label"].startswith("parent")]
    this = [r for r in off if not r["label"].startswith("parent")]
    rank1 = [r for r in rows if r["case"] == "rank1"]
    half = [r for r in rows if r["case"] == "half"]
    first = rows[0]
    out = ["# Arrival rule (`irs_set_arrival_rule`): what the step costs with the rule off and on, and what the rule saves", "",
           "Written by `python tools/arrival_bench.py --case report` from `arrival_bench.jsonl` (one process per row, the processes "
           f"alternating inside one call on one MI355X, which torch names `{first['device']}`). The feature is off by default; these figures are all that is "
           "claimed about its speed. Nobody had measured any of this before.", "",
           f"C2 shape ({first['n_item']} items, d 128, L 200, 6 layers), {first['B']} users, {first['steps']} steps, k = 100, random "
           "windows and targets, the path trace bound once before the calls. Host clock around one call that ends in a device "
           "synchronise, divided by the steps; a warm-up call, then the rounds; the median is the figure, the range of the rounds in "
           "brackets.", "",
           "## (a) the parent commit and (b) this commit, trace bound, no rule", "",
           "The parent's package and library are taken with `--tree`. Processes in the order they ran:", "",
           "| process | ms / step | paths_sum | rank_sum |", "|---|---|---|---|"]
    for r in off:
        out.append(f"| {r['label']} | {_fmt(r)} | {r['paths_sum']} | {r['rank_sum']} |")
    if parent and this:
        pm, tm = [r["ms_per_step"] for r in parent], [r["ms_per_step"] for r in this]
        pr = [v for r in parent for v in r["rounds_ms"]]
        inside = sum(1 for v in tm if v <= max(pm))
        out += ["", f"The parent's own spread: its medians span {min(pm):.4f} – {max(pm):.4f} ms, its rounds {min(pr):.4f} – {max(pr):.4f}. "
                f"This commit's rule-off medians: {', '.join(f'{v:.4f}' for v in tm)}; {inside} of {len(tm)} lie inside the parent's span "
                f"of medians or below it, the highest {max(tm) - max(pm):+.4f} ms against the parent's highest median. `paths_sum` and "
                "`rank_sum` are the same number in every process: same inputs, same paths, same trace. With no rule set the loop launches "
                "what the parent launches; the host code differs by the `arr_on` tests in `enqueue_step` and the entry points."]
    out += ["", "## (c) `rank_max = 1`: the added launch alone", "",
            "On random targets the rule essentially never fires (`offered` users of the batch), so every step runs `k_arrival_offer` "
            "over all rows and rewrites next to nothing.", "", "| process | ms / step | offered |", "|---|---|---|"]
    for r in rank1:
        out.append(f"| {r['label']} | {_fmt(r)} | {r['offered']} of {r['B']} |")
    if rank1 and this:
        lo, hi = min(r["ms_per_step"] for r in this), max(r["ms_per_step"] for r in this)
        d = [r["ms_per_step"] for r in rank1]
        out += ["", f"Against this commit's rule-off processes ({lo:.4f} – {hi:.4f} ms): {min(d) - hi:+.4f} … {max(d) - lo:+.4f} ms per step "
                "for one more launch of one wave per row."]
    out += ["", "## (d) a rule at which about half the users arrive: `irs_generate_paths_until`", "",
            "`rank_max` = the median over users of the best `rank_target` the rule-off run recorded over its steps. `check_every = 1`. "
            "`row_steps` = decoded windows over all steps.", "",
            "| process | rule | steps run | row_steps | ms per call | users arrived | offered |", "|---|---|---|---|---|---|---|"]
    for r in half:
        for side in ("off", "on"):
            s = r[side]
            out.append(f"| {r['label']} | {'none' if side == 'off' else 'rank_max = %d' % r['rank_max']} | {s['steps']} | {s['row_steps']} | "
                       f"{s['ms_per_call']:.2f} ({min(s['rounds_ms']):.2f} – {max(s['rounds_ms']):.2f}) | {s['arrived']} of {r['B']} | {s['offered']} |")
    for r in half:
        out += ["", f"{r['label']}: row_steps {r['on']['row_steps']} against {r['off']['row_steps']} "
                f"({r['on']['row_steps'] / r['off']['row_steps']:.2f} of the rule-off loop's), "
                f"{r['on']['ms_per_call']:.2f} against {r['off']['ms_per_call']:.2f} ms per call."]
    here = os.path.dirname(os.path.abspath(rows_path))
    bench = os.path.join(here, "bench_ab.jsonl")
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
    dump = os.path.join(here, "dump_compare.txt")
    if os.path.exists(dump):
        names = [l.split()[1] for l in open(dump) if l.startswith("identical ")]
        bad = [l.split()[1] for l in open(dump) if l.startswith("DIFFERENT ")]
        out += ["", "## `bench.py --dump-outputs`: parent and this commit", "",
                f"The first pair of the call above wrote its outputs; `cmp` of every file (`dump_compare.txt`, with the SHA-256 of both "
                f"sides): {', '.join('`%s`' % n for n in names)} -- {len(names)} byte-identical, {len(bad)} different."]
    isa = os.path.join(here, "isa_kernel_diff.txt")
    if os.path.exists(isa):
        out += ["", "## Instruction sequences of the existing kernels", "",
                "`hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S` of `csrc/path.hip`, `csrc/score.hip` and "
                "`csrc/guide.hip` on the parent's tree and on this one, compared kernel by kernel with `tools/isa_kernel_diff.py` "
                "(`isa_kernel_diff.txt`):", ""]
        out += ["    " + l.rstrip() for l in open(isa)]
        out += ["", "The four kernels that exist only in the new `path.hip` are the instantiations of `k_arrival_offer<EXCL, SLOTS>`: "
                "43 – 44 VGPRs, no scratch, no LDS."]
    out.append("")
    with open(readme, "w") as f:
        f.write("\n".join(out))
    print(f"wrote {readme} from {len(rows)} rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("off", "rank1", "half", "report"), required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="profiles/arrival/arrival_bench.jsonl")
    ap.add_argument("--readme", default="profiles/arrival/README.md")
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
                 max_rows=B, max_seqs=B, max_k=100)
    eng.bind_state_dict({k: torch.from_numpy(v).to(DEV) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    seq0 = torch.from_numpy(synth.random_windows(B, cfg.max_len, cfg.n_item, seed=5)).to(DEV)
    users = (torch.arange(B, device=DEV) % cfg.n_user).to(torch.int64)
    hep0 = torch.full((B,), cfg.max_len - 2, dtype=torch.int32, device=DEV)
    paths = torch.zeros((B, steps), dtype=torch.float32, device=DEV)
    status = torch.zeros(B, dtype=torch.int32, device=DEV)
    seq, hep = seq0.clone(), hep0.clone()
    stats = {}

    def call(until):
        seq.copy_(seq0)
        hep.copy_(hep0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if until:
            out = eng.generate_paths_until(seq, users, hep, steps, k=100, sweep=IRS_SWEEP_BF16, paths=paths, status=status)
            stats["steps"], stats["row_steps"] = out[2], out[3]
        else:
            eng.generate_paths(seq, users, hep, steps, k=100, sweep=IRS_SWEEP_BF16, paths=paths, status=status)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def timed(until=False):
        call(until)
        return [call(until) for _ in range(a.rounds)]

    row = dict(bench="arrival", config="c2", n_item=cfg.n_item, B=B, steps=steps, k=100, label=a.label or a.case, case=a.case,
               device=torch.cuda.get_device_name(0))
    lp_item, lp_target, rank, scratch = eng.bind_path_trace(B, steps)
    try:
        if a.case in ("off", "rank1"):
            if a.case == "rank1":
                eng.set_arrival_rule(1, None)
            ms = [v / steps for v in timed()]
            torch.cuda.synchronize()
            row.update(rounds_ms=[round(v, 4) for v in ms], ms_per_step=round(_median(ms), 4),
                       paths_sum=int(paths.to(torch.float64).sum().item()), rank_sum=int(rank.to(torch.int64).sum().item()),
                       offered=int((status & 16).ne(0).sum().item()))
        else:
            targets = seq0[:, -1:].to(torch.float32)

            def side():
                ms = timed(until=True)
                torch.cuda.synchronize()
                return dict(steps=stats["steps"], row_steps=stats["row_steps"], rounds_ms=[round(v, 3) for v in ms],
                            ms_per_call=round(_median(ms), 3), arrived=int((paths == targets).any(dim=1).sum().item()),
                            offered=int((status & 16).ne(0).sum().item()))

            row["off"] = side()
            best = torch.where(rank > 0, rank, torch.full_like(rank, 2 ** 30)).min(dim=1).values
            row["rank_max"] = int(best.median().item())
            eng.set_arrival_rule(row["rank_max"], None)
            row["on"] = side()
    finally:
        if hasattr(eng, "set_arrival_rule"):
            eng.set_arrival_rule(None, None)
        eng.unbind_path_trace()
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
