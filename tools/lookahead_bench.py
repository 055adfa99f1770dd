"""Time the C2 search step with and without a bound lookahead (irs_bind_lookahead: the one-step lookahead choice).

    python tools/lookahead_bench.py --case unbound|bound [--tree DIR] [--batch N] [--steps 20] [--rounds 5] [--kcs 2,5]
                                    [--no-parts] [--out F]

irs_generate_paths at the C2 shape (n_item 3415, d 128, L 200, 6 layers; --batch users, --steps steps, random windows and
targets, k = 100).  ms per step = host clock around a call that ends in a device synchronise, divided by the steps; a warm-up
call first, then --rounds calls, every one reported, the median is the figure.  One process measures ONE side, so that the
sides can alternate as processes:

  --case unbound   nothing bound, --batch 4096 by default.  --tree DIR takes the package (and its built library) from another
                   checkout: the parent commit's tree gives the figure this commit's unbound run must not differ from.
  --case bound     --batch 768 by default, so that B k_c fits the context's 4096 sequences at k_c = 5.  The plain step at that
                   batch, then the bound step for k_c = 2 and k_c = 5 (the binding is made once before the calls), and the parts
                   the bound step is expected to be made of, each timed alone over the same number of repeats: the rows-only
                   decode of B and of B k_c windows, the LSE sweep and the one-id gather over B k_c rows.  paths_moved is the
                   share of path entries that differ from the unbound run's.  --kcs picks other candidate counts, --no-parts
                   leaves the parts out (a short process to put under a kernel trace).
One JSON line per row."""
import argparse
import json
import os
import sys
import time

import torch

DEV = "cuda:0"
MAX_SEQS = 4096


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("unbound", "bound"), required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kcs", default="2,5")
    ap.add_argument("--no-parts", action="store_true")
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from influentialrs_amd import synth
    from influentialrs_amd._lib import IRS_MASK_IRN, IRS_SWEEP_BF16
    from influentialrs_amd.engine import Engine

    B = a.batch if a.batch is not None else (4096 if a.case == "unbound" else 768)
    steps = a.steps
    cfg = synth.make_config("c2")
    eng = Engine(n_item=cfg.n_item, n_user=cfg.n_user, d=cfg.emb_dim, max_len=cfg.max_len, n_heads=cfg.n_heads,
                 ffn_dim=cfg.ffn_dim, n_layers=cfg.n_layers, u_dim=cfg.u_emb_dim, mask_mode=IRS_MASK_IRN, device=torch.device(DEV),
                 max_rows=MAX_SEQS, max_seqs=MAX_SEQS, max_k=100)
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

    def timed(fn=call):
        fn()
        ms = [fn() for _ in range(a.rounds)]
        return ms, int(paths.to(torch.float64).sum().item())

    def part(fn):
        """ms per launch of `fn`, `steps` launches per round like a search call."""
        def one():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / steps
        return timed(one)[0]

    base = dict(bench="generate_paths", config="c2", B=B, steps=steps, k=100, label=a.label or a.case,
                device=torch.cuda.get_device_name(0))

    def row(case, ms, **kw):
        return dict(base, case=case, rounds_ms=[round(v, 4) for v in ms], ms_per_step=round(_median(ms), 4), **kw)
    rows = []
    ms, chk = timed()
    unbound = paths.clone()
    rows.append(row("unbound", ms, paths_sum=chk))
    if a.case == "bound":
        kcs = [int(v) for v in a.kcs.split(",")]
        for k_c in kcs:
            if B * k_c > MAX_SEQS:
                raise SystemExit(f"--batch {B} x k_c {k_c} exceeds the context's {MAX_SEQS} sequences")
            eng.bind_lookahead(k_c, B, steps)
            try:
                ms, chk = timed()
                rows.append(row(f"lookahead k_c={k_c}", ms, k_c=k_c, paths_sum=chk,
                                paths_moved=round(float((paths != unbound).float().mean().item()), 4)))
            finally:
                torch.cuda.synchronize()
                eng.unbind_lookahead()
        # the parts, each alone: windows as the search starts from (children differ from parents in one slot)
        for n in ([] if a.no_parts else [B] + [k_c * B for k_c in kcs if k_c > 1]):
            s_n, u_n, h_n = seq0.repeat(n // B, 1), users.repeat(n // B), hep0.repeat(n // B)
            rows.append(row(f"decode rows-only {n}", part(lambda: eng.decode(s_n, u_n, want_x=False, pos=h_n)), rows_decoded=n))
            if n > B:
                _, xr, _ = eng.decode(s_n, u_n, want_x=False, pos=h_n)
                ids = (s_n[:, -1:] - 1).contiguous()
                rows.append(row(f"score_lse {n}", part(lambda: eng.score_lse(xr)), rows_scored=n))
                rows.append(row(f"score_gather 1 id {n}", part(lambda: eng.score_gather(xr, ids)), rows_scored=n))
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
