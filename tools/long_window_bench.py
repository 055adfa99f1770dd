"""Time the rows-only decode behind long windows (irs_create_ex, IRS_CREATE_LONG_WINDOWS), next to the stock torch trunk.

    python tools/long_window_bench.py time [--lens 256,320,512,1024] [--batches 1,256] [--calls 20] [--rounds 5] [--out F]
    rocprofv3 --kernel-trace --pmc SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES --output-format csv -d DIR -- \\
        python tools/long_window_bench.py pmc-run [--len 1024] [--batch 256]
    python tools/long_window_bench.py pmc-report DIR [--out F]

time: the 6-layer c2-shaped model (n_item 3415, d 128, 4 heads, ffn 256) at max_len = L, rows-only decode (irs_decode with pos,
no x) of B random pre-padded windows (synth.random_windows: histories of every length up to L - 1), consumed at L - 2.  L = 256 is
the existing route, created through irs_create; above it the context comes from irs_create_ex.  ms per decode = host clock around
--calls decodes that end in a device synchronise, divided by the calls; a warm-up first, then --rounds such windows, every one
reported, the median is the figure.  Next to it, on the same GPU and inputs, the stock torch trunk (InfluentialNet's train-mode
path: nn.TransformerDecoder with the as-called float mask) in eval mode under no_grad -- what a user can run at these lengths
without this library's long windows; it computes every row, the library's figure is the consumed row only.
pmc-run: a few decodes for a counter pass of its own; pmc-report: k_attn_long's time per launch and the share of the matrix
pipe's cycles its float32 MFMAs keep busy (SQ_VALU_MFMA_BUSY_CYCLES over 4 SIMDs x 256 CUs x the busy clock cycles).
One JSON line per row."""
import argparse
import collections
import csv
import glob
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
DEV = "cuda:0"


def _median(v):
    return sorted(v)[len(v) // 2]


def _setup(L, B):
    import torch
    from influentialrs_amd import synth
    from influentialrs_amd._lib import IRS_MASK_IRN
    from influentialrs_amd.engine import Engine
    cfg = synth.make_config("c2", max_len=L, dropout=0.0)
    sd = synth.irn_state_dict(cfg, 1234)
    eng = Engine(n_item=cfg.n_item, n_user=cfg.n_user, d=cfg.emb_dim, max_len=L, n_heads=cfg.n_heads, ffn_dim=cfg.ffn_dim,
                 n_layers=cfg.n_layers, u_dim=cfg.u_emb_dim, mask_mode=IRS_MASK_IRN, device=torch.device(DEV), max_rows=B, max_seqs=B)
    eng.bind_state_dict({k: torch.from_numpy(v).to(DEV) for k, v in sd.items()})
    seq = torch.from_numpy(synth.random_windows(B, L, cfg.n_item, seed=5)).to(DEV)
    users = (torch.arange(B, device=DEV) % cfg.n_user).to(torch.int64)
    pos = torch.full((B,), L - 2, dtype=torch.int32, device=DEV)
    return cfg, sd, eng, seq, users, pos


def _timed(fn, calls, rounds):
    import torch

    def window():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls
    window()
    return [window() for _ in range(rounds)]


def cmd_time(a):
    import torch
    from influentialrs_amd.model.influentialRS import InfluentialNet
    rows = []
    for L in [int(v) for v in a.lens.split(",")]:
        for B in [int(v) for v in a.batches.split(",")]:
            cfg, sd, eng, seq, users, pos = _setup(L, B)
            ms = _timed(lambda: eng.decode(seq, users, want_x=False, pos=pos), a.calls, a.rounds)
            route = eng.decoder_route_last
            _, xr, _ = eng.decode(seq, users, want_x=False, pos=pos)
            net = InfluentialNet(cfg)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            net.to(DEV).eval()
            net.trunk = "torch"
            with torch.no_grad():
                stock = lambda: net._decoding_autograd(seq, users)[0]
                ms_t = _timed(stock, max(1, a.calls // 4), a.rounds)
                diff = float((stock()[torch.arange(B, device=DEV), pos.long()] - xr).abs().max().item())
            rows.append(dict(bench="rows_only_decode", config="c2", n_layers=cfg.n_layers, L=L, B=B, calls=a.calls,
                             entry="irs_create" if L <= 256 else "irs_create_ex",
                             route={k: route[k] for k in ("plan", "embed", "layer", "tail")},
                             rounds_ms=[round(v, 4) for v in ms], ms_per_decode=round(_median(ms), 4),
                             torch_rounds_ms=[round(v, 4) for v in ms_t], torch_ms_per_forward=round(_median(ms_t), 4),
                             max_abs_diff_vs_torch=diff, device=torch.cuda.get_device_name(0)))
            print(json.dumps(rows[-1]), flush=True)
            del eng, net
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def cmd_pmc_run(a):
    import torch
    cfg, sd, eng, seq, users, pos = _setup(a.len, a.batch)
    for _ in range(4):
        eng.decode(seq, users, want_x=False, pos=pos)
    torch.cuda.synchronize()
    print(json.dumps(dict(pmc_run=True, L=a.len, B=a.batch, decodes=4, packed_rows=int((seq != 0).sum().item()))), flush=True)


def cmd_pmc_report(a):
    f = glob.glob(os.path.join(a.dir, "**", "*counter_collection.csv"), recursive=True)[0]
    agg = collections.defaultdict(lambda: collections.defaultdict(list))
    dur = collections.defaultdict(dict)
    for r in csv.DictReader(open(f)):
        agg[r["Kernel_Name"]][r["Counter_Name"]].append(float(r["Counter_Value"]))
        dur[r["Kernel_Name"]][r["Dispatch_Id"]] = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    rows = []
    for name in agg:
        if "k_attn_long" not in name and "k_attn_row_long" not in name:
            continue
        m = {c: sum(v) / len(v) for c, v in agg[name].items()}
        ds = sorted(dur[name].values())
        clk = m["SQ_BUSY_CYCLES"] / 32.0  # the counter sums over 32 shader engines
        rows.append(dict(kernel=name.split("(")[0], launches=len(ds), median_us=ds[len(ds) // 2] / 1e3,
                         mfma_busy=m["SQ_VALU_MFMA_BUSY_CYCLES"] / (1024.0 * clk) if clk else None))  # 256 CUs x 4 SIMDs
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--lens", default="256,320,512,1024")
    t.add_argument("--batches", default="1,256")
    t.add_argument("--calls", type=int, default=20)
    t.add_argument("--rounds", type=int, default=5)
    t.add_argument("--out", default=None)
    p = sub.add_parser("pmc-run")
    p.add_argument("--len", type=int, default=1024)
    p.add_argument("--batch", type=int, default=256)
    r = sub.add_parser("pmc-report")
    r.add_argument("dir")
    r.add_argument("--out", default=None)
    a = ap.parse_args()
    {"time": cmd_time, "pmc-run": cmd_pmc_run, "pmc-report": cmd_pmc_report}[a.cmd](a)


if __name__ == "__main__":
    main()
