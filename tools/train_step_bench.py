"""Time IRSNN.train_batch with the stock and the native decoder trunk (net.trunk = "torch" | "hip") and with the chunked
and the fused backward of projection + cross entropy (net.ce_backward = "chunked" | "fused").

    python tools/train_step_bench.py [--configs default,c2,c4d] [--trunks torch,hip] [--ce chunked,fused] [--steps 20]
                                     [--warmup 5] [--batch B] [--project M,N,d[:M,N,d...]] [--rounds 3] [--out F]

Per (config, trunk): ms per whole train_batch step (trunk + projection / cross entropy + Adam), ms of the trunk's forward +
backward alone (same batch, dL/dx of ones), the trunk's share of the step, and kernel launches per step counted by the torch
profiler.  Configs: the reference default (B = 128, L = 60, d = 30, H = 6, ffn 256, dropout 0.05), c2 (B = 64, L = 200,
d = 128, H = 4) and c4d (B = 64, L = 200, d = 256, H = 8), all 6 layers and dropout 0.05.  One JSON line per row.

--project: projection only -- project_ce forward + backward on M random rows against an N-item, d-wide catalog (30 % pad
targets), per --ce route: ms per forward + backward (host clock around --steps calls that end in a device synchronise;
the routes alternate over --rounds rounds in one process, every round is reported and the median is the figure), the
forward's share, and the peak memory allocated beyond the live tensors (catalog, rows, gradients of the previous call).
Both routes see the same seeded inputs; their gradients are compared once (max |difference| over max |gradient|)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from influentialrs_amd import synth  # noqa: E402
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet  # noqa: E402

BATCH = {"default": 128, "c2": 64, "c4d": 64}


def _timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def _launches(fn):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type.name == "CUDA")
    except Exception:  # no device tracing in this torch build
        return None


def run_project(M, N, d, routes, steps, warmup, rounds):
    from influentialrs_amd.model import _backend
    nh = d // 32 if d % 32 == 0 else 1
    cfg = synth.make_config("tiny", n_item=N, emb_dim=d, n_heads=nh, n_layers=1, max_len=4, ffn_dim=8, n_user=2)
    net = InfluentialNet(cfg).to("cuda:0")
    g = torch.Generator(device="cuda:0")
    g.manual_seed(M + N)
    with torch.no_grad():
        net.project.weight.copy_((torch.rand((N, d), generator=g, device="cuda:0") * 2 - 1) * d ** -0.5)
        net.project.bias.copy_(torch.randn((N,), generator=g, device="cuda:0") * 0.1)
    x = torch.randn((M, d), generator=g, device="cuda:0", requires_grad=True)
    labels0 = torch.randint(0, N, (M,), generator=g, device="cuda:0")
    labels0[torch.rand((M,), generator=g, device="cuda:0") < 0.3] = -1

    def fwd():
        with torch.no_grad():
            _backend.project_ce(x, net.project, labels0, net._hip)

    def both():
        x.grad = net.project.weight.grad = net.project.bias.grad = None
        _backend.project_ce(x, net.project, labels0, net._hip).backward()

    ms = {r: [] for r in routes}
    ms_fwd, peak, grads = {}, {}, {}
    for r in routes:
        net.ce_backward = r
        for _ in range(warmup):
            both()
        grads[r] = (x.grad.clone(), net.project.weight.grad.clone(), net.project.bias.grad.clone())
        x.grad = net.project.weight.grad = net.project.bias.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        both()
        torch.cuda.synchronize()
        peak[r] = torch.cuda.max_memory_allocated() - base
        ms_fwd[r] = _timed(fwd, steps)
    for _ in range(rounds):
        for r in routes:
            net.ce_backward = r
            ms[r].append(_timed(both, steps))
    rows = []
    for r in routes:
        row = dict(bench="project_ce", ce=r, M=M, n_item=N, d=d, steps=steps, rounds_ms=[round(v, 3) for v in ms[r]],
                   ms_fwd_bwd=round(sorted(ms[r])[len(ms[r]) // 2], 3), ms_fwd=round(ms_fwd[r], 3),
                   peak_extra_mib=round(peak[r] / 2 ** 20, 1), device=torch.cuda.get_device_name(0))
        if r != routes[0]:
            row["max_rel_diff_vs_" + routes[0]] = [float("%.3g" % ((a - b).abs().max() / b.abs().max()).item())
                                                   for a, b in zip(grads[r], grads[routes[0]])]
        rows.append(row)
    return rows


def run(name, trunk, steps, warmup, batch=None, ce="chunked"):
    cfg = synth.make_config(name, dropout=0.05)
    B = batch or BATCH[name]
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    net.to("cuda:0")
    net.trunk = trunk
    net.ce_backward = ce
    irn = IRSNN(cfg, net, "cuda:0")
    seq = torch.from_numpy(synth.random_windows(B, cfg.max_len, cfg.n_item, seed=1)).cuda()
    user = torch.arange(B, device="cuda:0") % cfg.n_user

    def step():
        irn.train_batch(seq, user)

    def trunk_only():
        net.train()
        x, _ = net._decoding_autograd(seq, user)
        x.backward(torch.ones_like(x))

    for _ in range(warmup):
        step()
    ms_step = _timed(step, steps)
    ms_trunk = _timed(trunk_only, steps)
    return dict(config=name, trunk=trunk, ce=ce, B=B, L=cfg.max_len, d=cfg.emb_dim, H=cfg.n_heads, ffn=cfg.ffn_dim,
                layers=cfg.n_layers, dropout=cfg.dropout, ms_per_step=round(ms_step, 3), trunk_ms=round(ms_trunk, 3),
                trunk_share=round(ms_trunk / ms_step, 3), launches_per_step=_launches(step),
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="default,c2,c4d")
    ap.add_argument("--trunks", default="torch,hip")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="sequences per step for every config (default: per config)")
    ap.add_argument("--ce", default="chunked", help="projection + cross-entropy backward routes: chunked,fused")
    ap.add_argument("--project", default=None, help="projection-only timing at these M,N,d shapes (':'-separated)")
    ap.add_argument("--rounds", type=int, default=3, help="--project: alternating rounds per route")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    if a.project:
        for shape in a.project.split(":"):
            M, N, d = (int(v) for v in shape.split(","))
            for r in run_project(M, N, d, a.ce.split(","), a.steps, a.warmup, a.rounds):
                rows.append(r)
                print(json.dumps(r), flush=True)
    for name in (a.configs.split(",") if a.configs else []):
        for trunk in a.trunks.split(","):
            for ce in a.ce.split(","):
                r = run(name, trunk, a.steps, a.warmup, a.batch, ce)
                rows.append(r)
                print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
