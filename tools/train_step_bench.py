"""Time IRSNN.train_batch with the stock and the native decoder trunk (net.trunk = "torch" | "hip").

    python tools/train_step_bench.py [--configs default,c2,c4d] [--trunks torch,hip] [--steps 20] [--warmup 5] [--batch B]
                                     [--out F]

Per (config, trunk): ms per whole train_batch step (trunk + projection / cross entropy + Adam), ms of the trunk's forward +
backward alone (same batch, dL/dx of ones), the trunk's share of the step, and kernel launches per step counted by the torch
profiler.  Configs: the reference default (B = 128, L = 60, d = 30, H = 6, ffn 256, dropout 0.05), c2 (B = 64, L = 200,
d = 128, H = 4) and c4d (B = 64, L = 200, d = 256, H = 8), all 6 layers and dropout 0.05.  One JSON line per row."""
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


def run(name, trunk, steps, warmup, batch=None):
    cfg = synth.make_config(name, dropout=0.05)
    B = batch or BATCH[name]
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    net.to("cuda:0")
    net.trunk = trunk
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
    return dict(config=name, trunk=trunk, B=B, L=cfg.max_len, d=cfg.emb_dim, H=cfg.n_heads, ffn=cfg.ffn_dim,
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.configs.split(","):
        for trunk in a.trunks.split(","):
            r = run(name, trunk, a.steps, a.warmup, a.batch)
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
