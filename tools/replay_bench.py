"""Time Evaluator.get_path_metrics_in_batch (one batched replay, irs_replay_paths) against the methods it stands in for.

    python tools/replay_bench.py [--batch 128] [--steps 20] [--rounds 7] [--only replay] [--out F]

The evaluator's default shape (eval_default: n_item 3415, d 30, L 60, 6 layers), --batch users with FULL windows (L history
items each, so every step shifts the window) and --steps-step paths that close with the target.  Both sides run in this one
process and alternate round by round: get_rr_increase_in_batch + get_grad_in_batch (what the replay replaces), then
get_path_metrics_in_batch; get_pp_in_batch, which stays out of the replay, is timed beside them.  ms per call = host clock
around a call that ends with its results on the host (every method returns numpy); a warm-up call of each first, then --rounds
calls, every one reported, the median is the figure.  The row also says how far the two sides' results are apart.
--only replay: the warm-up and ONE call of the replay alone (the run to put a kernel trace around).  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from influentialrs_amd import harness, synth  # noqa: E402
from influentialrs_amd.model.evaluator import Evaluator  # noqa: E402
from influentialrs_amd.model.uRS import SampleNet  # noqa: E402

DEV = "cuda:0"


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=("replay",), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, S = a.batch, a.steps
    cfg = synth.make_config("eval_default")
    L, N = cfg.max_len, cfg.n_item
    net = SampleNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 17, evaluator=True).items()})
    net.to(DEV)
    ev = Evaluator(cfg, net, DEV)
    ev.eval()
    rng = np.random.default_rng(5)
    hists = rng.integers(1, N, (B, L))        # full windows; item N is everybody's target and occurs nowhere else
    paths = rng.integers(1, N, (B, S - 1))    # build_eval_nn1 closes each path with the target: S steps
    targets = np.full(B, N, dtype=np.int64)
    data = harness.build_eval_nn1(list(hists), paths, targets, seq_len=L)
    h, d, t, sp, lp = (x.to(DEV) for x in next(iter(harness.eval_batches_nn1(data, B))))
    assert int(lp.min()) == S and int(lp.max()) == S

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    old = lambda: (ev.get_rr_increase_in_batch(h, d, t), ev.get_grad_in_batch(h, d, t, sp, lp))  # noqa: E731
    new = lambda: ev.get_path_metrics_in_batch(h, d, t, sp, lp)  # noqa: E731
    pp = lambda: ev.get_pp_in_batch(d, sp, lp)  # noqa: E731
    row = dict(bench="evaluator_replay", config="eval_default", n_item=N, d=cfg.emb_dim, L=L, n_layers=cfg.n_layers, B=B, steps=S,
               rows=B * S, chunk=min(B * S, ev.REPLAY_CHUNK), device=torch.cuda.get_device_name(0))
    with torch.no_grad():
        if a.only == "replay":
            timed(new)
            ms, _ = timed(new)
            row.update(only="replay", replay_ms=round(ms, 3))
        else:
            timed(old), timed(new), timed(pp)
            ms_old, ms_new, ms_pp = [], [], []
            for _ in range(a.rounds):
                m0, (rr, grad) = timed(old)
                m1, m = timed(new)
                m2, _ = timed(pp)
                ms_old.append(m0), ms_new.append(m1), ms_pp.append(m2)
            row.update(loop_rounds_ms=[round(v, 3) for v in ms_old], replay_rounds_ms=[round(v, 3) for v in ms_new],
                       pp_rounds_ms=[round(v, 3) for v in ms_pp], loop_ms=round(_median(ms_old), 3),
                       replay_ms=round(_median(ms_new), 3), pp_ms=round(_median(ms_pp), 3),
                       t_probs_max_diff=float(np.abs(m["t_probs"] - grad[0]).max()),
                       p_probs_max_diff=float(np.abs(m["p_probs"] - grad[1]).max()),
                       ir_equal=int((m["ir"] == rr[1]).sum()), irr_max_diff=float(np.abs(m["irr"] - rr[0]).max()))
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
