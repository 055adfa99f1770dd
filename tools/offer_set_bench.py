"""Measurements behind profiles/offer_set/README.md: the offer set's ranking next to what exists.

    python tools/offer_set_bench.py --leg small|large|search|kernel [--out FILE]

Every leg prints JSON lines (and appends them to --out).  Times are device events around one call, after warm-up: the median and
the minimum of --iters calls.  Operations are counted from shapes here: a score pass is 2 M C d.
  small   N = 3415, d = 128, 4096 rows: irs_score_topk_offer at C = N, N/10, N/100; irs_score_topk (both sweeps) on the same rows;
          irs_score_gather of the C ids per row + torch.topk, what a caller can do without the binding
  large   N = 1 M, d = 128, 1024 rows: the same (the gather leg not at C = N: its id array alone is 8 GB)
  search  the c2 shape (N = 3415, d = 128, max_len = 200, six layers), 20 greedy steps of 1024 users: unbound, and bound to N/10
  kernel  one offer call per shape and nothing else, for a kernel trace taken around this process
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from gpu_util import make_engine, scoring_only_engine  # noqa: E402
from influentialrs_amd import synth  # noqa: E402
from influentialrs_amd._lib import IRS_SWEEP_BF16, IRS_SWEEP_F32  # noqa: E402

DEV = "cuda:0"
K = 100


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def emit(out, **rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def catalog(n_item, d, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    W = (torch.randn((n_item, d), generator=g) / d ** 0.5).numpy()
    b = (0.1 * torch.randn(n_item, generator=g)).numpy()
    return W, b


def subset(n_item, C, seed=0):
    return torch.from_numpy(np.sort(np.random.default_rng(seed + C).permutation(n_item)[:C])).to(DEV)


def scoring_leg(name, n_item, M, iters, out, pass_rows, gather_max_c, kernel_only=False):
    d = 128
    W, b = catalog(n_item, d, 1)
    eng = scoring_only_engine(n_item, d, W, b, max_rows=M, max_k=K)
    x = torch.randn((M, d), generator=torch.Generator(device="cpu").manual_seed(2)).to(DEV)
    base = dict(leg=name, n_item=n_item, d=d, rows=M, k=K)
    for C in (n_item, n_item // 10, n_item // 100):
        S = subset(n_item, C)
        rows = min(M, pass_rows)
        eng.bind_offer_set(S, rows, prepared=True)
        if kernel_only:
            eng.score_topk_offer(x, K)
            torch.cuda.synchronize()
            eng.unbind_offer_set()
            emit(out, **base, what="offer (one call, for the kernel trace)", C=C, pass_rows=rows, flop_scores=2.0 * M * C * d)
            continue
        med, best = timed(lambda: eng.score_topk_offer(x, K), iters)
        eng.unbind_offer_set()
        emit(out, **base, what="irs_score_topk_offer", C=C, pass_rows=rows, ms_median=med, ms_min=best,
             tflops_whole_call=2.0 * M * C * d / (med * 1e-3) / 1e12)
        if C <= gather_max_c:
            ids = S.unsqueeze(0).expand(M, C).contiguous()

            def today():
                sc = eng.score_gather(x, ids)
                v, i = torch.topk(sc, min(K, C), dim=1)
                return v, torch.gather(ids, 1, i)

            med, best = timed(today, max(3, iters // 2))
            emit(out, **base, what="irs_score_gather + torch.topk", C=C, ms_median=med, ms_min=best)
            del ids
    if kernel_only:
        return
    for sweep, label in ((IRS_SWEEP_BF16, "bf16"), (IRS_SWEEP_F32, "f32")):
        med, best = timed(lambda: eng.score_topk(x, K, sweep), iters)
        emit(out, **base, what=f"irs_score_topk ({label} sweep, whole catalog)", C=n_item, ms_median=med, ms_min=best)


def search_leg(iters, out):
    cfg = synth.make_config("c2")
    sd = synth.irn_state_dict(cfg, 1234)
    B, P = 1024, 20
    eng = make_engine(cfg, sd, max_rows=B, max_seqs=B, max_k=K)
    g = np.random.default_rng(5)
    seqs = torch.from_numpy(g.integers(1, cfg.n_item + 1, (B, cfg.max_len)).astype(np.int64)).to(DEV)
    users = torch.from_numpy(g.integers(0, cfg.n_user, B).astype(np.int64)).to(DEV)
    hep = torch.full((B,), cfg.max_len - 2, dtype=torch.int32, device=DEV)

    def run():
        return eng.generate_paths(seqs.clone(), users, hep.clone(), P, k=K)

    base = dict(leg="search", workload="c2", users=B, steps=P, k=K)
    med, best = timed(run, iters, warm=2)
    emit(out, **base, what="irs_generate_paths, nothing bound", ms_median=med, ms_min=best)
    C = cfg.n_item // 10
    S = subset(cfg.n_item, C)
    eng.bind_offer_set(S, B, prepared=True)
    med, best = timed(run, iters, warm=2)
    paths = run()[0]
    eng.unbind_offer_set()
    live = paths[paths > 0].to(torch.int64) - 1
    assert bool(torch.isin(live, S).all())
    emit(out, **base, what="irs_generate_paths, offer set bound", C=C, ms_median=med, ms_min=best)
    med, best = timed(run, iters, warm=2)
    emit(out, **base, what="irs_generate_paths, nothing bound (again, after the unbind)", ms_median=med, ms_min=best)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["small", "large", "search", "kernel"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("offer_set_bench: needs the GPU (there is nothing to measure without one)")
    t0 = time.time()
    emit(a.out, leg=a.leg, device=torch.cuda.get_device_name(0), torch=torch.__version__)
    if a.leg == "small":
        scoring_leg("small", 3415, 4096, a.iters, a.out, 4096, 3415)
    elif a.leg == "large":
        scoring_leg("large", 1_000_000, 1024, max(3, a.iters // 4), a.out, 1024, 100_000)
    elif a.leg == "search":
        search_leg(max(3, a.iters // 4), a.out)
    else:
        scoring_leg("kernel_small", 3415, 4096, 1, a.out, 4096, 0, kernel_only=True)
        scoring_leg("kernel_large", 1_000_000, 1024, 1, a.out, 1024, 0, kernel_only=True)
    emit(a.out, leg=a.leg, wall_s=round(time.time() - t0, 1))


if __name__ == "__main__":
    main()
