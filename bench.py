#!/usr/bin/env python3
"""Benchmark of the hot path: one persuasion-path search STEP over a batch of users

    step = decoder over B windows -> row at history end -> score against the whole
           catalog -> top-100 -> window filter + greedy choice + window shift

(IRSNN.get_seq_in_batch's loop body, reference model/influentialRS.py:412-450).
Metric (BASELINE.json): scored user-item pairs/sec = users x n_item / time, whole job.
Headline workload = BASELINE.json configs[1] (C2): ml-1m-shaped, d=128, L=200, H=4,
6 layers, F=256, N=3415, synthetic weights and windows, inputs resident in HBM.

    python bench.py                       # 1 GPU
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, runs W warm-up steps, times K steps and prints the headline line (metric, value, unit, ms_per_step,
higher_is_better, dtype, config).  `--dump-outputs DIR` writes what the last timed step returned (rows, top-100 lists, next
items, windows) as DIR/<name>.npy; the inputs are seeded, so two builds can be compared output for output.

With `--full`, besides the headline line items the JSON carries the instrumented per-family pass (`roofline`,
`step_roofline`, `kernels`), the self-check (`verified`), the path-search latencies and
  * `scoring`: irs_score_topk and its emission sweep alone on the catalog-scale shapes (1M x 128 = C3,
    1.25M x 256 = C4's per-GPU shard) for 1 / 32 / 1024 rows, each with its fraction of the bf16 MFMA peak
    (>= 315 rows) or of the HBM floor of streaming the bf16 catalog once (small row counts);
  * `c4_item_sharded`: BASELINE configs[3] -- a 10M-item, d=256 catalog cut into N item shards (one GPU: the whole
    catalog = the N=1 anchor): rows all-gathered over RCCL, every rank sweeps its shard, ONE all_to_all of packed
    64-bit top-100 keys, merge, path step.  The C2 headline itself replicates its 1.7 MB catalog and
    partitions the users (no data-path collective);
  * `cpu_baseline`: the CPU restatement timed on this box's host cores (B-equiv and B-row).
"""
from __future__ import annotations

import argparse
import json
import threading
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

PEAK_F32_MATRIX_TFLOPS = 157.3  # MI355X_MICROARCH.md: fp32 MFMA (exact f32) dense peak
PEAK_BF16_TFLOPS = 2500.0       # dense bf16 MFMA
PEAK_HBM_GBS = 8000.0           # HBM3E spec
# Multi-rank legs: the sharded step runs below the C ABI either way; replaying it from a captured hipGraph (RCCL calls
# inside) is covered by the one-rank RCCL tests but has never run on more than one device, so the first real multi-GPU
# bench keeps to plain stream launches unless asked (a 12 ms C4 step gains nothing from it; C5's sub-millisecond steps would).
SHARDED_GRAPH = os.environ.get("IRS_BENCH_SHARDED_GRAPH", "0") == "1"


# ---------------------------------------------------------------------------------------------------- CPU baselines
def _cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _cpu_row_worker(job):
    """One worker of the B-row leg: greedy path steps for its users, consumed row only (single-threaded numpy + C)."""
    cfg_name, seqs, users, steps, seed = job
    from threadpoolctl import threadpool_limits
    from influentialrs_amd import synth
    from oracle import oracle_np as O
    O.lib().orc_set_threads(1)
    cfg = synth.make_config(cfg_name)
    sd = _CPU_SD
    W, b = sd["project.weight"], sd["project.bias"]
    hep = cfg.max_len - 2
    with threadpool_limits(limits=1):
        x, _ = O.decode(sd, cfg, seqs[0], users[0])  # warm-up (page in the weights, BLAS initialisation after the fork)
        t0 = time.perf_counter()
        for _ in range(steps):
            for r in range(seqs.shape[0]):
                x, _ = O.decode(sd, cfg, seqs[r], users[r])
                s = O.score_chain(x[hep], W, b)
                vals, ids0 = O.topk(s, 100)
                nxt = O.select_next(ids0 + 1, vals, seqs[r][:hep + 1])
                seqs[r][:-2] = seqs[r][1:-1].copy()
                seqs[r][-2] = nxt
    return seqs.shape[0] * steps, time.perf_counter() - t0


_CPU_SD = None


def cpu_baseline(cfg_name, budget_s=10.0):
    """The oracle (CPU restatement, kind "port") on this box's host cores, bounded samples of the headline workload.
    Runs BEFORE the process touches the GPU (it forks workers).  Checker code used as a yard-stick, never shipped.

    B-equiv (`value`): what the reference does per path step (influentialRS.py:412-434) -- decoder, logits of ALL L
      rows against the catalog, softmax over N for every row, top-100 of the consumed row, window filter, shift --
      one user at a time (the only batch size the published IRN runs at), numpy on `threads` BLAS threads.
    B-row: the fair algorithmic baseline -- consumed row only, 128 users per step spread over single-threaded
      worker processes on all cores (numpy float32 decoder + C fma-chain scoring / top-100)."""
    global _CPU_SD
    import multiprocessing as mp
    import subprocess
    from threadpoolctl import threadpool_limits
    so = os.path.join(REPO, "oracle", "_build", "liboracle.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(REPO, "oracle")], stdout=subprocess.DEVNULL)
    from influentialrs_amd import synth
    from oracle import oracle_np as O
    cfg = synth.make_config(cfg_name)
    sd = synth.irn_state_dict(cfg, 1234)
    _CPU_SD = sd
    cores = os.cpu_count() or 1
    W, b = sd["project.weight"], sd["project.bias"]
    hep = cfg.max_len - 2
    # ---- B-equiv: torch CPU operators, like the reference itself (oracle/oracle_torch.py); thread count = the
    #      fastest of a short calibration (tiny operators do not scale to hundreds of threads)
    import torch
    from oracle import oracle_torch as OT
    irn = OT.TorchIRN(sd, cfg)
    seqs = [torch.from_numpy(s_) for s_ in synth.random_windows(4, cfg.max_len, cfg.n_item, seed=3)]
    prev_threads = torch.get_num_threads()
    best = None
    for cand in sorted({min(cores, c) for c in (4, 8, 16, 32, 64)}):
        torch.set_num_threads(cand)
        for _ in range(3):
            irn.path_step_like_reference(seqs[0], 0, hep)
        ts = []
        for _ in range(12):
            t0 = time.perf_counter()
            irn.path_step_like_reference(seqs[0], 0, hep)
            ts.append(time.perf_counter() - t0)
        t = float(np.median(ts))
        if best is None or t < best[0]:
            best = (t, cand)
    thr = best[1]
    torch.set_num_threads(thr)
    done, t0 = 0, time.perf_counter()
    while True:
        for r in range(4):
            _, seqs[r] = irn.path_step_like_reference(seqs[r], r, hep)
            done += 1
        if time.perf_counter() - t0 > budget_s or done >= 4000:
            break
    dt_e = time.perf_counter() - t0
    torch.set_num_threads(prev_threads)
    equiv = done * cfg.n_item / dt_e
    # ---- B-row
    nproc = min(cores, 128)
    B = 128
    seqs = synth.random_windows(B, cfg.max_len, cfg.n_item, seed=5)
    users = np.arange(B)
    per = (B + nproc - 1) // nproc
    steps = 2
    # size the sample from the B-equiv step time (a consumed-row step costs about the same decoder work)
    est = 2.5 * (dt_e / max(done, 1)) * per  # numpy decoder: ~2.5x the torch step
    steps = int(max(1, min(40, budget_s / max(est, 1e-3))))
    jobs = [(cfg_name, seqs[i:i + per].copy(), users[i:i + per], steps, i) for i in range(0, B, per)]
    ctx = mp.get_context("fork")
    t0 = time.perf_counter()
    with ctx.Pool(len(jobs)) as pool:
        res = pool.map(_cpu_row_worker, jobs)
    dt_wall = time.perf_counter() - t0
    n_done = sum(r_[0] for r_ in res)
    dt_r = max(r_[1] for r_ in res)  # the slowest worker's compute time (pool start-up excluded)
    row = n_done * cfg.n_item / dt_r
    return {"value": equiv, "unit": "pairs/s", "cores": thr, "kind": "port",
            "sample": f"B-equiv: {done} greedy path steps (4 users, B=1 loop; all {cfg.max_len} rows scored, softmax over "
                      f"{cfg.n_item} items per row, top-100, filter, shift; torch CPU operators like the reference) in {dt_e:.1f}s on "
                      f"{thr} threads (fastest of a 4..64-thread calibration)",
            "b_row": {"value": row, "unit": "pairs/s", "cores": len(jobs),
                      "sample": f"{steps} steps x {B} users (consumed row only) over {len(jobs)} single-threaded worker "
                                f"processes: slowest worker {dt_r:.1f}s ({dt_wall:.1f}s with fork + pool start-up)"},
            "ms_per_user_step_b_equiv": dt_e / max(done, 1) * 1e3,
            "host": {"cpu_model": _cpu_model(), "logical_cpus": cores},
            "b_ref_note": "B-ref (the unmodified reference's pipeline.test_model timed in the build container) is recorded in "
                          "BASELINE.md section 4 (tools/time_reference.py)"}


# ---------------------------------------------------------------------------------------------------- GPU side
def gpu_state_dict(cfg, device, seed=1234, item_lo=0, item_hi=None, with_embedding=True):
    """Same init families as synth.irn_state_dict, generated on the device (large catalogs: no host round trip).
    project.weight / project.bias hold only rows [item_lo, item_hi): an item-sharded rank never materialises the
    rest of the table.  Rows come from per-chunk generators (1M rows each), so every shard layout of the same
    catalog draws identical numbers."""
    import torch
    from influentialrs_amd import synth
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    d, F, N = cfg.emb_dim, cfg.ffn_dim, cfg.n_item
    item_hi = N if item_hi is None else item_hi

    def normal(*shape, std=1.0, gen=g):
        return torch.randn(*shape, generator=gen, device=device, dtype=torch.float32) * std

    def uniform(*shape, bound, gen=g):
        return (torch.rand(*shape, generator=gen, device=device, dtype=torch.float32) * 2 - 1) * bound

    sd = {}
    if with_embedding:
        E = normal(N + 1, d)
        E[0] = 0
        sd["item_embedder.weight"] = E
    sd["user_embedder.weight"] = normal(cfg.n_user, cfg.u_emb_dim)
    sd["user_mask_layer.weight"] = uniform(1, cfg.u_emb_dim, bound=cfg.u_emb_dim ** -0.5)
    sd["user_mask_layer.bias"] = normal(1, std=0.1)
    sd["pos_embedder.pe"] = torch.from_numpy(synth.positional_encoding(d, cfg.max_len)).to(device)
    CH = 1 << 20
    pw = torch.empty((item_hi - item_lo, d), dtype=torch.float32, device=device)
    pb = torch.empty((item_hi - item_lo,), dtype=torch.float32, device=device)
    for c in range(item_lo // CH, (item_hi + CH - 1) // CH):
        gc = torch.Generator(device=device)
        gc.manual_seed(seed * 100003 + c)
        lo, hi = c * CH, min((c + 1) * CH, N)
        w = uniform(hi - lo, d, bound=d ** -0.5, gen=gc)
        bb = normal(hi - lo, std=0.1, gen=gc)
        a, e = max(lo, item_lo), min(hi, item_hi)
        pw[a - item_lo:e - item_lo] = w[a - lo:e - lo]
        pb[a - item_lo:e - item_lo] = bb[a - lo:e - lo]
        del w, bb
    sd["project.weight"], sd["project.bias"] = pw, pb
    xav = (6.0 / (4 * d)) ** 0.5
    for l in range(cfg.n_layers):
        p = f"decoder.layers.{l}."
        for att in ("self_attn", "multihead_attn"):
            sd[p + att + ".in_proj_weight"] = uniform(3 * d, d, bound=xav)
            sd[p + att + ".in_proj_bias"] = normal(3 * d, std=0.1)
            sd[p + att + ".out_proj.weight"] = uniform(d, d, bound=d ** -0.5)
            sd[p + att + ".out_proj.bias"] = normal(d, std=0.1)
        sd[p + "linear1.weight"] = uniform(F, d, bound=d ** -0.5)
        sd[p + "linear1.bias"] = normal(F, std=0.1)
        sd[p + "linear2.weight"] = uniform(d, F, bound=F ** -0.5)
        sd[p + "linear2.bias"] = normal(d, std=0.1)
        for n in ("norm1", "norm2", "norm3"):
            sd[p + n + ".weight"] = 1.0 + normal(d, std=0.05)
            sd[p + n + ".bias"] = normal(d, std=0.05)
    return sd


_ZIPF_CDF = {}


def zipf_distinct_ids(B, L, n_item, device, gen):
    """[B, L] item ids drawn Zipf(s = 1) over the catalog WITHOUT repeats inside a row (the host generator
    synth.user_histories draws the same law user by user): 4 L inverse-CDF draws per row, duplicates dropped keeping the first
    occurrence, the first L distinct ones kept.  A row that still comes up short (a tiny catalog) is topped up from a random
    permutation of the ids it lacks."""
    import torch
    key = (n_item, str(device))
    if key not in _ZIPF_CDF:
        p = 1.0 / torch.arange(1, n_item + 1, device=device, dtype=torch.float64)
        _ZIPF_CDF.clear()
        _ZIPF_CDF[key] = torch.cumsum(p / p.sum(), 0)
    cdf = _ZIPF_CDF[key]
    K = min(max(4 * L, 64), max(n_item, 1) * 4)
    out = torch.zeros((B, L), dtype=torch.int64, device=device)
    rows = torch.arange(B, device=device)[:, None].expand(B, K)
    u = torch.rand((B, K), generator=gen, device=device, dtype=torch.float64)
    cand = (torch.searchsorted(cdf, u.reshape(-1)).reshape(B, K) + 1).clamp(max=n_item)
    sv, si = torch.sort(cand, dim=1, stable=True)
    dup_s = torch.zeros_like(sv, dtype=torch.bool)
    dup_s[:, 1:] = sv[:, 1:] == sv[:, :-1]
    keep = ~torch.zeros_like(dup_s).scatter_(1, si, dup_s)
    rank = keep.cumsum(1) - 1
    m = keep & (rank < L)
    out[rows[m], rank[m]] = cand[m]
    short = (keep.sum(1) < L).nonzero().flatten().tolist()
    for b in short:  # (rare: only when 4 L draws hold fewer than L distinct ids)
        have = out[b][out[b] > 0]
        lack = torch.ones(n_item + 1, dtype=torch.bool, device=device)
        lack[0] = False
        lack[have] = False
        pool = lack.nonzero().flatten()
        need = L - have.numel()
        if pool.numel() >= need:
            out[b, have.numel():] = pool[torch.randperm(pool.numel(), generator=gen, device=device)[:need]]
        else:  # a catalog smaller than the window: repeats are unavoidable
            out[b, have.numel():] = torch.randint(1, n_item + 1, (need,), generator=gen, device=device)
    return out


def gpu_windows(B, L, n_item, device, seed):
    """ml-1m-shaped evaluation windows: history length log-normal (median 95, sigma 0.95)
    clipped to [18, 2276]; items Zipf(s = 1) without repeats per user; the window keeps the last L-1 history items,
    pre-padded, target last = a uniformly drawn item absent from the window
    (DataLoaderEvalIRS layout, reference data_provider.py:591-617; target rule :427-429)."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    seqs = zipf_distinct_ids(B, L, n_item, device, g)
    tgt = torch.randint(1, n_item + 1, (B,), generator=g, device=device, dtype=torch.int64)
    for _ in range(8):
        clash = (seqs[:, :L - 1] == tgt[:, None]).any(1)
        if not bool(clash.any()):
            break
        tgt = torch.where(clash, torch.randint(1, n_item + 1, (B,), generator=g, device=device, dtype=torch.int64), tgt)
    seqs[:, L - 1] = tgt
    ln = torch.exp(torch.randn((B, 1), generator=g, device=device) * 0.95 + float(np.log(95.0)))
    hl = ln.clamp(18, 2276).long().clamp(max=L - 1)  # items kept in the window
    col = torch.arange(L, device=device)[None, :]
    seqs[col < (L - 1 - hl)] = 0
    return seqs


def packed_fraction(job):
    """Fraction of the B*L window slots the decoder actually computes (non-pad tokens; the consumed row
    always counts).  The decoder packs them, so executed work scales with this."""
    import torch
    s = job.seqs
    valid = (s != 0)
    valid[torch.arange(s.shape[0], device=s.device), job.hep.long()] = True
    return float(valid.sum().item()) / float(s.numel())


class Job:
    """One workload on this rank: engine, weights (the local item shard only when sharded), windows, one step."""

    def __init__(self, workload, batch, rank, world, device, shard, sweep, n_item=0):
        import torch
        from influentialrs_amd import synth
        from influentialrs_amd._lib import IRS_MASK_IRN, IRS_SWEEP_BF16, IRS_SWEEP_F32
        from influentialrs_amd.engine import Engine, shard_bounds
        self.rank, self.world, self.device = rank, world, device
        self.cfg = synth.make_config(workload)
        if n_item:
            self.cfg.n_item = n_item
        cfg = self.cfg
        self.B = batch
        self.k = 100
        self.sweep = IRS_SWEEP_F32 if sweep == "f32" else IRS_SWEEP_BF16
        # Where the path shards: a large catalog is cut into item shards (one exchange step per search
        # step); a catalog that fits every GPU many times over is replicated and the USERS are partitioned, with no
        # data-path collective at all.
        self.sharded = world > 1 and (shard == "items" or (shard == "auto" and cfg.n_item >= 262144))
        rows = self.B * world if self.sharded else self.B
        self.eng = Engine(n_item=cfg.n_item, n_user=cfg.n_user, d=cfg.emb_dim, max_len=cfg.max_len,
                          n_heads=cfg.n_heads, ffn_dim=cfg.ffn_dim, n_layers=cfg.n_layers, u_dim=cfg.u_emb_dim,
                          mask_mode=IRS_MASK_IRN, device=device, max_rows=rows, max_seqs=self.B, max_k=self.k,
                          rank=rank if self.sharded else 0, world=world if self.sharded else 1)
        if cfg.n_item <= 100_000:
            sd = {k: torch.from_numpy(v).to(device) for k, v in synth.irn_state_dict(cfg, 1234).items()}
            if self.sharded:  # keep this rank's rows only
                lo, hi = shard_bounds(cfg.n_item, world, rank)
                sd["project.weight"] = sd["project.weight"][lo:hi].clone()
                sd["project.bias"] = sd["project.bias"][lo:hi].clone()
        else:
            lo, hi = shard_bounds(cfg.n_item, world, rank) if self.sharded else (0, cfg.n_item)
            sd = gpu_state_dict(cfg, device, 1234, lo, hi)
        self.eng.bind_state_dict(sd)
        self.sd = sd
        self.seqs = gpu_windows(self.B, cfg.max_len, cfg.n_item, device, seed=100 + rank)
        gu = torch.Generator(device=device)  # seeded like the windows: the same users in every run
        gu.manual_seed(200 + rank)
        self.users = torch.randint(0, cfg.n_user, (self.B,), generator=gu, device=device, dtype=torch.int64)
        self.hep = torch.full((self.B,), cfg.max_len - 2, dtype=torch.int32, device=device)
        self.paths = torch.zeros((self.B, 1), dtype=torch.float32, device=device)
        self.carry = False
        self.last_status = None
        self.last_out = None  # (rows, top-k values, top-k ids) of the latest single-GPU step: what --dump-outputs writes
        self.status = torch.zeros(self.B, dtype=torch.int32, device=device)
        self.comm = None
        if self.sharded:
            from influentialrs_amd.engine import Comm
            self.comm = Comm(device)  # RCCL (backend nccl) or, for the one-GPU rehearsal, gloo through the host
            self.x_all = torch.empty((rows, cfg.emb_dim), dtype=torch.float32, device=device)
            self.k_recv = torch.empty((world, self.B, self.k), dtype=torch.int64, device=device)

    def step(self):
        eng = self.eng
        if not self.sharded:
            _, xr, _ = eng.decode(self.seqs, self.users, want_x=False, pos=self.hep)
            # (the rows are the previous step's rows one item later: irs_score_topk_carry skips the pre-pass and the threshold
            #  selection on 7 steps of 8 on shards of >= 524288 items -- what irs_generate_paths does between its own steps)
            val, ids, st = eng.score_topk(xr, self.k, self.sweep, carry=self.carry)
            self.carry = True
            self.last_status = st
            self.last_out = (xr, val, ids)
            eng.path_step(self.seqs, self.hep, val, ids, 0, self.paths, self.status)
        else:
            # one search step below the C ABI (irs_generate_paths_sharded): decode -> row all-gather -> sweep of this rank's
            # item shard for all rows -> pack -> ONE all-to-all of 64-bit keys -> merge -> path step, one stream-ordered
            # sequence over workspace buffers (IRS_BENCH_SHARDED_GRAPH=1: replayed from a hipGraph over RCCL)
            eng.generate_paths_sharded(self.comm, self.seqs, self.users, self.hep, 1, k=self.k, sweep=self.sweep,
                                       use_graph=SHARDED_GRAPH and self.comm.is_rccl, paths=self.paths, status=self.status)


VERIFY_JOB_HOW = ("4 rows of the last step: ring-sweep top-100 (emission thresholds carried from the previous step, as in the timed loop; `fallback_rows` "
                  "counts the rows of nine such steps that had to take the exhaustive path) == float32-sweep top-100 (ids and value bits); 4 users of the last step "
                  "re-decoded 4 per call on the small-batch float32-chain kernels (pinned to the reference goldens irn_c2 / irn_c3 / "
                  "irn_c4d by tests/test_gpu_decoder_path.py): rows within 7.5e-5 of the throughput kernels'")
VERIFY_ROW_TOL = 7.5e-5  # decoder rows through the split-precision throughput kernels vs the small-batch float32 kernels (d = 256 bound of tests/test_gpu_decoder_path.py)


def verify_job(job, n=4):
    """Self-check of a catalog-scale leg: the rows of the windows as the timed loop left them go through the SAME
    irs_score_topk call the loop ran (>= 256 rows: the LDS-DMA ring sweep), and `n` of them are re-scored with the
    float32 sweep (another kernel family, the exact chain end to end): ids and value bits must be equal; `n` users are decoded
    again on the small-batch float32-chain kernels and their rows must agree within VERIFY_ROW_TOL.  Sharded: every rank checks
    its own shard's lists and its own users; the flag is the AND over ranks."""
    import torch
    from influentialrs_amd._lib import IRS_SWEEP_F32
    eng = job.eng
    # (single GPU: the loop's calls carry their emission thresholds from step to step; eight more such steps first, every row
    #  that had to take the exhaustive path in them counted into `fallback_rows` -- a carried threshold that did not fit shows there)
    fb_carry = 0
    if not job.sharded and getattr(job, "carry", False):
        acc = torch.zeros((), dtype=torch.int64, device=job.device)
        for _ in range(8):
            job.step()
            acc += (job.last_status & 1).sum()
        fb_carry = int(acc.item())
    _, xr, _ = eng.decode(job.seqs, job.users, want_x=False, pos=job.hep)
    rows = xr
    if job.sharded:
        rows = eng.allgather_rows(job.comm, xr, job.x_all)
    v, i, st = eng.score_topk(rows, job.k, job.sweep, carry=(not job.sharded and getattr(job, "carry", False)))
    sel = torch.linspace(0, rows.shape[0] - 1, n, device=rows.device).long()
    vf, i_f, _ = eng.score_topk(rows[sel].contiguous(), job.k, IRS_SWEEP_F32)
    # the decoder that produced the rows (round 5): `n` of this rank's users decoded again, n per call in IRS_GEMM_F32 -- at
    # that size irs_decode takes the small-batch float32-chain kernels (d = 256: k_block_small_wide + the float32 attention),
    # the ones tests/test_gpu_decoder_path.py pins to the reference's irn_c2 / irn_c3 / irn_c4d goldens user by user
    from influentialrs_amd._lib import IRS_GEMM_F32
    sel_d = torch.linspace(0, job.B - 1, min(n, job.B), device=rows.device).long()
    mode = eng.decoder_gemm
    eng.decoder_gemm = IRS_GEMM_F32
    try:
        _, xr_s, _ = eng.decode(job.seqs[sel_d].contiguous(), job.users[sel_d].contiguous(), want_x=False, pos=job.hep[sel_d].contiguous())
        xr_s = xr_s.clone()
    finally:
        eng.decoder_gemm = mode
    torch.cuda.synchronize()
    row_err = float((xr[sel_d] - xr_s).abs().max().item())
    job.verify_row_diff = row_err
    ok = bool(torch.equal(i[sel], i_f) and torch.equal(v[sel].view(torch.int32), vf.view(torch.int32)) and row_err < VERIFY_ROW_TOL)
    if job.world > 1:
        import torch.distributed as dist
        t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=job.device)
        if dist.get_backend() == "gloo":
            h = t.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.MIN)
            ok = bool(h.item())
        else:
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            ok = bool(t.item())
    return ok, int((st & 1).sum().item()) + fb_carry


def verify_headline(job, n=8):
    """Self-check of the headline leg.  The windows are the ones the timed loop left behind; `n` sampled users' step is
    run twice: (a) inside the full batch through the call the loop ran (throughput kernels: packed rows, fused layer
    kernel in the engine's decoder arithmetic, packed-sequence attention, irs_score_topk), (b) `n` users per call on a
    second engine over the same weight tensors in IRS_GEMM_F32 -- at that size irs_decode takes the small-batch float32-MFMA
    kernels, the ones tests/test_gpu_decoder_path.py pins to the reference's goldens user by user.  Decoder rows must agree
    within 5e-5 (the bound tests/test_gpu_decoder_path.py holds for rows through the split-precision kernels; observed maxima
    over millions of values are 4.1e-5, typical samples 4e-6 .. 1.2e-5), top-100 values within 5e-5, top-100 ids position by
    position except inside runs of (b)'s scores closer than that same 5e-5 (two scores that each may move by the value
    tolerance can swap), and the greedy next item wherever (b)'s two best surviving scores are further apart."""
    TOL = 5e-5
    import torch
    from influentialrs_amd._lib import IRS_GEMM_F32, IRS_MASK_IRN
    from influentialrs_amd.engine import Engine
    cfg, eng, dev = job.cfg, job.eng, job.device
    B = job.B
    n = min(n, B)
    sel = torch.linspace(0, B - 1, n, device=dev).long()
    _, xr, _ = eng.decode(job.seqs, job.users, want_x=False, pos=job.hep)
    val, ids, _ = eng.score_topk(xr, job.k, job.sweep)
    small = Engine(n_item=cfg.n_item, n_user=cfg.n_user, d=cfg.emb_dim, max_len=cfg.max_len, n_heads=cfg.n_heads,
                   ffn_dim=cfg.ffn_dim, n_layers=cfg.n_layers, u_dim=cfg.u_emb_dim, mask_mode=IRS_MASK_IRN, device=dev,
                   max_rows=n, max_seqs=n, max_k=job.k)
    small.bind_state_dict(job.sd)
    small.decoder_gemm = IRS_GEMM_F32
    seq_s, usr_s, hep_s = job.seqs[sel].contiguous(), job.users[sel].contiguous(), job.hep[sel].contiguous()
    _, xr_s, _ = small.decode(seq_s, usr_s, want_x=False, pos=hep_s)
    val_s, ids_s, _ = small.score_topk(xr_s, job.k, job.sweep)
    # greedy next items: the path step of both engines on copies of the windows
    nxt = []
    for e, sq, hp, v, i in ((eng, job.seqs.clone(), job.hep.clone(), val, ids), (small, seq_s.clone(), hep_s.clone(), val_s, ids_s)):
        pth = torch.zeros((sq.shape[0], 1), dtype=torch.float32, device=dev)
        stt = torch.zeros(sq.shape[0], dtype=torch.int32, device=dev)
        e.path_step(sq, hp, v, i, 0, pth, stt)
        nxt.append(pth[:, 0])
    torch.cuda.synchronize()
    row_err = float((xr[sel] - xr_s).abs().max().item())
    val_err = float((val[sel] - val_s).abs().max().item())
    vs, ia, ib = val_s.cpu().numpy(), ids[sel].cpu().numpy(), ids_s.cpu().numpy()
    ids_ok = True
    for b in range(n):
        for j in np.nonzero(ia[b] != ib[b])[0]:
            if (np.abs(vs[b] - vs[b, j]) < TOL).sum() <= 1 and j != job.k - 1:
                ids_ok = False
    na, nb = nxt[0][sel].cpu().numpy(), nxt[1].cpu().numpy()
    next_ok = True
    for b in range(n):
        if na[b] == nb[b]:
            continue
        pa, pb = np.nonzero(ib[b] == int(na[b]) - 1)[0], np.nonzero(ib[b] == int(nb[b]) - 1)[0]
        if not (len(pa) and len(pb) and abs(float(vs[b][pa[0]]) - float(vs[b][pb[0]])) < TOL):  # not a near-tie of (b)'s scores
            next_ok = False
    ok = bool(row_err < TOL and val_err < TOL and ids_ok and next_ok)
    del small
    return ok, {"users_checked": n, "max_row_diff": row_err, "max_top100_value_diff": val_err, "ids_agree_outside_near_ties": ids_ok,
                "greedy_next_item_agrees": bool(next_ok)}


def phase_times(job, steps=3):
    """Rank-local time of each phase of a step (torch.cuda events on the current stream, which the engine and the
    collectives both order against): where an N-GPU step goes -- reported beside the c4_item_sharded leg so that a
    scaling run can be read without a profiler.  Not part of any timed region."""
    import torch
    names = ["decode", "gather_rows", "score_topk", "exchange_keys", "merge_and_path_step"]
    acc = dict.fromkeys(names, 0.0)
    eng = job.eng
    for _ in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record()
        _, xr, _ = eng.decode(job.seqs, job.users, want_x=False, pos=job.hep)
        ev[1].record()
        rows = eng.allgather_rows(job.comm, xr, job.x_all) if job.sharded else xr   # irs_allgather_rows
        ev[2].record()
        v, i, _ = eng.score_topk(rows, job.k, job.sweep, carry=(not job.sharded and getattr(job, "carry", False)))
        keys = eng.pack_topk(v, i).view(job.world, job.B, job.k) if job.sharded else None
        ev[3].record()
        if job.sharded:
            eng.exchange_topk(job.comm, keys, job.k_recv)                           # irs_exchange_topk
        ev[4].record()
        if job.sharded:
            v, i = eng.merge_topk_keys(job.k_recv)
        eng.path_step(job.seqs, job.hep, v, i, 0, job.paths, job.status)
        ev[5].record()
        torch.cuda.synchronize()
        for n, a, b in zip(names, ev[:-1], ev[1:]):
            acc[n] += a.elapsed_time(b)
    return {n: round(t / steps, 4) for n, t in acc.items()}


def timed(job, steps, world):
    import torch
    import torch.distributed as dist
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        job.step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=job.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt


DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs: all files of all ranks together


def step_outputs(job):
    """What the timed path handed its caller in its last step, as host arrays with one row per user: the consumed rows, the
    top-100 lists and their status (single GPU), the greedy next item, the path step's status and the windows it left."""
    import torch
    torch.cuda.synchronize()
    out = {}
    if job.last_out is not None:
        xr, val, ids = job.last_out
        out["rows"] = xr.cpu().numpy()
        out["topk_values"] = val.cpu().numpy()
        out["topk_ids"] = ids.cpu().numpy().astype(np.float64)
        out["topk_status"] = job.last_status.cpu().numpy().astype(np.float64)
    out["next_items"] = job.paths[:, 0].cpu().numpy()
    out["path_status"] = job.status.cpu().numpy().astype(np.float64)
    out["windows"] = job.seqs.cpu().numpy().astype(np.float64)
    out["history_end"] = job.hep.cpu().numpy().astype(np.float64)
    return out


def write_outputs(outdir, arrays, limit=DUMP_LIMIT_BYTES, suffix=""):
    """`arrays` (float32 / float64, one row per user) as outdir/<name><suffix>.npy.  Above `limit` bytes the same fixed, seeded
    sample of users is kept in every array, and their indices are written as `sampled_rows`."""
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
    n = {a.shape[0] for a in arrays.values()}
    assert len(n) == 1, {k: a.shape for k, a in arrays.items()}
    n = n.pop()
    per_row = sum(a.nbytes for a in arrays.values()) / max(n, 1)
    if per_row * n > limit:
        keep = max(1, int(limit // (per_row + 8)))
        idx = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
        arrays = {k: a[idx] for k, a in arrays.items()}
        arrays["sampled_rows"] = idx.astype(np.float64)
    os.makedirs(outdir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(outdir, f"{name}{suffix}.npy"), np.ascontiguousarray(a))
    return sorted(arrays)


def run_config(args, job, world, packed_fraction=None):
    """The `config` object of the result line."""
    from influentialrs_amd._lib import IRS_GEMM_H3, IRS_GEMM_X6
    cfg = job.cfg
    gemm_mode = job.eng.decoder_gemm_effective
    x6 = gemm_mode in (IRS_GEMM_X6, IRS_GEMM_H3)
    out_cfg = {"workload": f"{args.workload}: n_item={cfg.n_item}, d={cfg.emb_dim}, L={cfg.max_len}, H={cfg.n_heads}, "
                           f"layers={cfg.n_layers}, ffn={cfg.ffn_dim}; one greedy path-search step",
               "users_per_step": job.B * world, "users_per_gpu": job.B, "top_k": 100,
               "windows": "ml-1m-shaped history lengths (log-normal, median 95), pre-padded; decoder skips pad tokens "
                          "(packed rows), results identical",
               "packed_row_fraction": packed_fraction,
               "sweep": args.sweep + (" filter + exact f32 re-score" if args.sweep == "bf16" else ""),
               "decoder_gemm": (("h3: float32 operands split into two float16 planes (22 of 24 significand bits; weight planes pre-scaled by 2^8 out of the float16 subnormal range), three plane products per "
                                 "float32 product on v_mfma_f32_32x32x16_f16" if gemm_mode == IRS_GEMM_H3 else
                                 "x6: float32 operands split exactly into three bf16 planes, six plane products per float32 product on "
                                 "v_mfma_f32_32x32x16_bf16") + ", float32 accumulation (fused layer kernel and embed + layer-0 q|k|v); attention "
                                "and the last layer's rows on float32 MFMAs" if x6 else "float32 MFMAs"),
               "decoder_layers": ("sequence-resident (irs_set_decoder_seq mode %d): layers 0 .. n-2 and the last layer's attention in ONE launch on "
                                  "whole sequences per workgroup, K / V in LDS, x resident across layers" % job.eng.decoder_seq
                                  if job.eng.decoder_seq_last else "layer kernel + packed-sequence attention kernel per layer (irs_set_decoder_seq mode %d)" % job.eng.decoder_seq),
               "parallelism": "single GPU" if world == 1 else (
                   f"rows data-parallel + item-sharded x{world}: RCCL all-gather of rows, one all_to_all of packed 64-bit top-100 keys "
                   f"(irs_generate_paths_sharded: collectives below the C ABI, "
                   f"{'step replayed from a captured hipGraph' if SHARDED_GRAPH and job.comm is not None and job.comm.is_rccl else 'plain stream launches'})"
                   if job.sharded else
                   f"users partitioned over {world} GPUs, catalog replicated ({cfg.n_item} items): no data-path collective")}
    if packed_fraction is None:
        del out_cfg["packed_row_fraction"]
    return out_cfg


def headline(args, world, value, dt, out_cfg):
    """The fields every result line starts with (a plain run prints these alone)."""
    return {
        "metric": "scored user-item pairs/sec (whole node)",
        "value": value,
        "unit": "pairs/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": out_cfg,
    }


def scoring_legs(device, reps=10):
    """irs_score_topk and its emission sweep alone on the catalog-scale shapes ('also report the scoring
    kernel in isolation'; the north star's 60 % MFMA target is quoted on this kernel)."""
    import torch
    from influentialrs_amd import synth
    from influentialrs_amd._lib import IRS_MASK_IRN, IRS_PROF_NONE, IRS_PROF_SWEEP_EMIT, IRS_SWEEP_BF16
    from influentialrs_amd.engine import Engine
    out = {}
    for name, N, d in (("1Mx128", 1_000_000, 128), ("1.25Mx256", 1_250_000, 256)):
        nh = d // 32
        cfg = synth.make_config("tiny", n_item=N, emb_dim=d, n_heads=nh, n_layers=1, max_len=4, ffn_dim=8, n_user=2)
        eng = Engine(n_item=N, n_user=2, d=d, max_len=4, n_heads=nh, ffn_dim=8, n_layers=1, u_dim=10, mask_mode=IRS_MASK_IRN,
                     device=device, max_rows=1024, max_seqs=1)
        sd = gpu_state_dict(cfg, device, 1)
        eng.bind_state_dict(sd)
        g = torch.Generator(device=device)
        g.manual_seed(7)
        legs = {}
        for M in (1, 32, 1024):
            x = torch.randn((M, d), generator=g, device=device)
            for _ in range(2):
                eng.score_topk(x, 100, IRS_SWEEP_BF16)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                eng.score_topk(x, 100, IRS_SWEEP_BF16)
            torch.cuda.synchronize()
            total_us = (time.perf_counter() - t0) / reps * 1e6
            eng.prof_enable(IRS_PROF_SWEEP_EMIT)
            for _ in range(reps):
                eng.score_topk(x, 100, IRS_SWEEP_BF16)
            torch.cuda.synchronize()
            n, ms, fl, by = eng.prof_read()
            eng.prof_enable(IRS_PROF_NONE)
            sweep_us = ms / max(n, 1) * 1e3
            flops = 2.0 * d * M * N
            wbytes = N * d * 2.0
            leg = {"rows": M, "score_topk_us": total_us, "emit_sweep_us": sweep_us}
            if M >= 315:
                leg.update(bound="mfma", emit_sweep_tflops=flops / sweep_us / 1e6,
                           emit_sweep_frac_bf16_peak=flops / sweep_us / 1e6 / PEAK_BF16_TFLOPS,
                           score_topk_frac_bf16_peak=flops / total_us / 1e6 / PEAK_BF16_TFLOPS)
            else:
                leg.update(bound="hbm", w_stream_floor_us=wbytes / PEAK_HBM_GBS / 1e3,
                           emit_sweep_frac_hbm=wbytes / sweep_us / 1e3 / PEAK_HBM_GBS,
                           score_topk_frac_hbm=wbytes / total_us / 1e3 / PEAK_HBM_GBS)
            if M == 32:  # a beam-search step's scoring: candidates AND log-sum-exp out of one pass over the fp32 catalog
                for _ in range(2):
                    eng.score_topk_lse(x, 100, IRS_SWEEP_BF16)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    eng.score_topk_lse(x, 100, IRS_SWEEP_BF16)
                torch.cuda.synchronize()
                fused_us = (time.perf_counter() - t0) / reps * 1e6
                leg.update(score_topk_lse_us=fused_us, fp32_stream_floor_us=N * d * 4.0 / PEAK_HBM_GBS / 1e3,
                           score_topk_lse_frac_hbm=N * d * 4.0 / fused_us / 1e3 / PEAK_HBM_GBS)
            legs[f"M={M}"] = leg
        out[name] = legs
        del eng, sd
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="c2", choices=["c1", "c2", "c3", "c4", "default", "tiny"])
    ap.add_argument("--batch", type=int, default=4096, help="users per rank per step")
    ap.add_argument("--n-item", type=int, default=0, help="override the catalog size")
    ap.add_argument("--sweep", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--full", action="store_true", help="also run everything beside the headline (CPU baseline, instrumented "
                    "per-family pass and rooflines, self-check, latency, scoring, C3, C4 / C5 legs); a plain run sets up, warms up, "
                    "times --steps steps and prints the headline line only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the timed path returned in its last step as "
                    "DIR/<name>.npy (float32 / float64, at most 64 MB in all: a seeded sample of users beyond that)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--no-scoring", action="store_true", help="skip the catalog-scale scoring legs")
    ap.add_argument("--no-c4", action="store_true", help="skip the 10M-item item-sharded leg")
    ap.add_argument("--extras-timeout", type=int, default=420, help="seconds the legs behind the headline may take before the "
                    "line is printed without them")
    ap.add_argument("--no-c3", action="store_true", help="skip the 1M-item (BASELINE configs[2]) leg")
    ap.add_argument("--c3-batch", type=int, default=1024, help="users per rank per step of the c3 leg")
    ap.add_argument("--c3-steps", type=int, default=10)
    ap.add_argument("--pmc-run", action="store_true",
                    help="the command rocprofv3 --pmc / --kernel-trace wraps (tools/r04_measure.sh): warm-up + timed steps of the "
                         "headline workload only -- no CPU legs, no instrumented pass, no other legs -- and the packed row "
                         "count of exactly those steps as a JSON line on stdout")
    ap.add_argument("--c4-batch", type=int, default=0, help="users per step of the c4_item_sharded leg: per rank under --scaling "
                    "weak (default 1024), in total under --scaling strong (default 8192)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="N > 1: 'weak' = --batch / --c3-batch / --c4-batch users PER RANK (work grows with N); 'strong' = that many "
                         "users IN TOTAL, divided over the ranks (C4: 8192 users over the 10M-item catalog whatever N is; C5 is one "
                         "user's beam search either way)")
    ap.add_argument("--c4-steps", type=int, default=5)
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only to rehearse "
                    "the N > 1 code path with several ranks on ONE GPU)")
    ap.add_argument("--same-device", action="store_true", help="rehearsal: every rank uses cuda:0")
    ap.add_argument("--shard", default="auto", choices=["auto", "items", "replicate"],
                    help="N > 1: 'items' = every rank holds a slice of the catalog (rows all-gathered, per-shard top-k "
                         "exchanged, merged); 'replicate' = every rank holds the whole catalog and scores its own users, no "
                         "data-path collective; 'auto' = items from 262144 catalog entries up (a 3415-item catalog is 1.7 MB)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit("launch with torch.distributed.run --nproc-per-node N for --gpus N")

    # the CPU legs run first: they fork worker processes, which must happen before this process touches the GPU
    if args.pmc_run:
        args.no_cpu_baseline = args.no_latency = args.no_scoring = args.no_c4 = args.no_c3 = True
    cpu = None
    if args.full and not args.no_cpu_baseline and world == 1 and rank == 0:
        cpu = cpu_baseline(args.workload if args.workload in ("c1", "c2", "default", "tiny") else "c2")

    import torch
    import torch.distributed as dist
    from influentialrs_amd._lib import (IRS_GEMM_H3, IRS_GEMM_X6, IRS_PROF_ATTN, IRS_PROF_LAYER, IRS_PROF_LINEAR, IRS_PROF_NONE, IRS_PROF_REFINE,
                                        IRS_PROF_SWEEP, IRS_SWEEP_BF16)
    device = torch.device("cuda", 0 if args.same_device else local_rank)
    torch.cuda.set_device(device)
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(args.backend)

    strong = args.scaling == "strong"
    if not args.c4_batch:
        args.c4_batch = 8192 if strong else 1024
    if strong:
        for nm in ("batch", "c3_batch", "c4_batch"):
            tot = getattr(args, nm)
            if tot % world:
                sys.exit(f"--scaling strong: --{nm.replace('_', '-')} {tot} is not divisible by {world} ranks")
            setattr(args, nm, tot // world)
    job = Job(args.workload, args.batch, rank, world, device, args.shard, args.sweep, args.n_item)
    cfg = job.cfg
    if args.pmc_run:
        # every step's packed row count (a window gains one token per step until it is full): the rows the decoder
        # kernels of THIS process executed, launch by launch -- what a --pmc pass's byte counts are compared with
        fr = []
        for _ in range(args.warmup + args.steps):
            fr.append(packed_fraction(job))
            job.step()
        torch.cuda.synchronize()
        rows = [f * job.B * cfg.max_len for f in fr]
        print(json.dumps({"pmc_run": True, "workload": args.workload, "users": job.B, "steps": len(rows),
                          "packed_rows_per_step": rows, "packed_rows_mean": float(np.mean(rows))}), flush=True)
        return
    for _ in range(args.warmup):
        job.step()
    # the windows as the timed region finds them: every instrumented pass below restarts from this state, so that it
    # executes exactly the timed region's work (a window gains a token per step until it is full: 20 steps later the
    # decoder would run ~10 % more packed rows)
    snap = (job.seqs.clone(), job.hep.clone()) if args.full else None
    dt = timed(job, args.steps, world)
    users_total = job.B * world
    value = users_total * cfg.n_item * args.steps / dt
    if args.dump_outputs:
        write_outputs(args.dump_outputs, step_outputs(job), limit=DUMP_LIMIT_BYTES // world,
                      suffix=f"_rank{rank}" if world > 1 else "")
    if not args.full:
        if rank == 0:
            print(json.dumps(headline(args, world, value, dt, run_config(args, job, world))), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # second, instrumented pass: HIP events around every launch of each kernel family
    fam = {}
    # ("layer" is the fused layer kernel alone, a subset of "linear": the kernel the decoder roofline is quoted on)
    for name, f in (("linear", IRS_PROF_LINEAR), ("attn", IRS_PROF_ATTN), ("sweep", IRS_PROF_SWEEP), ("refine", IRS_PROF_REFINE),
                    ("layer", IRS_PROF_LAYER)):
        job.seqs.copy_(snap[0])
        job.hep.copy_(snap[1])
        job.eng.prof_enable(f)
        f0 = packed_fraction(job)
        for _ in range(args.steps):
            job.step()
        torch.cuda.synchronize()
        f1 = packed_fraction(job)
        n, ms, fl, by = job.eng.prof_read()
        # decoder kernels run on the packed (non-pad) rows: executed flops = dense-shape flops x packed fraction
        scale = 0.5 * (f0 + f1) if name in ("linear", "attn", "layer") else 1.0
        fam[name] = dict(launches=n, ms=ms, flops=fl * scale, bytes=by, packed_fraction=scale)
    job.eng.prof_enable(IRS_PROF_NONE)
    # self-check of the headline: sampled users of the last step against the golden-pinned small-batch float32 kernels
    try:
        head_ok, head_how = verify_headline(job)
    except Exception as e:  # noqa: BLE001 -- reported, never hidden: verified stays false
        head_ok, head_how = False, {"error": f"{type(e).__name__}: {e}"}
    if world > 1:  # the flag is the AND over ranks; a failing rank's own findings travel with it
        box = [None] * world
        dist.all_gather_object(box, (bool(head_ok), head_how))
        head_ok = all(ok_ for ok_, _ in box)
        bad = {str(r_): how_ for r_, (ok_, how_) in enumerate(box) if not ok_}
        if bad:
            head_how = dict(head_how, failed_ranks=bad)
    layer = fam.pop("layer")
    gemm_mode = job.eng.decoder_gemm_effective
    x6 = gemm_mode in (IRS_GEMM_X6, IRS_GEMM_H3)  # a split-precision mode of the fused layer kernel
    nprod = 3.0 if gemm_mode == IRS_GEMM_H3 else 6.0  # matrix instructions' products per float32 product

    roof = None
    if rank == 0:
        # The instrumented pass brackets every launch with HIP events, which costs time of its own (round 2: families
        # summed to 8.96 ms against a 7.86 ms step).  The timed region is the truth: every family's time is scaled by
        # the same factor so that the families sum to no more than the un-instrumented step (the kernels outside the
        # four families -- embedding, plan, path step -- then count as zero: the scaled times are upper bounds, the
        # achieved rate a lower bound).
        ms_step = dt / args.steps * 1e3
        fam_sum = sum(v["ms"] for v in fam.values()) / args.steps
        fscale = min(1.0, ms_step / fam_sum) if fam_sum > 0 else 1.0
        for v in fam.values():
            v["ms_instrumented"] = v["ms"]
            v["ms"] = v["ms"] * fscale
        assert sum(v["ms"] for v in fam.values()) / args.steps <= 1.02 * ms_step
        dom = max(fam, key=lambda k: fam[k]["ms"])
        f = fam[dom]
        per_launch_ms = f["ms"] / max(f["launches"], 1)
        if dom == "linear" and layer["launches"] > 0:
            # the family's dominant KERNEL: the fused layer kernel (5 of the 8 launches of a C2 step, ~80 % of the
            # family's time).  Flops are the algorithmic ones (2 per float32 multiply-add of the dense shapes, x the packed
            # row fraction).  IRS_GEMM_X6 executes SIX bf16 MFMA products per float32 product, IRS_GEMM_H3 THREE float16 ones
            # (the same instruction rate), so the peak that bounds the kernel is the dense 16-bit MFMA peak / 6 resp. / 3;
            # IRS_GEMM_F32 is bounded by the float32-MFMA peak.
            layer["ms_instrumented"] = layer["ms"]
            layer["ms"] = layer["ms"] * fscale
            f = layer
            per_launch_ms = f["ms"] / max(f["launches"], 1)
            ach = f["flops"] / (f["ms"] * 1e-3) / 1e12 if f["ms"] > 0 else 0.0
            peak = PEAK_BF16_TFLOPS / nprod if x6 else PEAK_F32_MATRIX_TFLOPS
            roof = {"kernel": ("k_block_x6 (fused decoder layer: out-projection, layer norms, feed-forward, next q|k|v; "
                               + ("split-float16 MFMA, 3 f16 products per float32 product)" if gemm_mode == IRS_GEMM_H3 else
                                  "split-bf16 MFMA, 6 bf16 products per float32 product)") if x6 else
                               "k_block (fused decoder layer: out-projection, layer norms, feed-forward, next q|k|v; float32 MFMA)"),
                    "bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "traffic": None,
                    "peak_basis": ("dense 16-bit MFMA peak 2500 TFLOP/s / %d products" % int(nprod) if x6 else "float32 MFMA dense peak"),
                    "executed_mfma_tflops": ach * (nprod if x6 else 1.0),
                    "float32_equivalent_vs_f32_matrix_peak": ach / PEAK_F32_MATRIX_TFLOPS}
            # Which roof binds?  Per packed row the kernel's algorithmic HBM bytes are 6 d floats (in: attention output and
            # residual; out: x' and the next q | k | v).  With float16 planes the matrix floor (flops / (2500 / 3)) drops below
            # the HBM floor (bytes / 8 TB/s): the kernel is then an HBM-bound one by the roofline's own definition and the line
            # says so -- `achieved` = algorithmic bytes / launch time against the 8 TB/s peak -- with the matrix-side numbers kept
            # under `mfma_side`.
            rows_launch = fam[dom].get("packed_fraction", 1.0) * job.B * cfg.max_len
            nl_ = max(cfg.n_layers, 2)  # n_layers - 2 launches write q | k | v (6 d floats per row), the last one k | v only (5 d)
            alg_bytes = rows_launch * (6 * (nl_ - 2) + 5) / (nl_ - 1) * cfg.emb_dim * 4
            flops_launch = f["flops"] / max(f["launches"], 1)
            floor_hbm_ms = alg_bytes / (PEAK_HBM_GBS * 1e9) * 1e3
            floor_mfma_ms = flops_launch / (peak * 1e12) * 1e3
            roof["floor_ms"] = {"hbm": floor_hbm_ms, "mfma": floor_mfma_ms}
            # both roofs side by side, whatever `bound` says (round 5): algorithmic bytes resp. flops per launch / launch time / peak
            if per_launch_ms > 0:
                roof["frac_hbm"] = floor_hbm_ms / per_launch_ms
                roof["frac_mfma"] = floor_mfma_ms / per_launch_ms
            if floor_hbm_ms > floor_mfma_ms and per_launch_ms > 0:
                mfma_side = {k: roof[k] for k in ("achieved", "peak", "unit", "frac", "peak_basis", "executed_mfma_tflops",
                                                  "float32_equivalent_vs_f32_matrix_peak")}
                ach_gbs = alg_bytes / (per_launch_ms * 1e-3) / 1e9
                roof.update({"bound": "hbm", "achieved": ach_gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": ach_gbs / PEAK_HBM_GBS,
                             "peak_basis": "HBM3E 8 TB/s; algorithmic bytes = packed rows x 6 d x 4 B (5 d for the k | v-only launch)", "mfma_side": mfma_side})
                for k in ("executed_mfma_tflops", "float32_equivalent_vs_f32_matrix_peak"):
                    roof.pop(k, None)
        elif dom in ("linear", "attn"):
            ach = f["flops"] / (f["ms"] * 1e-3) / 1e12 if f["ms"] > 0 else 0.0
            roof = {"kernel": {"linear": "k_block + k_linear (decoder fp32 MFMA GEMM family: fused layer kernel, layer-0 QKV)",
                               "attn": "k_attn16 / k_attn_mfma (decoder self-attention, fp32 MFMA)"}[dom],
                    "bound": "mfma", "achieved": ach, "peak": PEAK_F32_MATRIX_TFLOPS, "unit": "TFLOP/s",
                    "frac": ach / PEAK_F32_MATRIX_TFLOPS, "traffic": None}
        else:
            if dom == "sweep" and users_total >= 315 and job.sweep == IRS_SWEEP_BF16:
                ach = f["flops"] / (f["ms"] * 1e-3) / 1e12 if f["ms"] > 0 else 0.0
                roof = {"kernel": "k_sweep_ring / k_sweep_bf16 (catalog sweep, bf16 MFMA)", "bound": "mfma", "achieved": ach,
                        "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_BF16_TFLOPS, "traffic": None}
            else:
                ach = f["bytes"] / (f["ms"] * 1e-3) / 1e9 if f["ms"] > 0 else 0.0
                roof = {"kernel": f"k_{dom}", "bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                        "frac": ach / PEAK_HBM_GBS, "traffic": None}
        # HBM traffic of the dominant kernel: PMC counters cannot be read from inside this process; the number is the
        # per-launch mean of the committed rocprofv3 passes of this same command (FETCH_SIZE doubled per the gfx950
        # note + WRITE_SIZE, separate --pmc passes), valid for the default workload only.  It is reported together with
        # the packed row count it was measured at; `algorithmic_bytes_per_launch` is quoted at that SAME row count.
        pmc_file = os.path.join(REPO, "profiles", "r05", "c2_b4096_pmc.json")
        if not os.path.exists(pmc_file):
            pmc_file = os.path.join(REPO, "profiles", "r04", "c2_b4096_pmc.json")
        pmc_rel = os.path.relpath(pmc_file, REPO)
        if dom == "linear" and world == 1 and args.workload == "c2" and args.batch == 4096 and not args.n_item and os.path.exists(pmc_file):
            try:
                with open(pmc_file) as fh:
                    pm = json.load(fh)
                kb = pm["kernels"]["k_block_x6" if x6 and "k_block_x6" in pm["kernels"] else "k_block"]
                roof["traffic"] = float(kb["hbm_bytes_per_launch"])
                roof["traffic_measured_at_packed_rows"] = float(pm["packed_rows_mean"])
                roof["traffic_source"] = (pmc_rel + " (tools/r05_measure.sh: `bench.py "
                                          "--pmc-run` under rocprofv3 --pmc, FETCH_SIZE and WRITE_SIZE in separate passes, "
                                          "2 x FETCH_SIZE + WRITE_SIZE per the gfx950 note): the fused layer kernel, at "
                                          "that run's own mean packed row count")
                roof["algorithmic_bytes_per_launch"] = float(kb["algorithmic_bytes_per_launch"])
                roof["mfma_busy_pmc"] = kb.get("mfma_busy")
                roof["packed_rows_this_run"] = fam[dom]["packed_fraction"] * job.B * cfg.max_len
            except Exception as e:  # a malformed profile file must not cost the bench line
                roof["traffic_source"] = f"{pmc_rel} unreadable: {e}"
        roof["flops_counted"] = "executed (dense-shape flops x packed non-pad row fraction %.3f)" % fam[dom].get("packed_fraction", 1.0)
        roof["time_basis"] = ("HIP events around every launch of the family (a second pass over the SAME K steps: the windows are "
                              "reset to their state at the start of the timed region), scaled by %.4f so that the four families "
                              "sum to no more than the un-instrumented ms_per_step" % fscale)
        roof["avg_launch_ms"] = per_launch_ms
        roof["launches_per_step"] = f["launches"] / args.steps
        roof["family_ms_per_step"] = {k: v["ms"] / args.steps for k, v in fam.items()}
        roof["family_ms_per_step_instrumented"] = {k: v["ms_instrumented"] / args.steps for k, v in fam.items()}

    # ---- the whole step against what its arithmetic and its compulsory bytes allow (round 5): algorithmic flops of ONE step on the
    # step's own windows, priced per pipe (split-precision GEMMs at the 16-bit dense peak / products per float32 product; attention
    # scores on the float32 matrix pipe; P.V and the bf16 catalog filter on the 16-bit pipe), and the bytes that MUST cross HBM
    # whatever the decomposition: the embedding rows in, the catalog once, the weights once, one row and one top-100 list per user
    # out.  Every q | k | v / attention-output / x round trip between the kernels is decomposition traffic and is NOT in the floor.
    step_roof = None
    kernels = None
    if rank == 0:
        d_, F_, L_, nl_ = cfg.emb_dim, cfg.ffn_dim, cfg.max_len, cfg.n_layers
        valid = (job.seqs != 0)
        valid[torch.arange(job.B, device=device), job.hep.long()] = True
        nseq = valid.sum(dim=1).double()
        tok = float(nseq.sum().item())
        sq_sum = float((nseq * nseq).sum().item())
        Bn = float(job.B)
        gemm_flops = tok * (nl_ - 1) * (8.0 * d_ * d_ + 4.0 * d_ * F_) - tok * 2.0 * d_ * d_ \
            + Bn * (8.0 * d_ * d_ + 4.0 * d_ * F_)                       # full layers (the last one's q for B rows only) + the last layer's B rows
        score_flops = (nl_ - 1) * sq_sum * d_ + 2.0 * tok * d_             # causal q.k: n^2 / 2 pairs x 2 d; last layer: one query per sequence
        pv_flops = score_flops
        sweep_flops = 2.0 * d_ * Bn * cfg.n_item
        gemm_peak = (PEAK_BF16_TFLOPS / nprod if x6 else PEAK_F32_MATRIX_TFLOPS) * 1e12
        # (the sequence-resident decoder computes its scores as three float16 plane products too: priced on the 16-bit pipe there)
        seq_ = bool(job.eng.decoder_seq_last)
        score_peak = (PEAK_BF16_TFLOPS / 3.0 if seq_ else PEAK_F32_MATRIX_TFLOPS) * 1e12
        floor_mfma_ms = (gemm_flops / gemm_peak + score_flops / score_peak + pv_flops / (PEAK_BF16_TFLOPS / 3.0 * 1e12)
                         + sweep_flops / (PEAK_BF16_TFLOPS * 1e12)) * 1e3
        w_bytes = (nl_ * (4.0 * d_ * d_ + 2.0 * d_ * F_) + L_ * d_) * 4.0
        comp_bytes = tok * d_ * 4.0 + job.eng.n_local * d_ * (2.0 + 4.0 * 100.0 / max(job.eng.n_local, 1)) + w_bytes + Bn * (d_ * 4.0 + 100.0 * 12.0)
        floor_hbm_ms = comp_bytes / (PEAK_HBM_GBS * 1e9) * 1e3
        ms_step_ = dt / args.steps * 1e3
        step_roof = {"packed_token_rows": tok, "algorithmic_gflop": {"decoder_gemms": gemm_flops / 1e9, "attention_scores": score_flops / 1e9,
                                                                       "attention_pv": pv_flops / 1e9, "catalog_sweep": sweep_flops / 1e9},
                     "compulsory_hbm_gb": comp_bytes / 1e9, "floor_ms_mfma": floor_mfma_ms, "floor_ms_hbm": floor_hbm_ms,
                     "ms_per_step": ms_step_, "ms_per_step_over_floor": ms_step_ / max(floor_mfma_ms, floor_hbm_ms),
                     "pricing": "GEMMs at %s, attention scores at %s, P.V at 2500 / 3, catalog sweep at 2500 TFLOP/s; "
                                "HBM 8 TB/s" % (("2500 / %d TFLOP/s" % int(nprod)) if x6 else "the float32 matrix peak",
                                                "2500 / 3 TFLOP/s (three float16 plane products)" if seq_ else "the float32 matrix peak %.1f TFLOP/s" % PEAK_F32_MATRIX_TFLOPS)}
        if job.eng.decoder_seq_last and layer["launches"] > 0:
            # the sequence-resident decoder: ONE launch per step holds layers 0 .. n - 2 AND the attention (and the last layer's
            # q | k | v + attention for the consumed tokens); it is the dominant kernel, and what bounds it is the matrix side --
            # its arithmetic priced on the 16-bit pipe at 3 products per float32 product (GEMMs, attention scores, P.V) against its
            # launch time; the bytes it MUST move are the embedded rows in and x of the last fused
            # layer out (its attention tiles and x' round trips are scratch traffic of this decomposition, counted by `traffic`).
            lt_ms = layer["ms"] / max(layer["launches"], 1)
            dec_floor_ms = (gemm_flops / gemm_peak + score_flops / score_peak + pv_flops / (PEAK_BF16_TFLOPS / 3.0 * 1e12)) * 1e3
            alg_b = tok * d_ * 4.0 * 2.0
            roof = {"kernel": "k_block_x6<.., SEQ> (sequence-resident decoder: layers 0 .. n-2 with their attention, and the last layer's "
                              "q|k|v + attention of the consumed tokens, in ONE launch; GEMMs, attention scores and P.V all on exact split-float16 MFMA products)",
                    "bound": "mfma", "achieved": (gemm_flops + score_flops + pv_flops) / (lt_ms * 1e-3) / 1e12, "peak": PEAK_BF16_TFLOPS / nprod,
                    "unit": "TFLOP/s", "frac": dec_floor_ms / lt_ms, "frac_mfma": dec_floor_ms / lt_ms,
                    "frac_hbm": alg_b / (lt_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, "traffic": None,
                    "peak_basis": "frac = (GEMM + attention-score + P.V flops) / (2500 / 3 TFLOP/s) / launch time: every float32 product is three float16 "
                                  "plane products on the 16-bit dense peak; `achieved` = all float32-equivalent flops / time",
                    "floor_ms": {"mfma": dec_floor_ms, "hbm": alg_b / (PEAK_HBM_GBS * 1e9) * 1e3},
                    "avg_launch_ms": lt_ms, "launches_per_step": layer["launches"] / args.steps,
                    "family_ms_per_step": (roof or {}).get("family_ms_per_step"),
                    "flops_counted": "executed on the step's own windows (packed non-pad tokens; causal attention pairs)",
                    "time_basis": (roof or {}).get("time_basis")}
        # per-kernel numbers of the committed PMC passes of this same command (tools/r05_measure.sh -> tools/r05_pmc.py)
        pmc5 = os.path.join(REPO, "profiles", "r05", "c2_b4096_pmc.json")
        if world == 1 and args.workload == "c2" and args.batch == 4096 and not args.n_item and os.path.exists(pmc5):
            try:
                with open(pmc5) as fh:
                    pm5 = json.load(fh)
                kernels = [{"kernel": lab, "launches_per_step": k_.get("launches_per_step"), "us": k_["median_us"], "mfma_busy": k_.get("mfma_busy"),
                            "hbm_gb": k_["hbm_bytes_per_launch"] / 1e9, "algorithmic_gb": k_["algorithmic_bytes_per_launch"] / 1e9,
                            "algorithmic_gbs": k_.get("algorithmic_gbs"), "frac_hbm": k_.get("frac_hbm_peak")}
                           for lab, k_ in pm5["kernels"].items() if lab != "k_block_x6"]
                step_roof["decoder_hbm_gb_per_step_pmc"] = pm5.get("decoder_hbm_bytes_per_step", 0.0) / 1e9
                if job.eng.decoder_seq_last and "seq_decoder" in pm5["kernels"]:
                    ks_ = pm5["kernels"]["seq_decoder"]
                    roof["traffic"] = float(ks_["hbm_bytes_per_launch"])
                    roof["traffic_measured_at_packed_rows"] = float(pm5["packed_rows_mean"])
                    roof["mfma_busy_pmc"] = ks_.get("mfma_busy")
                    roof["traffic_source"] = "profiles/r05/c2_b4096_pmc.json (tools/r05_measure.sh: separate --pmc passes of `bench.py --pmc-run`, 2 x FETCH_SIZE + WRITE_SIZE)"
                step_roof["pmc_source"] = "profiles/r05/c2_b4096_pmc.json at %d packed rows" % int(pm5["packed_rows_mean"])
            except Exception as e:  # noqa: BLE001
                kernels = [{"error": f"profiles/r05/c2_b4096_pmc.json unreadable: {e}"}]

    lat = lat128 = lat1024 = lat_tokens = None
    if rank == 0 and not args.no_latency and world == 1:
        # path-gen p50: one user, 20 greedy steps through irs_generate_paths, stream launches (as the front-end
        # calls it), on the user whose window holds the median number of items of this workload (a window's length
        # sets the decoder's row count, i.e. the latency); fresh windows of the workload's shape (job.seqs has been
        # advanced by every step above: by now those windows are full)
        fresh = gpu_windows(job.B, cfg.max_len, cfg.n_item, device, seed=100 + rank)
        nvalid = (fresh != 0).sum(dim=1)
        iu = int(torch.argsort(nvalid)[nvalid.numel() // 2].item())
        lat_tokens = int(nvalid[iu].item())

        def p50(ss, uu, hh, pp, stt, warm, reps):
            ts = []
            ss0, hh0 = ss.clone(), hh.clone()
            for it in range(warm + reps):
                ss.copy_(ss0)  # every repetition starts from the user's own window (a path search appends its
                hh.copy_(hh0)  # 20 items to the window it is given: without the reset the windows fill up)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                job.eng.generate_paths(ss, uu, hh, 20, k=100, sweep=job.sweep, use_graph=False, paths=pp, status=stt)
                torch.cuda.synchronize()
                if it >= warm:
                    ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts))

        lat = p50(fresh[iu:iu + 1].clone(), job.users[iu:iu + 1].clone(), job.hep[iu:iu + 1].clone(),
                  torch.zeros((1, 20), dtype=torch.float32, device=device), torch.zeros(1, dtype=torch.int32, device=device),
                  20, 200)  # >= 200 repetitions after 20 warm-ups

        def per_user(nb, warm, reps):
            return p50(fresh[:nb].clone(), job.users[:nb].clone(), job.hep[:nb].clone(),
                       torch.zeros((nb, 20), dtype=torch.float32, device=device),
                       torch.zeros(nb, dtype=torch.int32, device=device), warm, reps) / nb

        lat128 = per_user(min(128, job.B), 5, 30)
        lat1024 = per_user(min(1024, job.B), 3, 10)

    out_cfg = run_config(args, job, world, fam["linear"]["packed_fraction"])
    del job
    torch.cuda.empty_cache()

    # ---- the extra legs (scoring, C3, C4, C5).  The headline above is complete at this point: whatever happens below -- an
    #      exception on some rank, a collective that never returns on a node this build has not seen -- the line is still
    #      printed, with "extras_error" saying which leg did not finish.
    X = {"scoring": None, "c3": None, "c4": None, "stage": None, "err": None}

    emit_lock = threading.Lock()
    emitted = [False]

    def emit():
        with emit_lock:  # the watchdog thread and the main thread may both get here: ONE line
            if emitted[0]:
                return
            emitted[0] = True
        if rank != 0:
            return
        out = headline(args, world, value, dt, out_cfg)
        out.update({
            "verified": head_ok,
            "verified_how": dict(head_how, what="a comparison INSIDE this library (no oracle, no reference on the GPU box): sampled users of "
                                 "the timed loop's last windows, full-batch throughput kernels vs the same users 8 per call on the "
                                 "float32-MFMA small-batch kernels: rows < 5e-5, top-100 values < 5e-5, ids equal outside near-ties < 5e-5, same "
                                 "greedy item.  It is sound because tests/test_gpu_throughput_goldens.py and tests/test_gpu_decoder_path.py pin "
                                 "BOTH sides to the unmodified reference's goldens (irn_c2, irn_c3, irn_c4d)"),
            "path_gen_p50_ms_b1": lat,
            "path_gen_b1_window_tokens": lat_tokens,
            "path_gen_ms_per_user_b128": lat128,
            "path_gen_ms_per_user_b1024": lat1024,
            "roofline": roof,
            "step_roofline": step_roof,
            "kernels": kernels,
            "scoring": X["scoring"],
            "c3_1M_items": X["c3"],
            "c4_item_sharded": X["c4"],
            # what an N = 1 vs N = 8 comparison should read: BASELINE configs[3], the 10M-item catalog cut into N item shards
            # (the C2 headline above replicates its 1.7 MB catalog: its N-GPU value scales trivially)
            "scale_metric": (None if X["c4"] is None else
                             {k: X["c4"].get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "ms_per_step", "scaling",
                                                          "users_per_gpu", "items_per_gpu", "workload", "parallelism", "verified",
                                                          "verified_how", "fallback_rows", "phase_ms_rank0")}),
            "cpu_baseline": cpu,
        })
        if X["err"]:
            out["extras_error"] = X["err"]
        flat = {}
        if roof:
            fm = roof.get("family_ms_per_step") or {}
            flat.update(layer_frac_hbm=roof.get("frac_hbm"), layer_frac_mfma=roof.get("frac_mfma"), layer_launch_ms=roof.get("avg_launch_ms"),
                        linear_ms_per_step=fm.get("linear"), attn_ms_per_step=fm.get("attn"), sweep_ms_per_step=fm.get("sweep"),
                        refine_ms_per_step=fm.get("refine"))
        if step_roof:
            flat.update(step_floor_ms_mfma=step_roof["floor_ms_mfma"], step_floor_ms_hbm=step_roof["floor_ms_hbm"],
                        step_ms_over_floor=step_roof["ms_per_step_over_floor"], decoder_hbm_gb_per_step_pmc=step_roof.get("decoder_hbm_gb_per_step_pmc"))
        for k_ in (kernels or []):
            if k_.get("kernel") == "embed_qkv0":
                flat["k1_embed_gather_algorithmic_gbs"] = k_.get("algorithmic_gbs")
                flat["k1_embed_gather_us"] = k_.get("us")
        sc_ = X["scoring"] or {}
        for shape, tag in (("1Mx128", "1Mx128"), ("1.25Mx256", "1p25Mx256")):
            leg = sc_.get(shape) or {}
            m1024, m32 = leg.get("M=1024") or {}, leg.get("M=32") or {}
            flat[f"emit_sweep_frac_bf16_peak_{tag}"] = m1024.get("emit_sweep_frac_bf16_peak")
            flat[f"score_topk_frac_bf16_peak_{tag}"] = m1024.get("score_topk_frac_bf16_peak")
            flat[f"score_topk_frac_hbm_m32_{tag}"] = m32.get("score_topk_frac_hbm")
        if X["c3"]:
            flat["c3_ms_per_step"] = X["c3"]["ms_per_step"]
        if X["c4"]:
            flat["c4_ms_per_step"] = X["c4"]["ms_per_step"]
            ph_ = X["c4"].get("phase_ms_rank0") or {}
            flat["c4_decode_ms"], flat["c4_score_topk_ms"] = ph_.get("decode"), ph_.get("score_topk")
            c5_ = X["c4"].get("c5_beam32") or {}
            flat["c5_step_p50_ms"] = c5_.get("step_p50_ms_stream")
        out.update({k_: v_ for k_, v_ in flat.items() if v_ is not None})
        print(json.dumps(out), flush=True)

    def watchdog():
        # the headline line is still printed, but the process reports FAILURE (a hung collective or leg must not read as
        # success to torchrun or to a `|| exit 1` chain); non-zero ranks leave the same way
        if not X["err"]:
            X["err"] = f"extra legs did not finish within {args.extras_timeout} s (stage: {X['stage']})"
        emit()
        sys.stdout.flush()
        os._exit(3)

    wd = threading.Timer(args.extras_timeout, watchdog)
    wd.daemon = True
    wd.start()
    try:
        X["stage"] = "scoring"
        if rank == 0 and world == 1 and not args.no_scoring:
            X["scoring"] = scoring_legs(device)

        # ---- BASELINE configs[2]: the 1M-item / d = 128 catalog (item-sharded when N > 1), 1024 users per rank per step
        X["stage"] = "c3"
        if not args.no_c3:
            j3 = Job("c3", args.c3_batch, rank, world, device, "items", args.sweep)
            for _ in range(2):
                j3.step()
            dt3 = timed(j3, args.c3_steps, world)
            u3 = j3.B * world
            ok3, fb3 = verify_job(j3)
            X["c3"] = {"metric": "scored user-item pairs/sec (whole node)", "value": u3 * j3.cfg.n_item * args.c3_steps / dt3,
                  "unit": "pairs/s", "n_gpus": world, "steps": args.c3_steps, "ms_per_step": dt3 / args.c3_steps * 1e3,
                  "scaling": args.scaling, "users_per_gpu": j3.B, "items_per_gpu": j3.eng.n_local,
                  "workload": f"c3: n_item={j3.cfg.n_item}, d={j3.cfg.emb_dim}, L={j3.cfg.max_len}, H={j3.cfg.n_heads}; one greedy "
                              f"path-search step, top-100",
                  "verified": ok3, "verified_how": VERIFY_JOB_HOW, "max_row_diff": getattr(j3, "verify_row_diff", None),
                  "fallback_rows": fb3, "phase_ms_rank0": phase_times(j3)}
            del j3
            torch.cuda.empty_cache()

        # ---- BASELINE configs[3]: the 10M-item catalog, item-sharded over the N GPUs (N = 1: the whole catalog, the anchor)
        X["stage"] = "c4"
        if not args.no_c4:
            j4 = Job("c4", args.c4_batch, rank, world, device, "items", args.sweep)
            for _ in range(2):
                j4.step()
            dt4 = timed(j4, args.c4_steps, world)
            u4 = j4.B * world
            ok4, fb4 = verify_job(j4)
            c4 = {"metric": "scored user-item pairs/sec (whole node)", "value": u4 * j4.cfg.n_item * args.c4_steps / dt4,
                  "unit": "pairs/s", "n_gpus": world, "steps": args.c4_steps, "ms_per_step": dt4 / args.c4_steps * 1e3,
                  "scaling": args.scaling, "users_per_gpu": j4.B, "items_per_gpu": j4.eng.n_local,
                  "workload": f"c4: n_item={j4.cfg.n_item}, d={j4.cfg.emb_dim}, L={j4.cfg.max_len}, H={j4.cfg.n_heads}; one greedy "
                              f"path-search step, top-100",
                  "parallelism": "single GPU holds the whole catalog" if world == 1 else
                                 f"item shards of {j4.eng.n_local} rows x {world}; per step: all-gather of {u4} x {j4.cfg.emb_dim} f32 rows, "
                                 f"one all_to_all of {u4} x 100 packed 64-bit keys per rank, merge"}
            c4["verified"] = ok4
            c4["verified_how"] = VERIFY_JOB_HOW
            c4["max_row_diff"] = getattr(j4, "verify_row_diff", None)
            c4["fallback_rows"] = fb4
            ph = phase_times(j4)  # every rank runs it (the collectives inside need all of them); rank 0 reports
            c4["phase_ms_rank0"] = ph
            X["c4"] = c4
            X["stage"] = "c5"
            if not args.no_latency:
                # BASELINE configs[4] (C5), D1 (ii): beam-width-32 persuasion-path search over the 10M-item catalog for ONE
                # user -- 32 windows decoded, scored (top-100 + exact log-sum-exp over the catalog) and re-ranked per step,
                # 20 steps; p50 over 10 repetitions after 2 warm-ups, stream launches and the captured two-step hipGraph.
                # N > 1: the SAME user on every rank (seeded windows), the 32 beam windows' decode split 32 / N per rank, rows
                # all-gathered, every rank sweeps its item shard for all 32 rows, packed lists all-gathered and merged,
                # log-sum-exp all-reduced, beam step replicated (irs_beam_search_sharded, split_decode); max over ranks.
                fresh = gpu_windows(4, j4.cfg.max_len, j4.cfg.n_item, device, seed=7)
                g5 = torch.Generator(device=device)
                g5.manual_seed(5)
                b_seq, b_hep = fresh[:1].contiguous(), j4.hep[:1].contiguous()
                b_usr = torch.randint(0, j4.cfg.n_user, (1,), generator=g5, device=device, dtype=torch.int64)
                c5 = {"window_tokens": int((b_seq != 0).sum().item()),
                      "workload": "c5: beam 32 x 20 steps, 1 user, n_item=10000000, d=256 (" +
                                  ("one GPU holds the whole catalog)" if world == 1 else
                                   f"{world} item shards of {j4.eng.n_local} rows; beam windows decoded {32 // world} per rank)"),
                      "n_gpus": world,
                      "beam_oracle": "build-defined, no reference counterpart (the reference has no beam search: beam > 1 is pinned by "
                                     "this repo's CPU statement oracle_np.beam_search only; beam = 1 equals the reference's greedy paths)"}
                for label, graph in (("stream", False), ("hipgraph", True)):
                    if graph and world > 1 and not SHARDED_GRAPH:
                        continue
                    ts = []
                    for it in range(12):
                        if world > 1:
                            dist.barrier()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        if world == 1:
                            j4.eng.beam_search(b_seq, b_usr, b_hep, 20, 32, k=100, sweep=j4.sweep, use_graph=graph)
                        else:
                            j4.eng.beam_search_sharded(j4.comm, b_seq, b_usr, b_hep, 20, 32, k=100, sweep=j4.sweep, split_decode=True,
                                                       use_graph=graph)
                        torch.cuda.synchronize()
                        dt5 = time.perf_counter() - t0
                        if world > 1:
                            t5 = torch.tensor([dt5], dtype=torch.float64, device=device)
                            if dist.get_backend() == "gloo":
                                h5 = t5.cpu()
                                dist.all_reduce(h5, op=dist.ReduceOp.MAX)
                                dt5 = float(h5.item())
                            else:
                                dist.all_reduce(t5, op=dist.ReduceOp.MAX)
                                dt5 = float(t5.item())
                        if it >= 2:
                            ts.append(dt5 * 1e3)
                    c5[f"search_p50_ms_{label}"] = float(np.median(ts))
                    c5[f"step_p50_ms_{label}"] = float(np.median(ts)) / 20
                # HBM floor of a step per GPU: its share of the fp32 catalog once (candidates + exact log-sum-exp out of one
                # pass) + the 1/8 sample of the bf16 catalog the threshold comes from
                c5["step_hbm_floor_ms"] = (j4.eng.n_local * j4.cfg.emb_dim * (4.0 + 2.0 / 8)) / (PEAK_HBM_GBS * 1e9) * 1e3
                X["c4"] = dict(c4, c5_beam32=c5)
                c4 = X["c4"]
            del j4
            torch.cuda.empty_cache()

    except Exception as e:  # noqa: BLE001 -- the headline must survive a failing extra leg
        X["err"] = f"{X['stage']}: {type(e).__name__}: {e}"
        print("bench.py: extra leg failed: " + X["err"], file=sys.stderr, flush=True)
    emit()
    unverified = [nm for nm, ok_ in (("headline", head_ok), ("c3", (X["c3"] or {}).get("verified", True)),
                                     ("c4", (X["c4"] or {}).get("verified", True))) if ok_ is False]
    if unverified and not X["err"]:
        # a failed self-check must not read as success to a `|| exit 1` chain (the line above still carries the numbers)
        print("bench.py: self-check failed (verified = false): " + ", ".join(unverified), file=sys.stderr, flush=True)
        sys.stdout.flush()
        os._exit(4)
    if X["err"]:
        sys.stdout.flush()
        os._exit(3)  # (N > 1: the other ranks may sit in a collective of the failed leg; their own watchdogs end them, non-zero too)
    if world > 1:
        X["stage"] = "final barrier"   # the watchdog stays armed: a peer that left through os._exit would block this forever
        dist.barrier()
        dist.destroy_process_group()
    wd.cancel()


if __name__ == "__main__":
    main()
