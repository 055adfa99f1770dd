"""The plan in front of the sequence-resident launch and the absorbed attention behind it.

The plan is three dependent launches: k_plan_count (valid tokens per sequence, r_u by k_pif's expression), k_plan_seq (thread 0
works the whole plan out on counts, every thread owns workgroups that pull their sequences, no barrier in the class loop; it
leaves one word per sequence) and k_plan_fill (every workgroup sums the counts in front of its own four sequences: no scan
launch; its wave of sequence b also writes that sequence's lines of the launch's tables).  What that can break, and where it would show:
  * a per-workgroup base that is wrong past some chunk: batches of 515 (no multiple of 4) and 1030 (past 1024) sequences, every
    table against NumPy -- counts, offsets, packed consumed rows, and r_u bitwise against irs_pif;
  * the pull placement: every block of every sequence exactly once, one workgroup per sequence, -1 behind the workgroups in
    use, the sequence's first image row, the tile-order consumed row, and the counts of full and half-live workgroups against
    the host replica of the rule (test_gpu_seq_tail_plan.expected_plan) -- on bench-shaped windows, a ramp of 1 .. 200 tokens,
    only 1-token windows (16 sequences per workgroup), only 200-token windows (one per workgroup) and a mix of consumed positions;
  * the route without k_plan_seq (decoder_seq = 0) gets the same counts, offsets and consumed rows from the same two kernels.
The absorbed attention (k_absorb_attn) walks a sequence's x' blocks 0 .. ib, then the target's block: windows of 4 .. 13 blocks on
each side of every block edge, consumed at L - 2 and at a middle token (the target's block is then fetched out of order), with a
target and without one: five calls give the same bits, rows within 5e-5 of the two-kernel route (the bound both routes hold
against the reference in tests/test_gpu_decoder_path.py), equal NaN patterns.

The only geometry the launch supports: d = 128, 4 heads, F = 256, L = 200; n_item = 300, 2 layers."""
import functools

import numpy as np
import pytest
import torch

import bench
from gpu_util import make_engine
from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_GEMM_H3
from test_gpu_seq_tail_plan import expected_plan
from test_gpu_throughput_goldens import X_TOL

pytestmark = pytest.mark.gpu

C = 16
B_PLAN = (515, 1030)
KINDS = ("bench", "ramp", "ones", "full", "positions")
X_TOL_ROW = 5e-5
CALLS = 5
B_RING = 192
RING_LENGTHS = [64, 65, 80, 81, 96, 97, 112, 113, 128, 129, 144, 145, 160, 161, 176, 177, 192, 193, 199, 200]


@functools.lru_cache(maxsize=None)
def _rig():
    cfg = synth.make_config("c2", n_item=300, n_layers=2)
    assert (cfg.emb_dim, cfg.n_heads, cfg.ffn_dim, cfg.max_len) == (128, 4, 256, 200)
    eng = make_engine(cfg, synth.irn_state_dict(cfg, 31), max_rows=max(B_PLAN), max_seqs=max(B_PLAN))
    eng.decoder_gemm = IRS_GEMM_H3
    return cfg, eng, torch.cuda.get_device_properties(0).multi_processor_count


def _plan_batch(cfg, B, kind):
    """(windows, consumed positions) of one plan case, pre-padded with the target last"""
    dev, L = torch.device("cuda:0"), cfg.max_len
    if kind == "bench":
        return bench.gpu_windows(B, L, cfg.n_item, dev, seed=11), torch.full((B,), L - 2, dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev).manual_seed(B)
    full = torch.randint(1, cfg.n_item + 1, (B, L), device=dev, generator=g)
    i = torch.arange(B, device=dev)
    n = {"ramp": 1 + i % L, "ones": torch.ones_like(i), "full": torch.full_like(i, L), "positions": 1 + (7 * i) % L}[kind]
    col = torch.arange(L, device=dev)[None, :]
    seqs = torch.where(col >= L - n[:, None], full, torch.zeros_like(full))
    pos = torch.full((B,), L - 2, dtype=torch.int64, device=dev)
    if kind == "positions":  # L - 2, the target, the first valid token, a pad in front of the history
        first = L - n
        pad = torch.where(n < L, first - 1, torch.full_like(n, L - 2))
        pos = torch.stack([pos, torch.full_like(pos, L - 1), first, pad])[i % 4, i]
    return seqs, pos.to(torch.int32)


@functools.lru_cache(maxsize=None)
def _plan_case(B, kind):
    """one decode by each route and what the plan kernels left behind"""
    cfg, eng, n_cu = _rig()
    seqs, pos = _plan_batch(cfg, B, kind)
    users = torch.randint(0, cfg.n_user, (B,), device=seqs.device, generator=torch.Generator(device=seqs.device).manual_seed(B + 1))
    read = lambda which, n: eng.debug_buffer(which, n, torch.int32).clone().cpu().numpy()
    out = {}
    try:
        for on in (1, 0):
            eng.decoder_seq = on
            _, xr, ru = eng.decode(seqs, users, want_x=False, pos=pos, want_r_u=True)
            torch.cuda.synchronize()
            assert eng.decoder_seq_last == bool(on) and eng.decoder_route_last["plan"] == "MULTI"
            out[on] = {"rows": xr.clone(), "r_u": ru.clone(), "cnt": read(8, B), "off": read(7, B), "qrow": read(10, B)}
            if on:
                out[on].update(tseq=read(2, 16 * B), tqb=read(3, 16 * B), row0=read(4, B), qtile=read(5, B), n_wg=read(6, 2))
        pif = eng.pif(users).clone()
    finally:
        eng.decoder_seq = None
    return seqs.cpu().numpy(), pos.cpu().numpy().astype(np.int64), pif, n_cu, out


def _expected_counts(seqs, pos):
    B, L = seqs.shape
    valid = (seqs != 0) | (np.arange(L)[None, :] == pos[:, None])
    cnt = valid.sum(1)
    off = np.cumsum(cnt) - cnt
    before = (valid & (np.arange(L)[None, :] < pos[:, None])).sum(1)
    return cnt, off, before


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", B_PLAN)
def test_plan_tables_against_numpy(B, kind):
    seqs, pos, pif, n_cu, out = _plan_case(B, kind)
    o = out[1]
    cnt, off, before = _expected_counts(seqs, pos)
    assert np.array_equal(o["cnt"], cnt), "seq_cnt"
    assert np.array_equal(o["off"], off), "seq_off: the exclusive sum of the counts"
    assert np.array_equal(o["qrow"], off + before), "seq_qrow: the packed row of the consumed token"
    assert torch.equal(o["r_u"].view(torch.int32), pif.view(torch.int32)), "r_u of the plan kernel: the bits of irs_pif"
    # ---- the workgroup plan
    nb = np.clip((cnt + 15) // 16, 1, C)
    nwg, tail0 = (int(v) for v in o["n_wg"])
    assert (tail0, nwg - tail0) == expected_plan(nb, n_cu), "full and half-live workgroups: the host replica of the rule"
    assert 0 < nwg <= B
    tseq, tqb = o["tseq"], o["tqb"]
    assert (tseq[16 * nwg:] == -1).all(), "-1 behind the workgroups in use"
    used = np.nonzero(tseq[:16 * nwg] >= 0)[0]
    assert ((tseq[:16 * nwg] >= 0) | (tseq[:16 * nwg] == -1)).all() and (tseq[used] < B).all()
    seen = np.zeros((B, C), dtype=np.int32)
    np.add.at(seen, (tseq[used], tqb[used]), 1)
    assert np.array_equal(seen, (np.arange(C)[None, :] < nb[:, None]).astype(np.int32)), "every block of every sequence exactly once"
    wg_of = used // 16
    wg = np.full(B, -1)
    wg[tseq[used]] = wg_of
    assert np.array_equal(wg[tseq[used]], wg_of), "a sequence sits in one workgroup"
    first = np.full(B, 16)
    np.minimum.at(first, tseq[used], used % 16)
    assert np.array_equal(o["row0"], 16 * first), "seq_row0: the sequence's first half tile in its workgroup"
    half = np.full((B, C), -1)
    half[tseq[used], tqb[used]] = used
    assert np.array_equal(o["qtile"], 16 * half[np.arange(B), before >> 4] + (before & 15)), "qrow_tile"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", B_PLAN)
def test_plan_without_the_workgroup_plan(B, kind):
    """decoder_seq = 0: a MULTI plan without k_plan_seq gets the same counts, offsets and consumed rows"""
    _, _, pif, _, out = _plan_case(B, kind)
    for k in ("cnt", "off", "qrow"):
        assert np.array_equal(out[0][k], out[1][k]), k
    assert torch.equal(out[0]["r_u"].view(torch.int32), pif.view(torch.int32))
    a, two = out[1]["rows"], out[0]["rows"]
    assert torch.equal(torch.isnan(a), torch.isnan(two)), "NaN pattern of the two-kernel path"
    fin = ~torch.isnan(two)
    assert fin.any()
    err = (a - two)[fin].abs().max().item()
    print(f"B={B} {kind}: sequence-resident vs two-kernel rows: max {err:.3g} (bound {X_TOL[IRS_GEMM_H3]:.3g})")
    assert err < X_TOL[IRS_GEMM_H3], err


@functools.lru_cache(maxsize=None)
def _ring_case(target):
    """192 IRN windows of RING_LENGTHS tokens, consumed at L - 2 (even variants) or at a middle token (odd ones)"""
    cfg, eng, _ = _rig()
    L = cfg.max_len
    g = np.random.default_rng(77 + target)
    seqs = np.zeros((B_RING, L), dtype=np.int64)
    pos = np.zeros(B_RING, dtype=np.int32)
    for b in range(B_RING):
        n, v = RING_LENGTHS[b % len(RING_LENGTHS)], b // len(RING_LENGTHS)
        items = n if target else n - 1  # without a target: the last column stays 0
        seqs[b, L - n:L - n + items] = g.integers(1, cfg.n_item + 1, size=items)
        pos[b] = L - 2 if v % 2 == 0 else L - n + items // 2
    perm = g.permutation(B_RING)
    seq, p = torch.from_numpy(seqs[perm]).cuda(), torch.from_numpy(pos[perm]).cuda()
    usr = torch.from_numpy(np.random.default_rng(5).integers(0, cfg.n_user, size=B_RING)).cuda()
    got = []
    try:
        for on in [1] * CALLS + [0]:
            eng.decoder_seq = on
            got.append(eng.decode(seq, usr, want_x=False, pos=p)[1].clone())
            torch.cuda.synchronize()
            assert eng.decoder_seq_last == bool(on)
    finally:
        eng.decoder_seq = None
    return got[:CALLS], got[CALLS]


@pytest.mark.parametrize("target", [True, False])
def test_absorbed_attention_block_edges(target):
    got, two = _ring_case(target)
    for k in range(1, CALLS):
        assert torch.equal(got[0].view(torch.int32), got[k].view(torch.int32)), f"call {k} of {CALLS}: other bits than call 0"
    assert torch.equal(torch.isnan(got[0]), torch.isnan(two)), "NaN pattern of the two-kernel path"
    fin = ~torch.isnan(two)
    assert fin.all(dim=1).float().mean().item() > 0.6
    err = (got[0] - two)[fin].abs().max().item()
    print(f"target={target}: sequence-resident vs two-kernel rows: max {err:.3g} (bound {X_TOL_ROW:.3g})")
    assert err < X_TOL_ROW, err
