"""The sequence-resident decoder's front when a head's steps run in the order k, v, q and the K / V epilogues (bias, split into
float16 planes, image rows) ride between the matrix instructions of the NEXT step (k_block_x6<.., SEQ>).

What the new placement can break, and where it would show:
  * the ring: front step i now fetches component (i % 3 + 1) % 3 -- in the live waves' refills, in the idle path of empty waves and
    in the prefetch of the next layer's first steps behind a layer's body.  A mismatch gives live waves the wrong weights: rows far
    outside the bound between the two decoder paths, at 2 layers (one boundary, then the last trip) and at 3;
  * the images: head h + 1's K rows are written one workgroup barrier behind the last read of head h's.  A race would show as
    run-to-run differences: five calls on one batch must give the same bits;
  * the image rows themselves (inline-asm stores behind the `l_b >= 0` predicate): windows of 1, 2, 15, 16, 17, 31, 32, 33, 47,
    48, 49 and 200 tokens in one call -- one block alone, mirrored pairs, odd middle blocks, a wave whose other half is empty or
    another sequence's --, IRN mask on pre-padded windows with a target, causal mask on post-padded evaluator windows;
  * every head position with full and with single-tile blocks: every window 16 tokens, every window 208 (clipped to L = 200).

Rows of irs_set_decoder_seq mode 1 against mode 0 (the layer + attention kernel pair) on the same batch within the 5e-5 that
test_gpu_decoder_path.py holds the two paths to; NaN patterns equal.  The only geometry the kernel supports: d = 128, 4 heads,
F = 256, L = 200; about 170 windows (the smallest batch above the switch to the throughput kernels)."""
import numpy as np
import pytest
import torch

from gpu_util import make_engine
from influentialrs_amd import synth
from test_gpu_seq_tail_plan import B_MAX, _windows, plain_workgroups

pytestmark = pytest.mark.gpu

X_TOL_PATHS = 5e-5  # sequence-resident against two-kernel rows (the bound of tests/test_gpu_decoder_path.py's row comparisons)
CALLS = 5

LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 200]
B = len(LENGTHS) * 14  # 168 windows of 200 columns: above the switch to the throughput kernels


def _batch(cfg, evaluator, seed, lengths=LENGTHS):
    L = cfg.max_len
    assert B * L > 32768
    g = np.random.default_rng(seed)
    seqs = np.zeros((B, L), dtype=np.int64)
    pos = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = min(lengths[b % len(lengths)], L)
        c0 = 0 if evaluator else L - n  # post-padded (evaluator windows) or pre-padded with the target last
        seqs[b, c0:c0 + n] = g.integers(1, cfg.n_item + 1, size=n)
        pos[b] = (n - 1) if evaluator else (L - 2 if n > 1 else L - 1)
    perm = g.permutation(B)
    return seqs[perm], pos[perm]


def _rows(eng, seq, usr, pos, on):
    eng.decoder_seq = on
    xr = eng.decode(seq, usr, want_x=False, pos=pos)[1].clone()
    torch.cuda.synchronize()
    assert eng.decoder_seq_last == bool(on)
    return xr


def _compare(eng, seq, usr, pos, all_finite=False):
    try:
        ref = _rows(eng, seq, usr, pos, 0)
        got = [_rows(eng, seq, usr, pos, 1) for _ in range(CALLS)]
    finally:
        eng.decoder_seq = None
    for k in range(1, CALLS):
        assert torch.equal(got[0].view(torch.int32), got[k].view(torch.int32)), f"call {k} of {CALLS}: other bits than call 0"
    # (a consumed position with no visible key is NaN on both sides, as in the reference)
    assert torch.equal(torch.isnan(ref), torch.isnan(got[0]))
    fin = ~torch.isnan(ref)
    if all_finite:
        assert fin.all()
    assert fin.all(dim=1).float().mean().item() > 0.6
    err = (ref - got[0])[fin].abs().max().item()
    print(f"sequence-resident vs two-kernel rows: max {err:.3g} (bound {X_TOL_PATHS:.3g})")
    assert err < X_TOL_PATHS, err


def _idle_waves(eng, n_seq):
    """(workgroups in use, fully idle waves among them, first half-live workgroup) of the last decode's plan"""
    nwg, tail0 = (int(v) for v in eng.debug_buffer(6, 2, torch.int32).cpu().numpy())
    tseq = eng.debug_buffer(2, n_seq * 16, torch.int32).clone().cpu().numpy()[:16 * nwg].reshape(nwg, 8, 2)
    return nwg, int((tseq < 0).all(2).sum()), tail0


def _engine(n_layers, evaluator, max_rows=B):
    cfg = synth.make_config("c2", n_item=300, n_layers=n_layers, **({"n_user": 0} if evaluator else {}))
    assert (cfg.emb_dim, cfg.n_heads, cfg.ffn_dim, cfg.max_len) == (128, 4, 256, 200)
    return cfg, make_engine(cfg, synth.irn_state_dict(cfg, 31, evaluator=evaluator), evaluator=evaluator, max_rows=max_rows, max_seqs=max_rows)


def _users(cfg, evaluator, n):
    return None if evaluator else torch.from_numpy(np.random.default_rng(5).integers(0, cfg.n_user, size=n)).cuda()


@pytest.mark.parametrize("evaluator", [False, True])
@pytest.mark.parametrize("n_layers", [2, 3])
def test_window_lengths_masks_and_layer_counts(n_layers, evaluator):
    """IRN mask / pre-padded with a target (evaluator = False), causal mask / post-padded (True); 2 and 3 layers."""
    cfg, eng = _engine(n_layers, evaluator)
    seqs, pos = _batch(cfg, evaluator, 20261019 + n_layers)
    _compare(eng, torch.from_numpy(seqs).cuda(), _users(cfg, evaluator, B), torch.from_numpy(pos).cuda())


@pytest.mark.parametrize("tokens", [16, 208])
def test_every_head_position_on_uniform_windows(tokens):
    """Every window the same length: the head loop's four positions with single-tile blocks (16) and with full ones (208 -> L).
    The 16-token batch also leaves fully idle waves beside live ones (one block per window, two per wave): the idle path's ring
    duty against the live waves' consumption."""
    cfg, eng = _engine(2, False)
    seqs, pos = _batch(cfg, False, 77 + tokens, lengths=[tokens])
    _compare(eng, torch.from_numpy(seqs).cuda(), _users(cfg, False, B), torch.from_numpy(pos).cuda(), all_finite=True)
    nwg, idle, _ = _idle_waves(eng, B)
    print(f"{tokens} tokens: {nwg} workgroups, {idle} fully idle waves")
    if tokens == 16:
        assert idle > 0, "the plan left no fully idle wave: the idle path did not run"


def test_half_live_last_round():
    """The trigger of test_gpu_seq_tail_plan.py: a short last round is given half-live workgroups (live tiles on waves 4 .. 7,
    waves 0 .. 3 on the idle path for the whole launch)."""
    dev = torch.device("cuda:0")
    cfg = synth.make_config("c2", n_layers=2)
    eng = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=B_MAX, max_seqs=B_MAX)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    seqs = _windows(cfg, dev, "bench")
    nb = np.clip(((seqs != 0).sum(1).cpu().numpy() + 15) // 16, 1, 16)
    best = min((abs((plain_workgroups(nb[:b]) % n_cu) / n_cu - 0.1), b) for b in range(384, B_MAX + 1, 8)
               if plain_workgroups(nb[:b]) >= 2 * n_cu)
    assert best[0] < 0.05, best
    nB = best[1]
    users = torch.randint(0, cfg.n_user, (nB,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    pos = torch.full((nB,), cfg.max_len - 2, dtype=torch.int32, device=dev)
    _compare(eng, seqs[:nB].contiguous(), users, pos)
    nwg, idle, tail0 = _idle_waves(eng, nB)
    assert tail0 < nwg, "the last round was half-live"
    assert idle >= 4 * (nwg - tail0), "waves 0 .. 3 of a half-live workgroup are idle"
