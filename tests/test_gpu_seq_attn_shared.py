"""The sequence-resident decoder's attention when the two blocks of a wave share their per-head work (k_block_x6<.., SEQ>:
the target column's key and V row are rebuilt once per head and sequence, the diagonal masks once per wave).

Sharing can go wrong where the halves of a wave differ, so one call holds windows of 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49 and
200 tokens: one block alone (its wave's other half empty or another sequence's), two mirrored blocks in one wave, odd block
counts (3, 13: the middle block sits alone or beside another sequence's middle block), with a target item and (a test of its
own) without one, with the one pad a packed sequence may hold (the consumed position) at packed index 0, 15, 16 and n - 2, under the IRN and the causal
masks, at 2 and 3 layers.  Rows of irs_set_decoder_seq mode 1 against mode 0 (the layer + attention kernel pair) on the same
batch at the bound test_gpu_decoder_path.py holds the two paths to; two calls give the same bits.  A batch whose plan ends in
a half-live round (the trigger of test_gpu_seq_tail_plan.py) gets the same comparison."""
import numpy as np
import pytest
import torch

from gpu_util import make_engine
from influentialrs_amd import synth
from test_gpu_seq_tail_plan import B_MAX, _windows, plain_workgroups

pytestmark = pytest.mark.gpu

X_TOL_PATHS = 5e-5  # sequence-resident against two-kernel rows (the bound of tests/test_gpu_decoder_path.py's row comparisons)

LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 200]
KINDS = 7  # plain | pad at packed index 0 | 15 | 16 | n - 2 | plain, or no target item (no_target) | plain
B = len(LENGTHS) * KINDS * 2  # 168 windows of 200 columns: above the switch to the throughput kernels


def _batch(cfg, evaluator, seed, no_target=False):
    L = cfg.max_len
    assert B * L > 32768
    g = np.random.default_rng(seed)
    seqs = np.zeros((B, L), dtype=np.int64)
    pos = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = LENGTHS[b % len(LENGTHS)]
        kind = (b // len(LENGTHS)) % KINDS
        items = g.integers(1, cfg.n_item + 1, size=n)
        c0 = 0 if evaluator else L - n  # post-padded (evaluator windows) or pre-padded with the target last
        seqs[b, c0:c0 + n] = items
        pos[b] = (n - 1) if evaluator else (L - 2 if n > 1 else L - 1)
        q = {1: 0, 2: 15, 3: 16, 4: n - 2}.get(kind, -1)
        if 0 <= q < n - 1:  # the consumed position is a pad inside the window: the one pad of the packed sequence
            seqs[b, c0 + q] = 0
            pos[b] = c0 + q
        if no_target and kind == 5 and not evaluator and n > 1:
            seqs[b, L - 1] = 0  # target id 0: no target column
    perm = g.permutation(B)
    return seqs[perm], pos[perm]


def _rows(eng, seq, usr, pos, on):
    eng.decoder_seq = on
    xr = eng.decode(seq, usr, want_x=False, pos=pos)[1].clone()
    torch.cuda.synchronize()
    assert eng.decoder_seq_last == bool(on)
    return xr


def _compare(eng, seq, usr, pos):
    try:
        ref = _rows(eng, seq, usr, pos, 0)
        got = _rows(eng, seq, usr, pos, 1)
        again = _rows(eng, seq, usr, pos, 1)
    finally:
        eng.decoder_seq = None
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two calls: the same bits"
    # (a consumed position with no visible key -- a pad in front of the whole history -- is NaN on both sides, as in the reference)
    assert torch.equal(torch.isnan(ref), torch.isnan(got))
    fin = ~torch.isnan(ref)
    assert fin.all(dim=1).float().mean().item() > 0.6
    err = (ref - got)[fin].abs().max().item()
    print(f"sequence-resident vs two-kernel rows: max {err:.3g} (bound {X_TOL_PATHS:.3g})")
    assert err < X_TOL_PATHS, err


@pytest.mark.parametrize("evaluator", [False, True])
@pytest.mark.parametrize("n_layers", [2, 3])
def test_shared_target_and_masks_on_mixed_waves(n_layers, evaluator):
    cfg = synth.make_config("c2", n_item=300, n_layers=n_layers, **({"n_user": 0} if evaluator else {}))
    eng = make_engine(cfg, synth.irn_state_dict(cfg, 29, evaluator=evaluator), evaluator=evaluator, max_rows=B, max_seqs=B)
    seqs, pos = _batch(cfg, evaluator, 20261017 + n_layers)
    g = np.random.default_rng(5)
    seq = torch.from_numpy(seqs).cuda()
    usr = None if evaluator else torch.from_numpy(g.integers(0, cfg.n_user, size=B)).cuda()
    _compare(eng, seq, usr, torch.from_numpy(pos).cuda())


def test_irn_windows_without_a_target_item():
    """Target id 0 under the IRN mask (no target column) beside windows that have one.  Without a target item the last key of the
    packed sequence is the last history item, a causal key like any other (the reference masks the window's last COLUMN, which
    is then a pad).  The block attention kernels used to mask that key whatever it was while the single-query kernel of the
    rows-only last layer did not: rows of such windows differed between the two decoder paths by 8e-3 (200 tokens) to 0.144
    (16 tokens), and 2-token windows were NaN on one side only."""
    cfg = synth.make_config("c2", n_item=300, n_layers=2)
    eng = make_engine(cfg, synth.irn_state_dict(cfg, 29), max_rows=B, max_seqs=B)
    seqs, pos = _batch(cfg, False, 20261019, no_target=True)
    usr = torch.from_numpy(np.random.default_rng(5).integers(0, cfg.n_user, size=B)).cuda()
    _compare(eng, torch.from_numpy(seqs).cuda(), usr, torch.from_numpy(pos).cuda())


def test_half_live_last_round():
    dev = torch.device("cuda:0")
    cfg = synth.make_config("c2", n_layers=2)
    eng = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=B_MAX, max_seqs=B_MAX)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    seqs = _windows(cfg, dev, "bench")
    nb = np.clip(((seqs != 0).sum(1).cpu().numpy() + 15) // 16, 1, 16)
    # the prefix of the batch whose plain plan ends nearest 0.1 of a round behind two whole ones: the plan's tail rule applies
    best = min((abs((plain_workgroups(nb[:b]) % n_cu) / n_cu - 0.1), b) for b in range(384, B_MAX + 1, 8)
               if plain_workgroups(nb[:b]) >= 2 * n_cu)
    assert best[0] < 0.05, best
    nB = best[1]
    users = torch.randint(0, cfg.n_user, (nB,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    pos = torch.full((nB,), cfg.max_len - 2, dtype=torch.int32, device=dev)
    _compare(eng, seqs[:nB].contiguous(), users, pos)
    nwg, tail0 = (int(v) for v in eng.debug_buffer(6, 2, torch.int32).cpu().numpy())
    assert tail0 < nwg, "the last round was half-live"
