"""The model's last decoder layer behind the sequence-resident launch: the one consumed row per sequence attends from x' with
absorbed K / V projections (k_absorb_qu, k_absorb_attn, k_absorb_out), and k_block_x6<.., SEQ> ends behind
its last full layer instead of running a front-only trip for every token.

What the change can break, and where it would show:
  * the absorbed attention row itself: consumed rows against an all-float64 decode of the same window (oracle_np.decode, row
    pos[b]) within the project's row tolerance, 5e-5, and the same NaN pattern;
  * the tile-order walk over x' (seq_half_of_block, the sequence's first half tile, rows beyond cnt): windows of 1, 2, 15, 16, 17,
    31, 32, 33, 47, 48, 49 and 200 tokens in one call -- one block, a consumed token in the first / a middle / the last block, a
    mirrored pair whose partner is absent, a tile shared with a neighbouring sequence;
  * the mask rule: consumed positions L - 2 (the search's), L - 1 (the target itself), the first valid token, a middle token and a
    pad position, IRN mask on pre-padded windows with a target and without one, causal mask on post-padded evaluator windows;
  * the shortened ring of the fused launch: 2 layers (one loop layer, which is then also the launch's last) and 3, five calls on
    one batch with the same bits, a batch whose last round is half-live (waves 0 .. 3 on the idle path through the shortened loop);
  * agreement with the layer + attention kernel pair (irs_set_decoder_seq mode 0) within 5e-5 on the same batches.

An IRN window WITHOUT a target item and WITH pads in front is outside the reference's domain (its pad rows see no key, 0 x NaN
then poisons every row from layer 2 on: the oracle is NaN everywhere, the kernels skip pads and stay finite;
tests/test_gpu_decoder_path.py says the same).  Against the reference the target-less windows are therefore the ones without a
pad in front (199 items, last column 0); target-less windows of every length run in the comparison of the two kernel paths, where
a consumed pad with no visible key must be NaN on both sides.

The only geometry the launch supports: d = 128, 4 heads, F = 256, L = 200; n_item = 300, 168 windows (the smallest batch above
the 32768-row switch to the throughput kernels).

Measured on MI355X, rows against the float64 reference (bound 5e-5): see profiles/seq_last_absorbed/README.md."""
import functools

import numpy as np
import pytest
import torch

from gpu_util import make_engine
from influentialrs_amd import synth
from test_gpu_seq_front_order import B, CALLS, LENGTHS, _idle_waves
from test_gpu_seq_tail_plan import B_MAX, _windows, plain_workgroups

pytestmark = pytest.mark.gpu

X_TOL_ROW = 5e-5  # consumed rows: against the float64 reference and between the two decoder paths (tests/test_gpu_decoder_path.py)
NV = B // len(LENGTHS)  # 14 variants of every length


def make_batch(L, n_item, evaluator, seed, short_without_target=False):
    """168 windows: length LENGTHS[b % 12], variant b // 12 = the consumed position's kind (and, IRN, from variant 10 on: no target)."""
    g = np.random.default_rng(seed)
    seqs = np.zeros((B, L), dtype=np.int64)
    pos = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n, v = min(LENGTHS[b % len(LENGTHS)], L), b // len(LENGTHS)
        if evaluator:  # post-padded: items in columns [0, n)
            seqs[b, :n] = g.integers(1, n_item + 1, size=n)
            pos[b] = [n - 1, L - 1, 0, n // 2, min(n, L - 1), L - 2, n - 1][v % 7]  # last item, last column, first, middle, first pad, L - 2
            continue
        target = not (v >= 10 and (n == L or short_without_target))
        if target:  # pre-padded, target last: items in columns [L - n, L)
            seqs[b, L - n:] = g.integers(1, n_item + 1, size=n)
            pos[b] = [L - 2 if n > 1 else L - 1, L - 1, L - n, L - n + n // 2, L - n - 1 if n < L else L - 2][v % 5]
        else:  # n - 1 items in columns [L - n, L - 1), last column 0
            seqs[b, L - n:L - 1] = g.integers(1, n_item + 1, size=n - 1)
            # (variants 10 .. 13: L - 2, the pad in the last column, a middle token, a pad in front of the history)
            pos[b] = [L - 2, L - 1, L - n + (n - 1) // 2, L - n - 1 if n < L else L - 1][v - 10]
    perm = g.permutation(B)
    return seqs[perm], pos[perm]


def reference_rows(oracle, sd, cfg, seqs, users, pos, evaluator):
    """row pos[b] of an all-float64 decode of window b"""
    out = np.empty((len(seqs), cfg.emb_dim), dtype=np.float64)
    for b in range(len(seqs)):
        x, _ = oracle.decode(sd, cfg, seqs[b], None if evaluator else int(users[b]), evaluator=evaluator, dtype=np.float64)
        out[b] = x[pos[b]]
    return out


def _rows(eng, seq, usr, pos, on):
    eng.decoder_seq = on
    xr = eng.decode(seq, usr, want_x=False, pos=pos)[1].clone()
    torch.cuda.synchronize()
    assert eng.decoder_seq_last == bool(on)
    return xr


@functools.lru_cache(maxsize=None)
def _case(n_layers, evaluator, short_without_target=False):
    """engine, batch, five decodes by the sequence-resident route and one by the two-kernel route: shared by the tests below"""
    cfg = synth.make_config("c2", n_item=300, n_layers=n_layers, **({"n_user": 0} if evaluator else {}))
    assert (cfg.emb_dim, cfg.n_heads, cfg.ffn_dim, cfg.max_len) == (128, 4, 256, 200) and B * cfg.max_len > 32768
    sd = synth.irn_state_dict(cfg, 31, evaluator=evaluator)
    eng = make_engine(cfg, sd, evaluator=evaluator, max_rows=B, max_seqs=B)
    seqs, pos = make_batch(cfg.max_len, cfg.n_item, evaluator, 20261019 + n_layers + (50 if short_without_target else 0), short_without_target)
    users = None if evaluator else np.random.default_rng(5).integers(0, cfg.n_user, size=B)
    seq, p = torch.from_numpy(seqs).cuda(), torch.from_numpy(pos).cuda()
    usr = None if evaluator else torch.from_numpy(users).cuda()
    try:
        got = [_rows(eng, seq, usr, p, 1) for _ in range(CALLS)]
        two = _rows(eng, seq, usr, p, 0)
    finally:
        eng.decoder_seq = None
    return cfg, sd, seqs, pos, users, got, two


CASES = [(2, False), (3, False), (2, True), (3, True)]


@pytest.mark.parametrize("n_layers,evaluator", CASES)
def test_rows_against_float64_reference(oracle, n_layers, evaluator):
    cfg, sd, seqs, pos, users, got, _ = _case(n_layers, evaluator)
    ref = reference_rows(oracle, sd, cfg, seqs, users, pos, evaluator)
    fin = ~np.isnan(ref)
    assert fin.all(axis=1).mean() > 0.6, "the reference itself must be finite in most rows"
    g = got[0].cpu().numpy()
    assert np.array_equal(np.isnan(g), ~fin), "NaN pattern of the reference"
    err = np.abs(g.astype(np.float64) - ref)[fin]
    print(f"{n_layers} layers, {'causal' if evaluator else 'IRN'}: rows vs float64 max {err.max():.3g} mean {err.mean():.3g} (bound {X_TOL_ROW:.3g})")
    assert err.max() < X_TOL_ROW, err.max()


@pytest.mark.parametrize("n_layers,evaluator", CASES)
def test_five_calls_same_bits(n_layers, evaluator):
    got = _case(n_layers, evaluator)[5]
    for k in range(1, CALLS):
        assert torch.equal(got[0].view(torch.int32), got[k].view(torch.int32)), f"call {k} of {CALLS}: other bits than call 0"


def _agree(got, two):
    assert torch.equal(torch.isnan(two), torch.isnan(got)), "NaN pattern of the two-kernel path"
    fin = ~torch.isnan(two)
    assert fin.all(dim=1).float().mean().item() > 0.6
    err = (two - got)[fin].abs().max().item()
    print(f"sequence-resident vs two-kernel rows: max {err:.3g} (bound {X_TOL_ROW:.3g})")
    assert err < X_TOL_ROW, err


@pytest.mark.parametrize("n_layers,evaluator", CASES)
def test_agrees_with_two_kernel_path(n_layers, evaluator):
    _, _, _, _, _, got, two = _case(n_layers, evaluator)
    _agree(got[0], two)


def test_windows_without_target_agree_with_two_kernel_path():
    """IRN windows of every length without a target item (last column 0): the last key is a causal key like any other, a consumed
    pad in front of the history sees no key at all -- NaN on both paths --, the same bits on every call."""
    _, _, seqs, pos, _, got, two = _case(2, False, True)
    assert (seqs[:, -1] == 0).sum() >= 40
    for k in range(1, CALLS):
        assert torch.equal(got[0].view(torch.int32), got[k].view(torch.int32))
    assert torch.isnan(two).any(), "a consumed position without a visible key is in the batch"
    _agree(got[0], two)


def test_half_live_last_round():
    """A short last round is planned as half-live workgroups (tests/test_gpu_seq_tail_plan.py): their waves 0 .. 3 take the idle
    path through the shortened layer loop for the whole launch -- its ring duty must end with the live path's."""
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
    seq = seqs[:nB].contiguous()
    users = torch.randint(0, cfg.n_user, (nB,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    pos = torch.full((nB,), cfg.max_len - 2, dtype=torch.int32, device=dev)
    try:
        got = [_rows(eng, seq, users, pos, 1) for _ in range(CALLS)]
        nwg, idle, tail0 = _idle_waves(eng, nB)
        two = _rows(eng, seq, users, pos, 0)
    finally:
        eng.decoder_seq = None
    assert tail0 < nwg, "the last round was half-live"
    assert idle >= 4 * (nwg - tail0), "waves 0 .. 3 of a half-live workgroup are idle"
    for k in range(1, CALLS):
        assert torch.equal(got[0].view(torch.int32), got[k].view(torch.int32)), f"call {k} of {CALLS}: other bits than call 0"
    assert not torch.isnan(got[0]).any()
    _agree(got[0], two)
