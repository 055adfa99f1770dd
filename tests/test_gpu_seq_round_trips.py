"""The sequence-resident decoder launch with its global-memory traffic batched (k_block_x6<.., SEQ>): layer 0's
parameter vectors and the 32 pieces of a token's embedding and position rows requested by inline-asm loads with ONE wait each,
the token's row index by an inline-asm load of its own, the x' tile of LayerNorm 3 stored by inline-asm stores with no wait
between them, the idle waves ending the program where they stand.  None of it changes arithmetic.

What the new placement can break, and where it would show:
  * the gather: a piece at the wrong offset, a dead lane that keeps what it loaded (lanes beyond a window's tokens read row 0 of
    both tables and must hold zeros), the clamp of item ids to [0, n_item] -- windows of 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49,
    127, 128, 129, 199 and 200 tokens in one call: one, two and odd block counts, so empty halves and middle tiles shared by two
    sequences; a window whose first and last item is n_item (the last row of the table), windows whose leading columns are 0 and
    one without a target item (last column 0);
  * the x' stores: a tile base off by a wave or a workgroup puts one wave's residual under another's -- rows far outside the
    bound from the second layer on, so 3 layers (two trips of the layer loop, the first ordered by the empty step's wait) beside
    2 (one trip, ordered by the wait at the kernel's end);
  * an asm load used before its wait (a copy the register allocator places between them): wrong values in some lanes, possibly
    different from call to call -- five calls on one batch must give the same bits;
  * the idle waves' end: a batch that leaves fully idle waves beside live ones, and one whose last round is half-live.

Consumed rows against an all-float64 decode of the same window (oracle_np.decode) within 5e-5, the bound the other sequence
tests hold, and against the layer + attention kernel pair (irs_set_decoder_seq mode 0) within the same bound; NaN patterns equal.

The only geometry the launch supports: d = 128, 4 heads, F = 256, L = 200.  The route needs more than 32768 token rows, so the
batch is 176 windows, each of the 16 lengths 11 times.  The first three repeats of every length -- 48 windows, the special ones
among them -- are the ones held against float64 (the float64 decodes are the slow part of this file); all 176 are held against
the two-kernel route.  The float64 rows are computed once per (layers, mask) and shared; a test without the gpu mark checks that
they are finite.

Measured on MI355X (rows against float64 at most 8.34e-6, against the two-kernel route 1.14e-5): profiles/seq_round_trips/README.md."""
import functools

import numpy as np
import pytest
import torch

from gpu_util import make_engine
from influentialrs_amd import synth
from test_gpu_seq_front_order import CALLS, _idle_waves
from test_gpu_seq_last_absorbed import _agree, _rows, reference_rows
from test_gpu_seq_tail_plan import B_MAX, _windows, plain_workgroups

X_TOL_ROW = 5e-5  # consumed rows: against the float64 reference and between the two decoder routes (tests/test_gpu_decoder_path.py)
LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 127, 128, 129, 199, 200]
REPEATS = 11
REF_REPEATS = 3  # repeats of every length that are compared with the float64 decode: plain, n_item at both ends, (full length) no target
B = len(LENGTHS) * REPEATS  # 176 windows of 200 columns: above the switch to the throughput kernels
N_ITEM = 300
CASES = [(2, False), (3, False), (2, True), (3, True)]


def make_batch(L, evaluator, seed):
    """Window b has LENGTHS[b % 16] tokens.  Repeat 1 of every length starts and ends with item n_item; IRN: repeat 2 of the full
    length has no target item (199 items, last column 0: the target-less window inside the reference's domain).  Returns the
    windows, the consumed positions, the index of the target-less window (-1: none) and the indices of the windows of the first
    REF_REPEATS repeats, in a fixed random order."""
    assert B * L > 32768
    g = np.random.default_rng(seed)
    seqs = np.zeros((B, L), dtype=np.int64)
    pos = np.zeros(B, dtype=np.int32)
    no_target = -1
    for b in range(B):
        n, rep = min(LENGTHS[b % len(LENGTHS)], L), b // len(LENGTHS)
        c0 = 0 if evaluator else L - n  # post-padded (evaluator windows) or pre-padded with the target last
        seqs[b, c0:c0 + n] = g.integers(1, N_ITEM + 1, size=n)
        pos[b] = (n - 1) if evaluator else (L - 2 if n > 1 else L - 1)
        if rep == 1:
            seqs[b, c0] = seqs[b, c0 + n - 1] = N_ITEM
        if rep == 2 and n == L and not evaluator:
            seqs[b, L - 1] = 0
            no_target = b
    perm = g.permutation(B)
    inv = np.argsort(perm)
    return seqs[perm], pos[perm], (int(inv[no_target]) if no_target >= 0 else -1), np.sort(inv[:REF_REPEATS * len(LENGTHS)])


@functools.lru_cache(maxsize=None)
def _inputs(n_layers, evaluator):
    cfg = synth.make_config("c2", n_item=N_ITEM, n_layers=n_layers, **({"n_user": 0} if evaluator else {}))
    assert (cfg.emb_dim, cfg.n_heads, cfg.ffn_dim, cfg.max_len) == (128, 4, 256, 200)
    sd = synth.irn_state_dict(cfg, 31, evaluator=evaluator)
    seqs, pos, no_target, checked = make_batch(cfg.max_len, evaluator, 20261020 + n_layers)
    users = None if evaluator else np.random.default_rng(5).integers(0, cfg.n_user, size=B)
    return cfg, sd, seqs, pos, users, no_target, checked


@functools.lru_cache(maxsize=None)
def _reference(n_layers, evaluator):
    """row pos[b] of an all-float64 decode of every checked window: computed once, read by the tests below"""
    from oracle import oracle_np
    cfg, sd, seqs, pos, users, _, checked = _inputs(n_layers, evaluator)
    ref = reference_rows(oracle_np, sd, cfg, seqs[checked], None if users is None else users[checked], pos[checked], evaluator)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _decoded(n_layers, evaluator):
    """five decodes by the sequence-resident route and one by the two-kernel route"""
    cfg, sd, seqs, pos, users, _, _ = _inputs(n_layers, evaluator)
    eng = make_engine(cfg, sd, evaluator=evaluator, max_rows=B, max_seqs=B)
    seq, p = torch.from_numpy(seqs).cuda(), torch.from_numpy(pos).cuda()
    usr = None if evaluator else torch.from_numpy(users).cuda()
    try:
        got = [_rows(eng, seq, usr, p, 1) for _ in range(CALLS)]  # (_rows asserts that the route was the sequence-resident one)
        nwg, idle, _ = _idle_waves(eng, B)
        two = _rows(eng, seq, usr, p, 0)
    finally:
        eng.decoder_seq = None
    return got, two, nwg, idle


def test_batch_holds_the_windows_it_names():
    for evaluator in (False, True):
        seqs, pos, no_target, checked = make_batch(200, evaluator, 1)
        n = (seqs != 0).sum(1)
        assert len(checked) == 48 and sorted(set(n[checked].tolist()) | ({200} if not evaluator else set())) == sorted(LENGTHS)
        assert (seqs[checked] == N_ITEM).any(1).sum() >= len(LENGTHS) and (no_target in checked or evaluator)
        assert sorted(set(n.tolist()) | ({200} if not evaluator else set())) == sorted(LENGTHS)
        assert (seqs == N_ITEM).any(1).sum() >= len(LENGTHS) and seqs.max() == N_ITEM and seqs.min() == 0
        if not evaluator:
            assert no_target >= 0 and seqs[no_target, -1] == 0 and n[no_target] == 199 and seqs[no_target, 0] != 0
            assert (seqs[np.arange(B) != no_target, -1] != 0).all()


@pytest.mark.parametrize("n_layers,evaluator", CASES)
def test_reference_rows_are_finite(oracle, n_layers, evaluator):
    """(no GPU) the float64 oracle alone gives a finite consumed row for every window it is asked for"""
    assert np.isfinite(_reference(n_layers, evaluator)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_layers,evaluator", CASES)
def test_rows_against_float64_reference(oracle, n_layers, evaluator):
    ref, checked = _reference(n_layers, evaluator), _inputs(n_layers, evaluator)[6]
    g = _decoded(n_layers, evaluator)[0][0].cpu().numpy()
    assert not np.isnan(g).any(), "NaN pattern of the reference (finite everywhere)"
    err = np.abs(g[checked].astype(np.float64) - ref)
    print(f"{n_layers} layers, {'causal' if evaluator else 'IRN'}: rows vs float64 max {err.max():.3g} mean {err.mean():.3g} (bound {X_TOL_ROW:.3g})")
    assert err.max() < X_TOL_ROW, err.max()


@pytest.mark.gpu
@pytest.mark.parametrize("n_layers,evaluator", CASES)
def test_five_calls_same_bits(n_layers, evaluator):
    got = _decoded(n_layers, evaluator)[0]
    for k in range(1, CALLS):
        assert torch.equal(got[0].view(torch.int32), got[k].view(torch.int32)), f"call {k} of {CALLS}: other bits than call 0"


@pytest.mark.gpu
@pytest.mark.parametrize("n_layers,evaluator", CASES)
def test_agrees_with_two_kernel_route(n_layers, evaluator):
    got, two, nwg, idle = _decoded(n_layers, evaluator)
    print(f"{nwg} workgroups, {idle} fully idle waves")
    assert idle > 0, "the plan left no fully idle wave: the idle path did not run"
    _agree(got[0], two)


@pytest.mark.gpu
def test_half_live_last_round():
    """A short last round is planned as half-live workgroups (tests/test_gpu_seq_tail_plan.py): waves 0 .. 3 of each are idle for the
    whole launch and end the program from inside their loop, beside live waves 4 .. 7 that gather, store and read back their tiles."""
    dev = torch.device("cuda:0")
    cfg = synth.make_config("c2", n_layers=3)
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
