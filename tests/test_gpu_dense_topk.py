"""-m gpu: the dense form of the swept top-k (irs_set_topk_dense; csrc/score.hip: k_sweep_ring16 in image mode + k_dense_select)
against the exhaustive exact kernel (IRS_SWEEP_EXHAUSTIVE) on the same engine: ids equal, value bits equal, status equal
except bit 0 (IRS_ROW_FALLBACK).  The switch is forced to 1 so that the kernels are reached at a handful of rows."""
import numpy as np
import pytest
import torch

from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_SWEEP_BF16, IRS_SWEEP_EXHAUSTIVE, IRS_SWEEP_F32
from gpu_util import make_engine, scoring_only_engine

pytestmark = pytest.mark.gpu


def _weights(n_item, d, seed):
    g = np.random.default_rng(seed)
    W = ((g.random((n_item, d), dtype=np.float32) * 2 - 1) / np.sqrt(d)).astype(np.float32)
    b = (g.standard_normal(n_item) * 0.1).astype(np.float32)
    return W, b


def _rows(M, d, seed):
    return np.random.default_rng(seed + 100).standard_normal((M, d)).astype(np.float32)


def _same(got, ref, what=""):
    (v, i, s), (rv, ri, rs) = got, ref
    assert torch.equal(i, ri), f"{what}: ids differ in {int((i != ri).any(1).sum())} rows"
    assert torch.equal(v.view(torch.int32), rv.view(torch.int32)), f"{what}: value bits differ"
    assert torch.equal(s & ~1, rs & ~1), f"{what}: status differs beyond bit 0"


def _check(eng, x, k, taken=True):
    """forced dense call against the exhaustive kernel; returns the dense call's status"""
    x = torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else x
    eng.topk_dense = 1
    assert eng.topk_dense == 1
    got = eng.score_topk(x, k, IRS_SWEEP_BF16)
    assert eng.topk_dense_last == taken
    ref = eng.score_topk(x, k, IRS_SWEEP_EXHAUSTIVE)
    torch.cuda.synchronize()
    _same(got, ref, "dense vs exhaustive")
    return got[2].cpu().numpy()


@pytest.mark.parametrize("n_item", [99, 100, 101, 1000, 3415, 4065, 4096])
def test_catalog_sizes(n_item):
    """below k, equal to k, above k, not a multiple of the 32-item tile, the flagship catalog, the last size that fits"""
    d, M, k = 128, 33, 100
    W, b = _weights(n_item, d, 1)
    eng = scoring_only_engine(n_item, d, W, b, max_rows=64)
    st = _check(eng, _rows(M, d, 2), k)
    assert ((st & 4) != 0).all() == (n_item < k)
    if n_item >= 4 * k:
        assert not (st & 1).any(), "a fallback row on benign data"


def test_one_item_too_many_is_not_taken():
    n_item, d, M, k = 4097, 128, 33, 100
    W, b = _weights(n_item, d, 3)
    eng = scoring_only_engine(n_item, d, W, b, max_rows=64)
    _check(eng, _rows(M, d, 4), k, taken=False)


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_widths(d):
    n_item, M, k = 1000, 33, 100
    W, b = _weights(n_item, d, 5)
    eng = scoring_only_engine(n_item, d, W, b, max_rows=64)
    assert not (_check(eng, _rows(M, d, 6), k) & 1).any()


def test_narrow_model_is_not_taken():
    """d = 16 has no full 32-wide k-step: the form needs d_pad >= 32"""
    n_item, d = 1000, 16
    W, b = _weights(n_item, d, 7)
    eng = scoring_only_engine(n_item, d, W, b, max_rows=64)
    _check(eng, _rows(33, d, 8), 100, taken=False)


@pytest.fixture(scope="module")
def flagship():
    n_item, d = 3415, 128
    W, b = _weights(n_item, d, 9)
    return scoring_only_engine(n_item, d, W, b, max_rows=300, max_k=256), W, b


@pytest.mark.parametrize("M", [1, 31, 33, 257])
def test_row_counts(flagship, M):
    """max_rows = 300: padded rows exist behind every M; 257 rows are two row blocks of the sweep"""
    eng = flagship[0]
    assert not (_check(eng, _rows(M, 128, 10 + M), 100) & 1).any()


@pytest.mark.parametrize("k", [1, 100, 256])
def test_list_lengths(flagship, k):
    """k = 256: the bound is the SMALLEST of the 256 per-thread maxima, which keeps more than IRS_REFINE_CAP of 3415 items -- the
    rows are redone exhaustively (bit 0) and still match; auto never takes the form above k = 128"""
    eng = flagship[0]
    st = _check(eng, _rows(33, 128, 20 + k), k)
    if k <= 128:
        assert not (st & 1).any()


def test_second_shard_of_two():
    """rank 1 of world 2: ids carry the shard's item_lo"""
    n_item, d, M, k = 3415, 128, 33, 100
    W, b = _weights(n_item, d, 11)
    eng = scoring_only_engine(n_item, d, W, b, max_rows=64, rank=1, world=2)
    x = torch.from_numpy(_rows(M, d, 12)).cuda()
    _check(eng, x, k)
    ids = eng.score_topk(x, k, IRS_SWEEP_BF16)[1]
    assert eng.topk_dense_last and int(ids.min()) >= eng.item_lo > 0 and int(ids.max()) < eng.item_hi


# ---------------------------------------------------------------- catalogs that stress the bound
def test_all_items_equal():
    """every score ties: the order is by id, every item survives (more than IRS_REFINE_CAP), the row is redone exhaustively"""
    n_item, d, M, k = 3415, 128, 5, 100
    W, b = _weights(n_item, d, 13)
    W[:] = W[0]
    b[:] = 0.25
    eng = scoring_only_engine(n_item, d, W, b, max_rows=64)
    st = _check(eng, _rows(M, d, 14), k)
    assert (st & 1).all()
    ids = eng.score_topk(torch.from_numpy(_rows(M, d, 14)).cuda(), k, IRS_SWEEP_BF16)[1]
    assert torch.equal(ids.cpu(), torch.arange(k).expand(M, k))


def test_copies_of_the_kth_item():
    n_item, d, M, k = 3415, 128, 5, 100
    W, b = _weights(n_item, d, 15)
    x = _rows(M, d, 16)
    eng = scoring_only_engine(n_item, d, W, b, max_rows=64)
    kth = int(eng.score_topk(torch.from_numpy(x).cuda(), k, IRS_SWEEP_EXHAUSTIVE)[1][0, k - 1])
    spots = np.random.default_rng(17).choice(np.setdiff1d(np.arange(n_item), [kth]), 300, replace=False)
    W[spots], b[spots] = W[kth], b[kth]
    eng = scoring_only_engine(n_item, d, W, b, max_rows=64)
    _check(eng, x, k)


def test_masked_items():
    n_item, d, M, k = 3415, 128, 5, 100
    W, b = _weights(n_item, d, 18)
    b[np.random.default_rng(19).choice(n_item, 50, replace=False)] = -np.inf
    eng = scoring_only_engine(n_item, d, W, b, max_rows=64)
    _check(eng, _rows(M, d, 20), k)


@pytest.mark.parametrize("scale", [64.0, 1.0 / 64.0])
def test_scaled_rows(flagship, scale):
    eng = flagship[0]
    assert not (_check(eng, _rows(33, 128, 21) * np.float32(scale), 100) & 1).any()


# ---------------------------------------------------------------- state
def test_call_order_and_switch(flagship):
    """a dense call, a float32 swept call and a carried call on one engine, each equal to a fresh engine's; the switch at 0
    reproduces the five-kernel route at 1100 rows"""
    _, W, b = flagship
    n_item, d, k, M = 3415, 128, 100, 1100
    x = torch.from_numpy(_rows(M, d, 22)).cuda()
    xs = x[:33].contiguous()

    def fresh(mode):
        e = scoring_only_engine(n_item, d, W, b, max_rows=M)
        e.topk_dense = mode
        return e

    eng = fresh(1)
    a1 = eng.score_topk(xs, k, IRS_SWEEP_BF16)
    assert eng.topk_dense_last
    a2 = eng.score_topk(xs, k, IRS_SWEEP_F32)
    assert not eng.topk_dense_last
    a3 = eng.score_topk(xs, k, IRS_SWEEP_BF16, carry=True)
    assert eng.topk_dense_last
    f1 = fresh(1).score_topk(xs, k, IRS_SWEEP_BF16)
    f2 = fresh(1).score_topk(xs, k, IRS_SWEEP_F32)
    f3 = fresh(1).score_topk(xs, k, IRS_SWEEP_BF16, carry=True)
    torch.cuda.synchronize()
    for got, ref in ((a1, f1), (a2, f2), (a3, f3)):
        _same(got, ref, "against a fresh engine")
        assert torch.equal(got[2], ref[2])
    # 1100 rows: switch at 0 (the five-kernel route), at 1, and auto, against the exhaustive kernel
    ref = eng.score_topk(x, k, IRS_SWEEP_EXHAUSTIVE)
    eng.topk_dense = 0
    off = eng.score_topk(x, k, IRS_SWEEP_BF16)
    assert not eng.topk_dense_last and eng.topk_dense == 0
    eng.topk_dense = 1
    on = eng.score_topk(x, k, IRS_SWEEP_BF16)
    assert eng.topk_dense_last
    eng.topk_dense = None
    assert eng.topk_dense == 2
    auto = eng.score_topk(x, k, IRS_SWEEP_BF16)
    torch.cuda.synchronize()
    for got in (off, on, auto):
        _same(got, ref, "1100 rows")
    assert not (off[2] & 1).any() and not (on[2] & 1).any()


# ---------------------------------------------------------------- loops
@pytest.mark.parametrize("d", [16, 32])
def test_generate_paths_at_1100_users(d):
    """the tiny config at 1100 users (above the direct forms): use_graph true and false, the switch at 1 and at 0 -- the same
    paths and status four times.  At the tiny config's own d = 16 the form is not eligible (d_pad >= 32) and the switch must
    change nothing; the same config at d = 32 is the narrowest the form takes."""
    cfg = synth.make_config("tiny", emb_dim=d)
    sd = synth.irn_state_dict(cfg, 1234)
    B, L, P = 1100, cfg.max_len, 4
    eng = make_engine(cfg, sd, max_rows=B)
    g = np.random.default_rng(23)
    seqs = torch.from_numpy(g.integers(1, cfg.n_item + 1, size=(B, L)).astype(np.int64)).cuda()
    users = torch.from_numpy(g.integers(0, cfg.n_user, size=B).astype(np.int64)).cuda()
    out = []
    for mode in (1, 0):
        for use_graph in (False, True):
            eng.topk_dense = mode
            work = seqs.clone()
            hep = torch.full((B,), L - 2, dtype=torch.int32, device=work.device)
            paths, status = eng.generate_paths(work, users, hep, P, k=100, sweep=IRS_SWEEP_BF16, use_graph=use_graph)[:2]
            torch.cuda.synchronize()
            if not use_graph:
                assert eng.topk_dense_last == (mode == 1 and d >= 32)
            out.append((paths.clone(), status.clone(), work))
    for paths, status, work in out[1:]:
        assert torch.equal(paths, out[0][0]) and torch.equal(status, out[0][1]) and torch.equal(work, out[0][2])
