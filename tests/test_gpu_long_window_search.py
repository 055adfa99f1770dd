"""-m gpu: the search kernels behind long windows (256 < max_len <= 1024), against the CPU statements of tests/ (path_ref,
survivors_ref, exclusion_ref) and, for the whole loops, against oracle.get_seq / oracle.beam_search.

The window membership test holds a window in registers, 4 per lane up to 256 slots and 16 per lane beyond (irs_window in
csrc/irs_internal.h).  The inputs are built so that a test which remembers only 256 slots chooses wrongly: the leading candidates of
a row's ranked list are exactly the items of its LAST live window slots -- slots 256 and above wherever the window is that long --
so the first survivor is the candidate behind them.  One row keeps a survivor only at rank 100; one row has a short live window and
the leading candidates in stale slots behind it (they do not count).

Everything is equality (ids, float bits, status words), except float64 beam scores of the whole search (the bound of
test_gpu_beam.py: 2e-4, ids exact where consecutive scores are further apart than 1e-4)."""
import functools

import numpy as np
import pytest
import torch

import exclusion_ref
import path_ref
import survivors_ref
from gpu_util import make_engine, path_only_engine
from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_ROW_RESCUED, IRS_SWEEP_F32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 128  # (path_only_engine: max_k = 128)


@functools.lru_cache(maxsize=None)
def _engine(L, n_item=64):
    return path_only_engine(L, n_item=n_item)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _desc_vals(g, k):
    """k strictly descending float32 scores, multiples of 1/8 (their float64 sums are exact)."""
    return np.sort(g.permutation(4 * k)[:k].astype(np.float32) * 0.125 - 7.0)[::-1].copy()


def _row(g, L, hep, c, k=K, stale=False):
    """A window of distinct items whose last c live slots (hep - c + 1 .. hep) hold the c leading candidates, in a shuffled
    order; stale: they sit behind hep instead (slots 256 and above where the window is that long) and hide nothing."""
    ids0 = g.permutation(5000)[:k].astype(np.int64)
    win = (6001 + g.permutation(3000)[:L]).astype(np.int64)
    lead = ids0[:c][g.permutation(c)] + 1
    if stale:
        lo = max(hep + 1, min(256, L - 1 - c))
        win[lo:lo + c] = lead
    else:
        assert c <= hep + 1
        win[hep - c + 1:hep + 1] = lead
    return win, ids0, _desc_vals(g, k)


def _step_case(L, seed):
    """(seq, hep, val, ids0, expected index of the first survivor) for rows over shifting (hep = L - 2) and growing windows."""
    g = np.random.default_rng(seed)
    plan = [  # (hep, leading candidates in the window, stale)
        (L - 2, min(40, L - 1), False),       # shift; L = 320: slots 279 .. 318
        (L - 2, 100, False),                  # shift; the survivor only at rank 100
        (L - 3, min(64, L - 2), False),       # the last grow
        (min(L - 3, max(256, L - 30)), 7, False),  # grow, the live window ending behind slot 256 where L allows
        (10, min(40, L - 12), True),          # a short live window: the candidates behind it are not in it
        (255 if L > 257 else 200, 3, False),  # the live window ends where the first four registers end
        (L - 2, 0, False),                    # nothing hidden
    ]
    seq, hep, val, ids0, first = [], [], [], [], []
    for he, c, stale in plan:
        w, i, v = _row(g, L, he, c, stale=stale)
        seq.append(w), hep.append(he), ids0.append(i), val.append(v), first.append(0 if stale else c)
    return np.stack(seq), np.array(hep, dtype=np.int32), np.stack(val), np.stack(ids0), first


@pytest.mark.parametrize("L", [257, 320, 1024])
def test_path_step_greedy_sees_the_whole_window(L):
    eng = _engine(L)
    seq, hep, val, ids0, first = _step_case(L, seed=L)
    B = seq.shape[0]
    if L > 300:
        assert np.isin(ids0[0, :40] + 1, seq[0, 256:L - 1]).all(), "the leading candidates sit in slots 256 and above"
        assert np.isin(ids0[1, :100] + 1, seq[1, L - 101:L - 1]).all()
    step, path_ld = 1, 3
    paths = np.full((B, path_ld), 777.0, dtype=np.float32)
    status = np.zeros(B, dtype=np.int32)
    want = path_ref.path_step(seq, hep, val, ids0, step, paths, status)
    d_seq, d_hep, d_paths, d_st = _t(seq), _t(hep), _t(paths), _t(status)
    eng.path_step(d_seq, d_hep, _t(val), _t(ids0), step, d_paths, d_st)
    got = (_n(d_seq), _n(d_hep), _n(d_paths), _n(d_st))
    for name, w, g_ in zip(("seq", "hep", "paths", "status"), want, got):
        assert np.array_equal(w, g_), (name, np.argwhere(w != g_)[:8])
    for r in range(B):  # what that means: the survivor is the candidate behind the hidden ones
        assert got[2][r, step] == ids0[r, first[r]] + 1, r
    assert not got[3].any()
    shifted = hep == L - 2
    assert np.array_equal(got[0][shifted][:, :L - 2], seq[shifted][:, 1:L - 1]) and np.array_equal(got[0][:, L - 1], seq[:, L - 1])


@pytest.mark.parametrize("L", [257, 320, 1024])
def test_path_step_sampled_draws_among_the_survivors_of_the_whole_window(L):
    eng = _engine(L)
    seq, hep, val, ids0, first = _step_case(L, seed=L + 1)
    B = seq.shape[0]
    step, sk = 0, 3
    dists = path_ref.path_step(seq, hep, val, ids0, step, np.zeros((B, 2), np.float32), np.zeros(B, np.int32), sample=True, sample_k=sk)
    outs = []
    for seed in (11, 11, 12, 13, 14, 15, 16, 17):
        d_seq, d_hep = _t(seq), _t(hep)
        d_paths, d_st = _t(np.zeros((B, 2), dtype=np.float32)), _t(np.zeros(B, dtype=np.int32))
        eng.path_step(d_seq, d_hep, _t(val), _t(ids0), step, d_paths, d_st, sample=True, sample_k=sk, seed=seed)
        g_seq, g_hep, g_paths, g_st = _n(d_seq), _n(d_hep), _n(d_paths), _n(d_st)
        assert not g_st.any()
        for r in range(B):
            items, p = dists[r]
            assert items.tolist() == (ids0[r, first[r]:first[r] + sk] + 1).tolist()
            chosen = int(g_paths[r, step])
            assert chosen in items.tolist(), (r, chosen, items)
            w_seq, w_hep = path_ref.advance(seq[r], int(hep[r]), chosen)
            assert np.array_equal(g_seq[r], w_seq) and g_hep[r] == w_hep, r
        outs.append(g_paths[:, step].copy())
    assert np.array_equal(outs[0], outs[1])                      # same seed, same choices
    assert len({o.tobytes() for o in outs}) > 1                  # other seeds, other choices


@pytest.mark.parametrize("W,B", [(1, 5), (4, 3), (32, 2)])
def test_beam_step_sees_the_whole_window(W, B):
    L, P, step = 320, 6, 2
    eng = _engine(L)
    g = np.random.default_rng(100 + W)
    seq = np.zeros((B, W, L), dtype=np.int64)
    hep = np.zeros((B, W), dtype=np.int32)
    cum = np.zeros((B, W), dtype=np.float64)
    paths = g.integers(1, 5000, size=(B, W, P)).astype(np.float32)
    paths[:, :, step:] = 12345.0
    val = np.zeros((B * W, K), dtype=np.float32)
    ids0 = np.zeros((B * W, K), dtype=np.int64)
    shapes = [(L - 2, 40, False), (L - 2, 100, False), (L - 3, 64, False), (270, 7, False), (10, 40, True), (L - 2, K - 2, False)]
    for row in range(B * W):
        b, j = divmod(row, W)
        he, c, stale = shapes[int(g.integers(0, len(shapes)))] if row else shapes[1]
        seq[b, j], ids0[row], val[row] = _row(g, L, he, c, stale=stale)
        hep[b, j] = he
        cum[b, j] = -np.inf if (W > 1 and g.random() < 0.2 and j > 0) else -float(g.integers(0, 160)) * 0.125
    lmax, lsum = (None, None) if W == 1 else (np.zeros(B * W, dtype=np.float32), np.ones(B * W, dtype=np.float32))
    (w_seq, w_hep, w_cum, w_paths), w_st = path_ref.beam_step((seq, hep, cum, paths), val, ids0, lmax, lsum, step, P)
    out = (torch.full((B, W, L), -3, dtype=torch.int64, device=DEV), torch.full((B, W), -3, dtype=torch.int32, device=DEV),
           torch.full((B, W), 3.0, dtype=torch.float64, device=DEV), torch.full((B, W, P), 3.0, dtype=torch.float32, device=DEV))
    st = torch.zeros(B, dtype=torch.int32, device=DEV)
    eng.beam_step((_t(seq), _t(hep), _t(cum), _t(paths)), _t(val), _t(ids0), None if W == 1 else (_t(lmax), _t(lsum)), step, out, st)
    g_seq, g_hep, g_cum, g_paths = (_n(t) for t in out)
    assert np.array_equal(_n(st), w_st)
    live = w_cum > -np.inf
    assert live.any() and np.array_equal(g_cum > -np.inf, live)
    assert np.array_equal(g_cum[live], w_cum[live])              # (multiples of 1/8, norm = 0: the float64 sums are exact)
    assert np.array_equal(g_seq, w_seq) and np.array_equal(g_hep, w_hep)
    assert np.array_equal(g_paths[live], w_paths[live])
    # a membership test that remembers 256 slots chooses otherwise: the statement itself, asked about the first 256 slots only
    (_, _, _, t_paths), _ = path_ref.beam_step((seq, np.minimum(hep, 255), cum, paths), val, ids0, lmax, lsum, step, P)
    assert not np.array_equal(t_paths[..., step], w_paths[..., step])


# ------------------------------------------------------------------------------------------------ the loops on a model
@functools.lru_cache(maxsize=None)
def _model(W=1):
    """tiny at L = 272 with a 2000-item catalog, 12 users: windows of 271 (full), 258, 257, 256, 255 and shorter, pre-padded."""
    cfg = synth.make_config("tiny", max_len=272, n_item=2000)
    sd = synth.irn_state_dict(cfg, 1234)
    L, B = cfg.max_len, 12
    g = np.random.default_rng(272)
    lens = [271, 271, 258, 257, 256, 255, 200, 120, 64, 30, 3, 1]
    seqs = np.zeros((B, L), dtype=np.int64)
    for b, n in enumerate(lens):
        seqs[b, L - 1 - n:L - 1] = g.permutation(cfg.n_item)[:n] + 1
    seqs[:, L - 1] = g.integers(1, cfg.n_item + 1, size=B)
    users = g.integers(0, cfg.n_user, size=B).astype(np.int64)
    eng = make_engine(cfg, sd, max_rows=B * W, max_seqs=B * W)
    return cfg, sd, seqs, users, eng


def _hep(B, L):
    return torch.full((B,), L - 2, dtype=torch.int32, device=DEV)


def test_path_loops_walk_the_oracles_paths(oracle):
    cfg, sd, seqs, users, eng = _model()
    B, L = seqs.shape
    P = 6
    ref, tg, _, _ = oracle.get_seq(sd, cfg, seqs, users, seqs[:, L - 1], max_path_len=P)
    plain = oracle.get_seq(sd, cfg, seqs, users, np.zeros(B, dtype=np.int64), max_path_len=P)[0]  # (no tail zeroing)
    for graph in (False, True):
        paths, st = eng.generate_paths(_t(seqs), _t(users), _hep(B, L), P, sweep=IRS_SWEEP_F32, use_graph=graph)
        assert np.array_equal(_n(paths), plain), graph
        assert not _n(st).any()
    paths, st, steps, row_steps = eng.generate_paths_until(_t(seqs), _t(users), _hep(B, L), P, sweep=IRS_SWEEP_F32)
    assert np.array_equal(_n(paths), ref) and not _n(st).any()
    assert 1 <= steps <= P and row_steps <= B * P


def test_beam_search_walks_the_oracles_beams(oracle):
    W, P = 4, 6
    cfg, sd, seqs, users, eng = _model(W)
    B, L = seqs.shape
    paths, scores, st = eng.beam_search(_t(seqs), _t(users), _hep(B, L), P, W, sweep=IRS_SWEEP_F32)
    paths, scores = _n(paths), _n(scores)
    op, osc = oracle.beam_search(sd, cfg, seqs, users, max_path_len=P, gap_len=0, beam=W)
    assert not _n(st).any()
    assert np.allclose(scores, osc, rtol=0, atol=2e-4), (scores, osc)
    n_exact = 0
    for b in range(B):
        gaps = np.abs(np.diff(osc[b]))
        n_safe = W if gaps.min() > 1e-4 else int(np.argmax(gaps <= 1e-4)) + 1
        assert np.array_equal(paths[b, :n_safe], op[b, :n_safe]), (b, paths[b], op[b])
        n_exact += n_safe
    assert n_exact >= B * W - 4, "the fixture should separate nearly all beams by more than the float32 log-sum-exp noise"


# ------------------------------------------------------------------------------------------------ survivors and exclusions
@pytest.fixture(scope="module")
def starved(oracle):
    """L = 320, n_item = 512, k = 100, d = 32.  Rows:
      0 the window is the row's best 300 items, best last: the top-100 sits in slots 200 .. 299            starved
      1 the best 100 but rank 57, behind 199 of the worst items (slots 199 .. 297)                          untouched at want = 1
      2 a short random window                                                                               untouched
      3 the best 280 items, best last (the top-24 in slots 256 .. 279), grown (hep = 279 < L - 2)           starved"""
    L, n_item, d, M, k = 320, 512, 32, 4, 100
    g = np.random.default_rng(31)
    Wt = ((g.random((n_item, d), dtype=np.float32) * 2 - 1) / np.sqrt(d)).astype(np.float32)
    bias = (g.standard_normal(n_item) * 0.1).astype(np.float32)
    x = g.standard_normal((M, d)).astype(np.float32)
    rank = [oracle.topk(oracle.score_chain(x[m], Wt, bias), n_item) for m in range(M)]
    seq = np.zeros((M, L), dtype=np.int64)
    hep = np.zeros(M, dtype=np.int32)

    def window(m, items):
        seq[m, :len(items)] = items
        hep[m] = len(items) - 1
    window(0, rank[0][1][:300][::-1] + 1)
    window(1, np.concatenate([rank[1][1][-199:], np.delete(rank[1][1][:100], 57)]) + 1)
    window(2, g.permutation(n_item)[:40] + 1)
    window(3, rank[3][1][:280][::-1] + 1)
    seq[:, L - 1] = 1 + np.array([r[1][400] for r in rank])
    cfg = synth.make_config("tiny", n_item=n_item, emb_dim=d, n_heads=1, n_layers=1, max_len=L, ffn_dim=8, n_user=2)
    sd = synth.irn_state_dict(cfg, seed=1)
    sd["project.weight"], sd["project.bias"] = Wt, bias
    eng = make_engine(cfg, sd, max_rows=M, max_seqs=1, max_k=k)
    val, ids, _ = eng.score_topk(_t(x), k, IRS_SWEEP_F32)
    val, ids = _n(val), _n(ids)
    for m in range(M):
        assert np.array_equal(ids[m], rank[m][1][:k]) and val[m].tobytes() == rank[m][0][:k].tobytes()
    return dict(eng=eng, x=x, seq=seq, hep=hep, val=val, ids=ids, rank=rank, n_item=n_item, k=k)


@pytest.mark.parametrize("want", [1, 4])
def test_survivor_pass_over_a_300_item_window(starved, want):
    c = starved
    rank, M = c["rank"], c["x"].shape[0]
    status = np.array([0, 4, 1, 0], dtype=np.int32)
    e_val, e_ids, e_st, rows = survivors_ref.ensure_survivors(c["seq"], c["hep"], c["val"], c["ids"], status, want, lambda m: rank[m])
    assert rows == ([0, 3] if want == 1 else [0, 1, 3])
    v, i, s = _t(c["val"]), _t(c["ids"]), _t(status)
    c["eng"].ensure_survivors(_t(c["x"]), _t(c["seq"]), _t(c["hep"]), v, i, s, want=want)
    val, ids, st = _n(v), _n(i), _n(s)
    assert np.array_equal(ids, e_ids) and np.array_equal(val.view(np.uint32), e_val.view(np.uint32)) and np.array_equal(st, e_st)
    assert ids[0, 0] == rank[0][1][300] and ids[3, 0] == rank[3][1][280] and st[0] == IRS_ROW_RESCUED


def test_exclusions_and_no_repeat_over_a_300_item_window(starved):
    c = starved
    rank, M, n_item, k = c["rank"], c["x"].shape[0], c["n_item"], c["k"]
    g = np.random.default_rng(32)
    excl = np.full((M, 48), -1, dtype=np.int64)
    for m in range(M):  # the items right behind what the window hides, some holes, an id beyond the catalog
        excl[m, :20] = rank[m][1][300:320] if m == 0 else rank[m][1][g.permutation(n_item)[:20]]
        excl[m, 30] = n_item + 5
    excl[1, 21] = rank[1][1][57]  # row 1's only survivor is listed: starved once bound
    eng = c["eng"]
    scratch = eng.bind_exclusions(_t(excl), no_repeat=True)
    try:
        status = np.zeros(M, dtype=np.int32)
        e_val, e_ids, e_st, rows = exclusion_ref.ensure_survivors(c["seq"], c["hep"], c["val"], c["ids"], status, 1, lambda m: rank[m],
                                                                  excl, n_item)
        assert 0 in rows and 1 in rows and 3 in rows
        v, i, s = _t(c["val"]), _t(c["ids"]), _t(status)
        eng.ensure_survivors(_t(c["x"]), _t(c["seq"]), _t(c["hep"]), v, i, s, want=1)
        val, ids, st = _n(v), _n(i), _n(s)
        assert np.array_equal(ids, e_ids) and np.array_equal(val.view(np.uint32), e_val.view(np.uint32)) and np.array_equal(st, e_st)
        assert ids[0, 0] == rank[0][1][320]
        # the step on the rescued lists: the path so far holds each row's best admissible item, which no_repeat drops too
        step, P = 2, 4
        paths = np.zeros((M, P), dtype=np.float32)
        paths[:, 0] = ids[:, 0] + 1
        paths[2, 1] = ids[2, 1] + 1
        e_val2, e_ids2, _, _ = exclusion_ref.ensure_survivors(c["seq"], c["hep"], c["val"], c["ids"], status, 2, lambda m: rank[m],
                                                              excl, n_item)
        st0 = np.zeros(M, dtype=np.int32)
        want = exclusion_ref.path_step(c["seq"], c["hep"], e_val2, e_ids2, step, paths, st0, excl, n_item, no_repeat=True)
        d_seq, d_hep, d_paths, d_st = _t(c["seq"]), _t(c["hep"]), _t(paths), _t(st0)
        eng.path_step(d_seq, d_hep, _t(e_val2), _t(e_ids2), step, d_paths, d_st)
        for name, w, g_ in zip(("seq", "hep", "paths", "status"), want, (_n(d_seq), _n(d_hep), _n(d_paths), _n(d_st))):
            assert np.array_equal(w, g_), (name, np.argwhere(w != g_)[:8])
        assert _n(d_paths)[0, step] == rank[0][1][321] + 1  # 300 in the window, 20 listed, one on the path
    finally:
        eng.unbind_exclusions()
    del scratch


# ------------------------------------------------------------------------------------------------ evaluation batch
@pytest.mark.parametrize("gap_len,raw_len", [(0, 100), (20, 350), (318, 5)])
def test_build_eval_batch_at_320(gap_len, raw_len):
    L, n_item = 320, 600
    eng = _engine(L, n_item)
    g = np.random.default_rng(gap_len + raw_len)
    counts = [0, 1, 2, 256, 257, 319, 320, 321, 600, 3]
    hists = [g.permutation(n_item)[:c].astype(np.int64) + 1 for c in counts]
    items = np.concatenate(hists)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    given = g.integers(1, n_item + 1, size=len(counts)).astype(np.int64)
    w_seq, w_lab, w_raw, w_n = path_ref.build_eval_batch(items, offsets, L, raw_len, gap_len, given)
    seq, tgt, lab, raw, raw_n, st = (_n(t) for t in eng.build_eval_batch(_t(items), _t(offsets), raw_len=raw_len, gap_len=gap_len,
                                                                         targets=_t(given)))
    assert np.array_equal(seq, w_seq) and np.array_equal(tgt, given) and np.array_equal(lab, w_lab)
    assert np.array_equal(raw, w_raw) and np.array_equal(raw_n, w_n) and not st.any()
