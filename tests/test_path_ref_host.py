"""not-gpu: the plain references of tests/path_ref.py tied to the record, so that the GPU tests that lean on them
(test_gpu_path_kernels.py) lean on something checked: the greedy step against the reference's own golden paths, the
beam step against oracle_np.beam_search, keys and merge against the numpy wire-format restatement of
test_dist_gloo.py, the evaluation batch against the reference loader's output (contract golden)."""
import numpy as np
import pytest

import path_ref
from influentialrs_amd import synth
from test_dist_gloo import OracleShardScorer


@pytest.mark.parametrize("name,cfgname,n", [("irn_tiny", "tiny", None), ("irn_default", "default", 6)])
def test_greedy_step_reproduces_reference_paths(oracle, golden, name, cfgname, n):
    """path_ref.path_step driven by the oracle's per-step (vals, ids0) walks the reference's golden paths id for id
    (after the reference's tail-zeroing, influentialRS.py:459-467)."""
    g = golden(name)
    cfg = synth.make_config(cfgname)
    sd = synth.irn_state_dict(cfg, 1234)
    n = g["seqs"].shape[0] if n is None else n
    seqs, users, targets = g["seqs"][:n], g["users"][:n], g["targets"][:n]
    P = int(g["meta"][2])
    B, L = seqs.shape
    trace = oracle.get_seq(sd, cfg, seqs, users, targets, max_path_len=P, return_trace=True)[4]
    by = {(r, i): (vals, ids0) for r, i, _, vals, ids0, _ in trace}
    seq, hep = seqs.copy(), np.full(B, L - 2, dtype=np.int32)
    paths, status = np.zeros((B, P), dtype=np.float32), np.zeros(B, dtype=np.int32)
    for i in range(P):
        val = np.stack([by[(r, i)][0] for r in range(B)])
        ids0 = np.stack([by[(r, i)][1] for r in range(B)])
        seq, hep, paths, status = path_ref.path_step(seq, hep, val, ids0, i, paths, status)
    assert not status.any()
    for r in range(B):
        pos = np.where(paths[r] == targets[r])[0]
        if len(pos):
            paths[r, pos[0] + 1:] = 0
    assert np.array_equal(paths, g["paths"][:n])
    assert (seq[:, -1] == seqs[:, -1]).all() and (hep == L - 2).all()


def test_beam_step_equals_cpu_oracle(oracle):
    """path_ref.beam_step driven by the oracle's decode / top-k / (max, sum exp) equals oracle_np.beam_search on the
    tiny config (beam 4, P 6): paths exact, scores within 1e-12."""
    cfg = synth.make_config("tiny")
    sd = synth.irn_state_dict(cfg, 1234)
    hists = synth.user_histories(8, cfg.n_item, seed=7)
    rows = synth.eval_rows(hists, cfg.n_item, seed=11)[:3]
    _, seqs, users, _, _ = synth.collate_eval_irs(rows, cfg.max_len, gap_len=0)
    B, L = seqs.shape
    W, P, k = 4, 6, 100
    Wt, bias = sd["project.weight"], sd["project.bias"]
    seq = np.repeat(seqs[:, None], W, axis=1)
    hep = np.full((B, W), L - 2, dtype=np.int32)
    cum = np.full((B, W), -np.inf)
    cum[:, 0] = 0.0
    state = (seq, hep, cum, np.zeros((B, W, P), dtype=np.float32))
    status = np.zeros(B, dtype=np.int32)
    for step in range(P):
        val = np.zeros((B * W, k), dtype=np.float32)
        ids0 = np.full((B * W, k), -1, dtype=np.int64)
        mx, sm = np.zeros(B * W, dtype=np.float32), np.ones(B * W, dtype=np.float64)
        for row in range(B * W):
            b, j = divmod(row, W)
            if not state[2][b, j] > -np.inf:
                continue
            x, _ = oracle.decode(sd, cfg, state[0][b, j], users[b])
            s = oracle.score_chain(x[state[1][b, j]], Wt, bias)
            v, i = oracle.topk(s, k)
            val[row, :len(v)], ids0[row, :len(i)] = v, i
            mx[row], sm[row] = oracle.max_sumexp(s)
        state, status = path_ref.beam_step(state, val, ids0, mx, sm, step, P, status)
    op, osc = oracle.beam_search(sd, cfg, seqs, users, max_path_len=P, gap_len=0, beam=W)
    assert not status.any()
    assert np.array_equal(state[3], op)
    assert np.isfinite(osc).all() and np.abs(state[2] - osc).max() <= 1e-12


def _random_lists(g, W, M, k):
    """Lists with few distinct scores (ties across lists), special values, -1 holes anywhere and one empty row."""
    pool = np.array([0.0, -0.0, 1.5, -1.5, 1e-42, -1e-42, np.inf, -np.inf, 3.25, 2.0 ** -126], dtype=np.float32)
    val = pool[g.integers(0, len(pool), size=(W, M, k))]
    ids = g.integers(0, 2 ** 31, size=(W, M, k)).astype(np.int64)
    ids[:, :, 0] = np.arange(W)[:, None]  # small, distinct ids next to the large ones
    ids[g.random((W, M, k)) < 0.2] = -1
    ids[:, M // 2] = -1
    return val, ids


@pytest.mark.parametrize("W,M,k", [(1, 1, 1), (3, 5, 17), (8, 4, 100)])
def test_keys_and_merge_equal_the_wire_format_restatement(W, M, k):
    import torch
    g = np.random.default_rng(W * 1000 + k)
    val, ids = _random_lists(g, W, M, k)
    wire = object.__new__(OracleShardScorer)
    keys = wire.pack_topk(torch.from_numpy(val), torch.from_numpy(ids))
    mine = path_ref.pack_keys(val, ids)
    assert mine.dtype == np.uint64 and np.array_equal(mine, keys.numpy().view(np.uint64))
    ov, oi = wire.merge_topk_keys(keys)
    mv, mi = path_ref.merge(val, ids, k)
    assert np.array_equal(mi, oi.numpy())
    assert np.array_equal(mv.view(np.uint32), ov.numpy().view(np.uint32))
    assert (mi[M // 2] == -1).all() and np.isneginf(mv[M // 2]).all()


def test_merge_of_one_sorted_list_is_the_identity():
    g = np.random.default_rng(3)
    val = np.sort(g.standard_normal((1, 6, 40)).astype(np.float32), axis=2)[:, :, ::-1].copy()
    val[:, :, 10:14] = val[:, :, 10:11]  # a run of equal scores, ids ascending inside it
    ids = np.sort(g.choice(2 ** 31, size=(1, 6, 40), replace=False).astype(np.int64), axis=2)
    ids[:, :, 30:] = -1
    val[:, :, 30:] = -np.inf
    mv, mi = path_ref.merge(val, ids, 40)
    assert np.array_equal(mi, ids[0]) and np.array_equal(mv.view(np.uint32), val[0].view(np.uint32))
    # a shorter output is the head of the list
    mv, mi = path_ref.merge(val, ids, 7)
    assert np.array_equal(mi, ids[0, :, :7]) and np.array_equal(mv, val[0, :, :7])


def test_order_key_is_monotone_and_folds_minus_zero():
    v = np.array([-np.inf, -3.0, -1e-42, -0.0, 0.0, 1e-42, 2.0, np.inf], dtype=np.float32)
    key = path_ref.order_key(v)
    assert key[3] == key[4] and (np.diff(key.astype(np.int64)) >= 0).all() and len(np.unique(key)) == 7


def test_eval_batch_equals_reference_loader(golden):
    """path_ref.build_eval_batch with the contract golden's given targets equals the reference loader's own output
    (the arrays test_gpu_frontend.py compares the kernel with)."""
    g = golden("contract")
    cfg = synth.make_config("default")
    hists = synth.user_histories(12, cfg.n_item, seed=7)
    rows = synth.eval_rows(hists, cfg.n_item, seed=11)
    items = np.concatenate(hists).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int64)
    given = np.array([r[2] for r in rows], dtype=np.int64)
    for gap in (0, 5):
        seq, label, raw, raw_n = path_ref.build_eval_batch(items, offsets, cfg.max_len, 100, gap, given)
        assert np.array_equal(seq, g[f"collate_gap{gap}_seq"])
        assert np.array_equal(seq[:, -1], g[f"collate_gap{gap}_targets"])
        assert np.array_equal(label, g[f"collate_gap{gap}_labels"])
        assert np.array_equal(raw_n, g[f"collate_gap{gap}_raw_len"])
        for i in range(len(rows)):
            assert np.array_equal(raw[i, 100 - raw_n[i]:], g[f"collate_gap{gap}_raw"][i, :raw_n[i]])
            assert not raw[i, :100 - raw_n[i]].any()
