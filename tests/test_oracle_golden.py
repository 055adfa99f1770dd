"""not-gpu: the CPU oracle (oracle/) pinned against golden vectors captured by
importing the unmodified reference (tests/golden/make_golden.py).
Tolerances: float32 vs float32 with different accumulation orders, absolute on O(1) decoder
rows / logits, PER CONFIG: 5e-6 at tiny / default / c1 (observed over their 76 golden users:
<= 1.5e-6), 2e-5 at c2 / c3 only (the 6-layer x 200-token d = 128 decoder: 1.04e-5 on one c2 user, 7.1e-6 at c3) and c4d (d = 256: 8.5e-6); ranked ids
order-exact except inside runs of reference scores closer than TAU (rank_check.py), and the
number of users that are id for id identical to the reference is asserted EXACTLY: all of them
except the recorded near-tie users (NEAR_TIE_USERS: c2 user 20, one swap across a 2.4e-7 gap of
the reference's own scores); paths exact."""
import numpy as np
import pytest

from influentialrs_amd import synth
from rank_check import check_ranked

TAU = 1e-5  # reference near-tie width for id comparisons
TOLS = {"tiny": 5e-6, "default": 5e-6, "c1": 5e-6, "c2": 2e-5, "c3": 2e-5, "c4d": 2e-5}  # decoder rows / logits, absolute
NEAR_TIE_USERS = {"irn_c2": {20}}  # users whose top-100 differs from the reference's inside a run of gaps < TAU
# irn_c4d (round 5): C4 / C5's decoder shape -- d = 256, 8 heads, L = 200 -- on an ml-1m-sized catalog (observed 8.5e-6 over 32 users)
IRN = [("irn_tiny", "tiny"), ("irn_default", "default"), ("irn_c1", "c1"), ("irn_c2", "c2"), ("irn_c4d", "c4d")]


def _inputs(g):
    B = g["seqs"].shape[0]
    raws = [g["raw"][i, :g["raw_len"][i]] for i in range(B)]
    return raws, g["seqs"], g["users"], g["targets"], g["labels"]


@pytest.mark.parametrize("name,cfgname", IRN)
def test_irn_decoder_logits_topk(oracle, golden, name, cfgname):
    g = golden(name)
    cfg = synth.make_config(cfgname)
    sd = synth.irn_state_dict(cfg, 1234)
    raws, seqs, users, targets, labels = _inputs(g)
    B, L = seqs.shape
    hep = L - 2
    W, b = sd["project.weight"], sd["project.bias"]
    TOL = TOLS[cfgname]
    if cfgname == "c2":
        B = 8  # keep the CPU suite short (the GPU suite walks all 32)
    strict = 0
    for i in range(B):
        x, ru = oracle.decode(sd, cfg, seqs[i], users[i])
        assert abs(float(ru) - float(g["r_u"][i])) < 1e-6
        assert np.abs(x[hep] - g["x_hep"][i]).max() < TOL
        if "x_full" in g.files:
            assert np.abs(x - g["x_full"][i]).max() < TOL
        s = oracle.score_chain(x[hep], W, b)
        assert np.abs(s[g["probe_ids0"][i]] - g["probe_vals"][i]).max() < TOL
        if "logits_hep" in g.files:
            assert np.abs(s - g["logits_hep"][i]).max() < TOL
        v, ids = oracle.topk(s, 100)
        assert np.abs(v - g["top_vals"][i][:100]).max() < TOL
        strict += check_ranked(ids, g["top_ids0"][i], g["top_gaps"][i], TAU)
    known = len([u for u in NEAR_TIE_USERS.get(name, ()) if u < B])
    assert strict == B - known, f"{strict} of {B} users id-for-id identical to the reference, expected {B - known}"
    if "logits_full" in g.files:  # every row of forward(), tiny config
        lg = oracle.forward_logits(sd, cfg, seqs[0], users[0])
        assert np.abs(lg - g["logits_full"][0]).max() < TOL


@pytest.mark.parametrize("name,cfgname", IRN)
def test_irn_accuracy_and_paths(oracle, golden, name, cfgname):
    g = golden(name)
    cfg = synth.make_config(cfgname)
    sd = synth.irn_state_dict(cfg, 1234)
    raws, seqs, users, targets, labels = _inputs(g)
    n = seqs.shape[0] if cfgname != "c2" else 7  # keep the CPU suite short
    hit, rr, ranks = oracle.accuracy_metrics(sd, cfg, raws[:n], seqs[:n], users[:n], labels[:n], top_k=20, gap_len=0)
    ref_rr = g["rr"][:n]
    assert np.allclose(rr, ref_rr[ref_rr > 0], rtol=0, atol=1e-12)
    assert hit == int((g["hit_users"] < n).sum()) and int(g["hit_count"]) > 0
    P = int(g["meta"][2])
    paths, tg, hs, ne = oracle.get_seq(sd, cfg, seqs[:n], users[:n], targets[:n], max_path_len=P)
    assert np.array_equal(paths, g["paths"][:n])  # tails after an early success are zeroed on both sides
    assert ne == int((g["early_users"] < n).sum()) and int(g["n_early_success"]) > 0


def test_irn_c3_million_items(oracle, golden):
    """1M-item catalog: oracle top-100 and greedy steps against the reference."""
    g = golden("irn_c3")
    cfg = synth.make_config("c3")
    sd = synth.irn_state_dict(cfg, 1234)
    raws, seqs, users, targets, labels = _inputs(g)
    hep = cfg.max_len - 2
    TOL = TOLS["c3"]
    for i in (0, 6):  # 6: an early-success user
        x, _ = oracle.decode(sd, cfg, seqs[i], users[i])
        assert np.abs(x[hep] - g["x_hep"][i]).max() < TOL
        s = oracle.score_chain(x[hep], sd["project.weight"], sd["project.bias"])
        v, ids = oracle.topk(s, 100)
        assert np.abs(v - g["top_vals"][i][:100]).max() < TOL
        check_ranked(ids, g["top_ids0"][i], g["top_gaps"][i], TAU)
    P = int(g["meta"][2])
    sel = [0, 6]
    paths, _, _, ne = oracle.get_seq(sd, cfg, seqs[sel], users[sel], targets[sel], max_path_len=P)
    assert np.array_equal(paths, g["paths"][sel]) and ne == int(np.isin(g["early_users"], sel).sum())


@pytest.mark.parametrize("name,cfgname", [("eval_tiny", "eval_tiny"), ("eval_default", "eval_default")])
def test_evaluator_metrics(oracle, golden, name, cfgname):
    g = golden(name)
    cfg = synth.make_config(cfgname)
    sd = synth.irn_state_dict(cfg, 17, evaluator=True)
    h, d, t, sp, lp = g["histories"], g["new_seqs"], g["targets"], g["start_pos"], g["l_paths"]
    pp = oracle.eval_get_pp(sd, cfg, d, sp, lp)
    assert np.allclose(pp, g["pp"], rtol=2e-6, atol=2e-6)
    irr, ir = oracle.eval_get_rr_increase(sd, cfg, h, d, t)
    assert np.array_equal(ir, g["ir"]) and np.allclose(irr, g["irr"], atol=1e-12)
    tp, ppb, avg, ioi = oracle.eval_get_grad(sd, cfg, h, d, t, sp, lp)
    assert np.allclose(tp, g["t_probs"], rtol=2e-6, atol=2e-6)
    assert np.allclose(ppb, g["p_probs"], rtol=2e-6, atol=2e-6)
    assert np.allclose(avg, g["avg_ps"], atol=5e-6) and np.allclose(ioi, g["iois"], atol=5e-6)


@pytest.mark.parametrize("name,cfgname", [("eval_accuracy_tiny", "eval_tiny"), ("eval_accuracy_default", "eval_default")])
def test_evaluator_accuracy_metrics(oracle, golden, name, cfgname):
    """Evaluator.get_accuracy_metrics_in_batch as the unmodified reference ran it on 8 post-padded rows (make_golden.py:
    accuracy_batch -- a full window, a label inside its own history, labels at rank exactly top_k): the hit count equal, the
    reciprocal ranks equal as reciprocals of integer ranks."""
    g = golden(name)
    cfg = synth.make_config(cfgname)
    sd = synth.irn_state_dict(cfg, 17, evaluator=True)
    seqs = g["seqs"].astype(np.int64)
    assert seqs.shape == (8, cfg.max_len + 1) and (seqs[0] > 0).all() and seqs[1, -1] == 0
    lab1 = seqs[1][seqs[1] > 0][-1]
    assert lab1 in seqs[1][seqs[1] > 0][:-1]  # row 1: the label also occurs in its history
    ranks = {}
    for k in (1, 20):
        for h in (True, False):
            hit, rr, ranks[h] = oracle.eval_accuracy_metrics(sd, cfg, seqs, k, h)
            assert hit == int(g[f"hit_k{k}_h{int(h)}"]), (k, h)
            assert np.array_equal(rr, g[f"rr_k{k}_h{int(h)}"]), (k, h, 1 / rr, 1 / g[f"rr_k{k}_h{int(h)}"])
            assert len(rr) == (7 if h else 8) and hit == int((1 / rr <= k + 0.5).sum())
    # the edges the batch was built for: skipped under use_h only; ranks exactly top_k, and one behind it
    assert ranks[True][1] == 0 and ranks[False][1] > 0
    assert list(ranks[True][[2, 3, 6]]) == [20, 1, 21] and list(ranks[False][[4, 5]]) == [20, 1]


def test_selection_definitions(oracle):
    """top-k / rank total order (score desc, id asc), ties, -0 == +0, k > N."""
    s = np.array([1.0, 3.0, 3.0, -0.0, 0.0, 2.0], dtype=np.float32)
    v, i = oracle.topk(s, 4)
    assert list(i) == [1, 2, 5, 0]
    v, i = oracle.topk(s, 10)
    assert list(i) == [1, 2, 5, 0, 3, 4]
    assert oracle.rank_of(s, 2, []) == 2 and oracle.rank_of(s, 1, []) == 1
    assert oracle.rank_of(s, 4, [1, 1, 7, -1]) == 5  # 2,5,0,3 precede 4 once item 1 is excluded
    x = np.array([1.5, -2.0], dtype=np.float32)
    W = np.array([[1.0, 1.0], [0.5, 0.25]], dtype=np.float32)
    b = np.array([0.25, 0.0], dtype=np.float32)
    assert list(oracle.score_chain(x, W, b)) == [-0.25, 0.25]
    assert oracle.bf16_round(np.array([1.00390625], dtype=np.float32))[0] == 1.0  # ties to even
