"""-m gpu: the path replay (include/irs_hip.h, "path replay"): irs_replay_windows id for id against tests/replay_ref.py,
irs_replay_paths bit for bit against the composition of the public calls on the same chunks and against float64, the invalid
rows, determinism, independence of the bound opt-in state, and the front end: Evaluator.get_path_metrics_in_batch,
harness.evaluate_prob(replay=True) and IRSNN.replay_paths.

Bounds.  Bit for bit wherever both sides run the same launches on the same bytes.  Against float64 and against the goldens: the
tolerances tests/test_gpu_frontend.py applies to the same quantities -- log-probabilities rtol 1e-5 / atol 2e-5, avg_ps 2e-5,
iois 4e-5, irr 1e-12 -- and equal ranks, except under the project's near-tie rule: a rank may differ only where the float64
score of the target has a neighbour outside the window closer than TAU = 2e-5; the accepted rows are listed exactly."""
import numpy as np
import pytest
import torch

import replay_ref as ref
from gpu_util import make_engine, path_only_engine
from influentialrs_amd import harness, synth
from influentialrs_amd._lib import IRS_REPLAY_FULL as FULL
from influentialrs_amd._lib import IRS_REPLAY_SLOT as SLOT
from influentialrs_amd._lib import IRS_ROW_NO_CANDIDATE
from influentialrs_amd.model.evaluator import Evaluator
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
from influentialrs_amd.model.uRS import SampleNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAU = 2e-5
CHUNK = 16


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _rows_of(n_steps):
    """Rows (b, i), i < n_steps[b], user by user."""
    ru = np.repeat(np.arange(len(n_steps)), n_steps).astype(np.int32)
    rs = np.concatenate([np.arange(n) for n in n_steps]).astype(np.int32)
    return ru, rs


# ============================================================================ 1. windows id for id
@pytest.mark.parametrize("L", [3, 12, 64, 300])  # 300: a long-window context (irs_create_ex)
@pytest.mark.parametrize("layout", [SLOT, FULL])
def test_windows_id_for_id(L, layout):
    eng = path_only_engine(L)
    N, B, P = 64, 5, 2 * L + 1  # every step of a path that shifts the whole start window out
    rng = np.random.default_rng(100 * L + layout)
    seq0 = np.zeros((B, L), dtype=np.int64)
    hep0 = rng.integers(0, L - 1, B).astype(np.int32)  # [0, L - 2]
    hep0[0], hep0[1] = 0, L - 2
    n0 = rng.integers(1, L + 1, B)  # [1, L]
    n0[0], n0[1] = 1, L
    for b in range(B):
        if layout == FULL:
            seq0[b, :n0[b]] = rng.integers(1, N + 1, n0[b])
        else:
            seq0[b, :hep0[b] + 1] = rng.integers(1, N + 1, hep0[b] + 1)
            seq0[b, 0] = 0 if hep0[b] > 0 else seq0[b, 0]  # a leading pad
            seq0[b, L - 1] = rng.integers(1, N + 1)
    paths = rng.integers(1, N + 1, (B, P + 2)).astype(np.int64)  # path_ld = P + 2
    ru = np.repeat(np.arange(B), P + 1).astype(np.int32)
    rs = np.tile(np.arange(P + 1), B).astype(np.int32)
    perm = rng.permutation(len(ru))
    ru, rs = ru[perm], rs[perm]
    users = np.arange(10, 10 + B, dtype=np.int64)
    seq, hep, usr, st = (_n(v) for v in eng.replay_windows(layout, _t(seq0), _t(paths), _t(ru), _t(rs), hep0=_t(hep0),
                                                           users=_t(users), P=P))
    w_seq, w_hep, w_st = ref.replay_windows(seq0, hep0, paths, P, N, ru, rs, layout)
    assert not w_st.any() and np.array_equal(st, w_st)
    assert np.array_equal(seq, w_seq), np.where((seq != w_seq).any(1))
    assert np.array_equal(hep, w_hep) and hep.dtype == np.int32 and np.array_equal(usr, users[ru])
    last = (rs == P)
    assert (hep[last] == (L - 1 if layout == FULL else L - 2)).all()
    if layout == FULL or L > 2:
        keep = L if layout == FULL else L - 1
        assert all(np.array_equal(seq[r, :keep], paths[ru[r], P - keep:P]) for r in np.where(last)[0])


# ============================================================================ engines and inputs of the model tests
_CACHE = {}


def _eval_engine(name):
    """(cfg, sd, engine) of an evaluator golden: a causal context, for the FULL layout."""
    if ("eval", name) not in _CACHE:
        cfg = synth.make_config(name)
        sd = synth.irn_state_dict(cfg, 17, evaluator=True)
        _CACHE[("eval", name)] = (cfg, sd, make_engine(cfg, sd, evaluator=True, max_rows=64, max_seqs=64))
    return _CACHE[("eval", name)]


def _irn_engine():
    if "irn" not in _CACHE:
        cfg = synth.make_config("tiny")
        sd = synth.irn_state_dict(cfg, 1234)
        _CACHE["irn"] = (cfg, sd, make_engine(cfg, sd, max_rows=64, max_seqs=64))
    return _CACHE["irn"]


def _eval_case(golden, name):
    g = golden(name)
    h, d, t, sp, lp = (g[k] for k in ("histories", "new_seqs", "targets", "start_pos", "l_paths"))
    P = int(lp.max())
    paths = np.zeros((len(lp), P), dtype=np.int64)
    for b in range(len(lp)):
        paths[b, :lp[b]] = d[b, sp[b]:sp[b] + lp[b]]
    ru, rs = _rows_of(lp)
    return dict(layout=FULL, seq0=np.ascontiguousarray(h[:, :-1]), hep0=None, users=None, targets=t.astype(np.int64), paths=paths,
                ru=ru, rs=rs)


def _irn_case(golden, users=(0, 2, 3, 6, 10, 11), P=8):
    """Greedy paths of the tiny golden's users, replayed in the slot layout: P steps each, and the row after the last."""
    g = golden("irn_tiny")
    src = np.asarray(users)
    seq0 = np.ascontiguousarray(g["seqs"][src])
    paths = np.ascontiguousarray(g["paths"][src][:, :P].astype(np.int64))
    n = np.array([int((p > 0).sum()) for p in paths])  # (a path is zeroed behind its arrival)
    ru, rs = _rows_of(n + 1)
    rs[np.cumsum(n + 1) - 1] = P  # the row after the whole path: no item
    ok = [i for i in range(len(ru)) if rs[i] < P or n[ru[i]] == P]
    return dict(layout=SLOT, seq0=seq0, hep0=np.full(len(src), seq0.shape[1] - 2, dtype=np.int32), users=g["users"][src],
                targets=None, paths=paths, ru=ru[ok], rs=rs[ok])


def _replay(eng, c, chunk=CHUNK, ru=None, rs=None):
    out = eng.replay_paths(c["layout"], _t(c["seq0"]), _t(c["paths"]), _t(c["ru"] if ru is None else ru),
                           _t(c["rs"] if rs is None else rs), hep0=None if c["hep0"] is None else _t(c["hep0"]),
                           users=None if c["users"] is None else _t(c["users"]),
                           targets=None if c["targets"] is None else _t(c["targets"]), chunk=chunk)
    return tuple(_n(v) for v in out)


def _row_items_targets(c):
    P = c["paths"].shape[1]
    items = np.array([c["paths"][b, i] if i < P else 0 for b, i in zip(c["ru"], c["rs"])], dtype=np.int64)
    tg = c["seq0"][c["ru"], -1] if c["targets"] is None else c["targets"][c["ru"]]
    return items, tg


def _host_formula(e, mx, sm):
    return np.float32(np.float64(e) - (np.float64(mx) + np.log(np.float64(sm))))


def _composition(eng, c, chunk=CHUNK):
    """irs_replay_windows -> irs_decode -> the scoring calls -> the host formula, chunk by chunk."""
    items, tg = _row_items_targets(c)
    R = len(c["ru"])
    lp_item, lp_target, rank = np.zeros(R, dtype=np.float32), np.zeros(R, dtype=np.float32), np.zeros(R, dtype=np.int32)
    for r0 in range(0, R, chunk):
        sl = slice(r0, min(R, r0 + chunk))
        seq, hep, usr, st = eng.replay_windows(c["layout"], _t(c["seq0"]), _t(c["paths"]), _t(c["ru"][sl]), _t(c["rs"][sl]),
                                               hep0=None if c["hep0"] is None else _t(c["hep0"]),
                                               users=None if c["users"] is None else _t(c["users"]))
        assert not _n(st).any()
        _, xr, _ = eng.decode(seq, usr, want_x=False, pos=hep)
        e_item = _n(eng.score_gather(xr, _t(items[sl, None] - 1)))[:, 0]
        if c["layout"] == SLOT:
            mx, sm, ts, rk = (_n(v) for v in eng.score_target_trace(xr, seq, hep))
        else:
            ts_t = eng.score_gather(xr, _t(tg[sl, None] - 1))[:, 0].contiguous()
            mx, sm = (_n(v) for v in eng.score_lse(xr))
            L = seq.shape[1]
            keep = torch.arange(L, device=DEV).unsqueeze(0) <= hep.unsqueeze(1)
            excl = torch.where(keep & (seq > 0), seq - 1, torch.full_like(seq, -1))
            rk = _n(eng.score_count_before(xr, ts_t, _t(tg[sl] - 1), excl)) + 1
            ts = _n(ts_t)
        lp_target[sl], rank[sl] = _host_formula(ts, mx, sm), rk
        lp_item[sl] = np.where(items[sl] > 0, _host_formula(e_item, mx, sm), np.float32(0))
    return lp_item, lp_target, rank


# ============================================================================ 2. bit for bit against the public calls
def test_full_layout_equals_composition_bit_for_bit(golden):
    cfg, sd, eng = _eval_engine("eval_tiny")
    c = _eval_case(golden, "eval_tiny")
    assert len(c["ru"]) == 36  # chunk 16: three passes, the last one of 4 rows
    got = _replay(eng, c)
    assert not got[3].any() and got[0].dtype == np.float32 and got[2].dtype == np.int32
    want = _composition(eng, c)
    assert _same_bits(got[:3], want), [np.where(_bits(a) != _bits(b)) for a, b in zip(got[:3], want)]
    assert (got[0] < 0).all() and (got[1] < 0).all() and (got[2] >= 1).all()


def test_slot_layout_equals_composition_bit_for_bit(golden):
    cfg, sd, eng = _irn_engine()
    c = _irn_case(golden)
    assert len(c["ru"]) > 2 * CHUNK and len(c["ru"]) % CHUNK
    got = _replay(eng, c)
    assert not got[3].any()
    want = _composition(eng, c)
    assert _same_bits(got[:3], want), [np.where(_bits(a) != _bits(b)) for a, b in zip(got[:3], want)]
    no_item = c["rs"] == c["paths"].shape[1]
    assert no_item.any() and (got[0][no_item] == 0).all() and (got[0][~no_item] < 0).all() and (got[2] >= 1).all()


# ============================================================================ 3. against float64
def _float64_rows(oracle, sd, cfg, c, evaluator):
    """(logits float64 [R, N], seq, hep) of the case's rows: oracle_np.decode in float64, windows from replay_ref."""
    N = cfg.n_item
    seq, hep, st = ref.replay_windows(c["seq0"], c["hep0"], c["paths"], c["paths"].shape[1], N, c["ru"], c["rs"], c["layout"])
    assert not st.any()
    W, b = sd["project.weight"].astype(np.float64), sd["project.bias"].astype(np.float64)
    logits = np.zeros((len(seq), N))
    for r in range(len(seq)):
        x, _ = oracle.decode(sd, cfg, seq[r], None if evaluator else int(c["users"][c["ru"][r]]), evaluator=evaluator,
                             dtype=np.float64)
        logits[r] = W @ x[hep[r]] + b
    return logits, seq, hep


def _near_tie(logits64, window, target):
    """The float64 score of the target has a neighbour outside the window closer than TAU."""
    hidden = set(int(v) - 1 for v in window if v > 0) | {int(target) - 1}
    others = np.array([j for j in range(len(logits64)) if j not in hidden])
    return bool((np.abs(logits64[others] - logits64[int(target) - 1]) < TAU).any())


def _check_against_float64(got, logits, seq, hep, items, tg, accepted):
    want = ref.replay_rows(logits.astype(np.float32), seq, hep, np.zeros(len(seq), dtype=np.int32), tg, items)
    print("max |lp_item - f64|", np.abs(got[0] - want[0]).max(), "max |lp_target - f64|", np.abs(got[1] - want[1]).max())
    assert np.allclose(got[0], want[0], rtol=1e-5, atol=2e-5) and np.allclose(got[1], want[1], rtol=1e-5, atol=2e-5)
    differ = set(np.where(got[2] != want[2])[0].tolist())
    print("rank rows that differ from float64:", sorted(differ))
    assert all(_near_tie(logits[r], seq[r][:hep[r] + 1], tg[r]) for r in differ), differ
    assert differ == set(accepted), (differ, accepted)


def test_full_layout_against_float64(golden, oracle):
    cfg, sd, eng = _eval_engine("eval_tiny")
    c = _eval_case(golden, "eval_tiny")
    logits, seq, hep = _float64_rows(oracle, sd, cfg, c, True)
    _check_against_float64(_replay(eng, c), logits, seq, hep, *_row_items_targets(c), accepted=())


def test_slot_layout_against_float64(golden, oracle):
    cfg, sd, eng = _irn_engine()
    c = _irn_case(golden, users=(0, 2, 6), P=6)
    logits, seq, hep = _float64_rows(oracle, sd, cfg, c, False)
    _check_against_float64(_replay(eng, c), logits, seq, hep, *_row_items_targets(c), accepted=())


# ============================================================================ 4. the evaluator's front end
def _evaluator(cfgname):
    cfg = synth.make_config(cfgname)
    net = SampleNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 17, evaluator=True).items()})
    net.to(DEV)
    ev = Evaluator(cfg, net, DEV)
    ev.eval()
    return cfg, ev


@pytest.mark.parametrize("name", ["eval_tiny", "eval_default"])
def test_get_path_metrics_in_batch_matches_reference(golden, oracle, name):
    g = golden(name)
    cfg, ev = _evaluator(name)
    h, d, t, sp, lp = (torch.from_numpy(g[k]).to(DEV) for k in ("histories", "new_seqs", "targets", "start_pos", "l_paths"))
    with torch.no_grad():
        h_before = h.clone()
        m = ev.get_path_metrics_in_batch(h, d, t, sp, lp)
        assert torch.equal(h, h_before)
    assert sorted(m) == ["avg_ps", "iois", "ir", "irr", "p_probs", "ranks", "t_probs"]
    assert m["t_probs"].shape == g["t_probs"].shape and m["ranks"].shape == g["t_probs"].shape
    assert np.allclose(m["t_probs"], g["t_probs"], rtol=1e-5, atol=2e-5)
    assert np.allclose(m["p_probs"], g["p_probs"], rtol=1e-5, atol=2e-5)
    assert np.allclose(m["avg_ps"], g["avg_ps"], atol=2e-5) and np.allclose(m["iois"], g["iois"], atol=4e-5)
    live = np.arange(m["ranks"].shape[1])[None, :] < g["l_paths"][:, None]
    assert (m["ranks"][live] >= 1).all() and not m["ranks"][~live].any() and not m["t_probs"][~live].any()
    differ = np.where(m["ir"] != g["ir"])[0]
    print(name, "users whose ir differs from the golden:", differ.tolist())
    if len(differ):  # the near-tie rule, on the two rank rows of those users
        c = _eval_case(golden, name)
        sd = synth.irn_state_dict(cfg, 17, evaluator=True)
        rows = [r for r in range(len(c["ru"])) if c["ru"][r] in differ and c["rs"][r] in (0, g["l_paths"][c["ru"][r]] - 1)]
        sub = dict(c, ru=c["ru"][rows], rs=c["rs"][rows])
        logits, seq, hep = _float64_rows(oracle, sd, cfg, sub, True)
        tg = c["targets"][sub["ru"]]
        for u in differ:
            assert any(_near_tie(logits[k], seq[k][:hep[k] + 1], tg[k]) for k in range(len(rows)) if sub["ru"][k] == u), u
    assert set(differ.tolist()) == set()  # the accepted set
    keep = np.setdiff1d(np.arange(len(g["ir"])), differ)
    assert np.allclose(m["irr"][keep], g["irr"][keep], atol=1e-12)


def test_harness_evaluate_prob_with_replay(golden, tmp_path):
    g = golden("harness_tiny")
    cfg = synth.make_config("tiny")
    cfg.max_path_len = int(g["max_path_len"])
    P = cfg.max_path_len
    np.save(tmp_path / f"paths_d_{P}.npy", g["paths"])
    np.save(tmp_path / f"targets_d_{P}.npy", g["targets"])
    harness._save_ragged(str(tmp_path / "histories.npy"), [g["histories"][i, :g["histories_len"][i]] for i in range(len(g["targets"]))])
    ecfg, ev = _evaluator("eval_tiny")
    ecfg.batch_size = 3
    out = harness.evaluate_prob(cfg, ecfg, ev, DEV, result_dir=str(tmp_path), verbose=False, replay=True)
    _, _, _, _, pp, ii, irr, ir, ap = g["printed"]
    for got, want in ((out["perplexity"], pp), (out["ii"], ii), (out["irr"], irr), (out["ir"], ir), (out["ap"], ap)):
        assert abs(got - want) <= 2e-5 * max(1.0, abs(want)) + 1e-6
    assert out["p_probs"].shape == g["p_probs"].shape and out["t_probs"].shape == g["t_probs"].shape
    assert np.abs(out["p_probs"] - g["p_probs"]).max() < 1e-4 and np.abs(out["t_probs"] - g["t_probs"]).max() < 1e-4
    assert np.load(tmp_path / "p_probs.npy").dtype == np.dtype(str(g["dtypes"][3]))


# ============================================================================ 5. IRSNN.replay_paths
def _irn_front():
    cfg = synth.make_config("tiny")
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    net.to(DEV)
    irn = IRSNN(cfg, net, DEV)
    irn.eval()
    return cfg, irn


def test_front_end_replay_equals_the_search_trace_and_scores_beam_paths(golden, oracle):
    g = golden("irn_tiny")
    cfg, irn = _irn_front()
    seq, u, t = (torch.from_numpy(g[k]).to(DEV) for k in ("seqs", "users", "targets"))
    P = 8
    with torch.no_grad():
        paths, _, _, early = irn.get_seq_in_batch(seq, u, t, P, 0, trace=True)
        tr = irn.last_trace
        rp = irn.replay_paths(seq, u, paths, gap_len=0)
    assert early > 0 and np.array_equal(rp["n_steps"], tr["n_steps"]) and (tr["n_steps"] < P).any()
    for k in ("lp_item", "lp_target"):
        assert rp[k].dtype == np.float32 and np.allclose(rp[k], tr[k], rtol=1e-5, atol=2e-5), k
        assert np.array_equal(rp[k] == 0, tr[k] == 0)
    assert np.allclose(rp["avg_lp_item"], tr["avg_lp_item"], atol=2e-5) and np.allclose(rp["ioi"], tr["ioi"], atol=4e-5)
    differ = np.argwhere(rp["rank_target"] != tr["rank_target"])
    print("rank entries that differ from the search's trace:", differ.tolist())
    assert len(differ) == 0  # the accepted set (near ties between two decoder routes)
    assert np.array_equal(rp["ior"], tr["ior"])
    # beam paths carry no trace: replay them and check two users against float64
    with torch.no_grad():
        bp, _, _, _ = irn.get_seq_in_batch(seq, u, t, P, 0, beam_width=4)
        rb = irn.replay_paths(seq, u, bp, gap_len=0)
    assert not np.array_equal(bp, paths) and (rb["rank_target"][:, 0] >= 1).all()
    sd = synth.irn_state_dict(cfg, 1234)
    users2 = [0, 1]
    items = bp[users2].astype(np.int64)
    n = rb["n_steps"][users2]
    ru, rs = _rows_of(n)
    c = dict(layout=SLOT, seq0=g["seqs"][users2], hep0=np.full(2, cfg.max_len - 2, dtype=np.int32), users=g["users"][users2],
             targets=None, paths=items, ru=ru, rs=rs)
    logits, wseq, whep = _float64_rows(oracle, sd, cfg, c, False)
    got = tuple(np.array([rb[k][users2[b], i] for b, i in zip(ru, rs)]) for k in ("lp_item", "lp_target", "rank_target"))
    _check_against_float64(got, logits, wseq, whep, *_row_items_targets(c), accepted=())


# ============================================================================ 6. invalid rows
@pytest.mark.parametrize("layout", [FULL, SLOT])
def test_invalid_rows_read_zeros_and_leave_the_others_alone(golden, layout):
    if layout == FULL:
        cfg, sd, eng = _eval_engine("eval_tiny")
        c = _eval_case(golden, "eval_tiny")
    else:
        cfg, sd, eng = _irn_engine()
        c = _irn_case(golden)
    clean = _replay(eng, c)
    assert not clean[3].any()
    B, P = c["paths"].shape
    victim = 17  # inside the second pass
    b_v = int(c["ru"][victim])
    kinds = {"user below": (-1, 0), "user above": (B, 0), "step below": (b_v, -1), "step above": (b_v, P + 1)}
    for kind, (b, i) in kinds.items():
        ru, rs = c["ru"].copy(), c["rs"].copy()
        ru[victim], rs[victim] = b, i
        got = _replay(eng, c, ru=ru, rs=rs)
        assert got[3][victim] == IRS_ROW_NO_CANDIDATE and got[0][victim] == 0 and got[1][victim] == 0 and got[2][victim] == 0, kind
        others = np.arange(len(ru)) != victim
        assert not got[3][others].any() and _same_bits([a[others] for a in got[:3]], [a[others] for a in clean[:3]]), kind
    # an item outside the catalog in the forced prefix: the rows behind it are invalid, the rows up to it are not
    bad = dict(c, paths=c["paths"].copy())
    bad["paths"][b_v, 0] = cfg.n_item + 1
    got = _replay(eng, bad)
    hit = (c["ru"] == b_v) & (c["rs"] >= 1)
    assert hit.any() and (got[3][hit] == IRS_ROW_NO_CANDIDATE).all() and not got[3][~hit].any()
    assert not got[0][hit].any() and not got[1][hit].any() and not got[2][hit].any()
    first = (c["ru"] == b_v) & (c["rs"] == 0)  # the row that would force it: a valid window, no item to score
    assert got[0][first] == 0 and _same_bits([got[1][first], got[2][first]], [clean[1][first], clean[2][first]])
    rest = ~hit & ~first
    assert _same_bits([a[rest] for a in got[:3]], [a[rest] for a in clean[:3]])
    if layout == FULL:  # an empty window: an empty history and no forced item -> the single item 1
        e = dict(c, seq0=c["seq0"].copy())
        e["seq0"][b_v] = 0
        ru, rs = np.array([b_v, b_v], dtype=np.int32), np.array([0, 1], dtype=np.int32)
        seq, hep, _, st = (v if v is None else _n(v) for v in eng.replay_windows(FULL, _t(e["seq0"]), _t(e["paths"]), _t(ru), _t(rs)))
        assert st.tolist() == [IRS_ROW_NO_CANDIDATE, 0] and hep.tolist() == [0, 0]
        assert seq[0].tolist() == [1] + [0] * (seq.shape[1] - 1) and seq[1, 0] == e["paths"][b_v, 0] and not seq[1, 1:].any()
        got = _replay(eng, e, ru=ru, rs=rs)
        assert got[3].tolist() == [IRS_ROW_NO_CANDIDATE, 0] and got[2][0] == 0 and got[2][1] >= 1
    else:  # a start hep outside [0, L - 2]
        e = dict(c, hep0=c["hep0"].copy())
        e["hep0"][b_v] = c["seq0"].shape[1] - 1
        got = _replay(eng, e)
        hit = c["ru"] == b_v
        assert (got[3][hit] == IRS_ROW_NO_CANDIDATE).all() and not got[3][~hit].any() and not got[2][hit].any()
        assert _same_bits([a[~hit] for a in got[:3]], [a[~hit] for a in clean[:3]])


# ============================================================================ 7. determinism, 8. the bound opt-in state
def test_two_identical_calls_give_identical_bits_whatever_is_bound(golden):
    cfg, sd, eng = _irn_engine()
    c = _irn_case(golden)
    first = _replay(eng, c)
    assert _same_bits(first, _replay(eng, c))
    whole = _replay(eng, c, chunk=64)  # one pass or five: the same rows (the decoder's route may differ: not bit for bit)
    assert np.array_equal(whole[2], first[2]) and np.allclose(whole[1], first[1], rtol=1e-5, atol=2e-5)
    B = len(c["users"])
    held = eng.bind_path_trace(B, 8)
    excl = eng.bind_exclusions(_t(np.tile(np.arange(40, dtype=np.int64), (B, 1))), no_repeat=True)
    try:
        bound = _replay(eng, c)
    finally:
        eng.unbind_exclusions()
        eng.unbind_path_trace()
    assert _same_bits(first, bound)
    assert not _n(held[0]).any() and not _n(held[2]).any() and excl is not None  # replay wrote nothing into the bound trace
    cfg_e, sd_e, eng_e = _eval_engine("eval_tiny")
    ce = _eval_case(golden, "eval_tiny")
    assert _same_bits(_replay(eng_e, ce), _replay(eng_e, ce))
