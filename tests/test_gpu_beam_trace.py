"""-m gpu: the beam trace (include/irs_hip.h, "beam trace"): irs_beam_search / irs_beam_search_until under irs_bind_beam_trace
against the step-by-step composition of the public calls (decode, irs_score_target_trace, irs_score_topk_lse,
irs_beam_step_linked, irs_beam_trace_carry), against the greedy path trace at W = 1, against the CPU statement of
tests/beam_trace_ref.py on the engine's own dense logits, against float64 and the path replay, the carry kernel's bounds, the
until loop's compaction, the other bound options, the unbind, and IRSNN.get_seq_in_batch(beam_trace=True).

Bounds.  Bit for bit wherever both sides run the same launches on the same bytes (the loop and the composition; W = 1 and the
greedy loop; graph and stream).  Against the CPU statement and against float64: links, paths and ranks exact -- a rank may differ
only under the project's near-tie rule (tests/test_gpu_replay.py: a neighbour outside the window closer than TAU = 2e-5 to the
target's score) -- and log-probabilities within the project's rtol 1e-5 / atol 2e-5.  Where the until loop decodes a compacted
batch (check_every below P) the same tolerance holds between two check intervals.

What the CPU statement gives alone on the grow-then-shift case (hep0 = L - 4, W 4, k 3, P 6, stop rule ALL, users 2, 6, 10, 0, 4
of the tiny golden; asserted again in the test): a finished beam of users 2, 6 and 10 changes its slot, and slot 3 of every user
is dead after step 0 (at most three candidates for four slots; user 4 has two).  On the float64 case (users 0 and 2, W 4, P 8, stop
rule ALL) the first GPU run found no rank entry that differs from the float64 oracle: ACCEPTED_RANKS_VS_FLOAT64 is empty."""
import numpy as np
import pytest
import torch

import beam_trace_ref as ref
import path_ref
import path_trace_ref
from gpu_util import make_engine
from influentialrs_amd import _lib, synth
from influentialrs_amd._lib import IRS_BEAM_STOP_ALL, IRS_BEAM_STOP_BEST, IRS_ROW_RESCUED, IRS_SWEEP_BF16
from influentialrs_amd.engine import IrsError
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet, pick_beam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAU = 2e-5
USERS6 = [0, 2, 3, 6, 10, 11]
P8 = 8
DEAD, COPY = _lib.IRS_BEAM_LINK_DEAD, _lib.IRS_BEAM_LINK_COPY
_ENG = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


def _same_bits(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _engine(rows=128, **cfg_kw):
    key = (rows, tuple(sorted(cfg_kw.items())))
    if key not in _ENG:
        cfg = synth.make_config("tiny", **cfg_kw)
        _ENG[key] = (cfg, make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=rows, max_seqs=rows))
    return _ENG[key][1]


def _inputs(g, src):
    src = np.asarray(src)
    seq = g["seqs"][src]
    return seq, g["users"][src], np.full(len(src), seq.shape[1] - 2, dtype=np.int32)  # the goldens' gap_len is 0


def _loop(eng, seq, usr, hep, W, P, rule=None, check_every=1, k=100, **kw):
    """(paths, scores, status, fin or None, (lp_item, lp_target, rank_target)) of the bound loop, as numpy."""
    if rule is None:
        paths, scores, status, tr = eng.beam_search(_t(seq), _t(usr), _t(hep), P, W, k=k, sweep=IRS_SWEEP_BF16, trace=True, **kw)
        fin = None
    else:
        paths, scores, status, fin, _, _, tr = eng.beam_search_until(_t(seq), _t(usr), _t(hep), P, W, k=k, sweep=IRS_SWEEP_BF16,
                                                                     stop_rule=rule, check_every=check_every, trace=True, **kw)
        fin = _n(fin)
    return _n(paths), _n(scores), _n(status), fin, tuple(_n(a) for a in tr)


def _compose(eng, seq0, usr0, hep0, W, P, rule=None, k=100, ld=None, record=None):
    """The same search from the public calls: decode -> score_target_trace -> score_topk_lse (W = 1: score_topk) ->
    beam_step_linked -> beam_trace_carry, P times.  record (a list): per step, numpy copies of the step's inputs, its dense
    logits and its outputs."""
    B, L = seq0.shape
    ld = P if ld is None else ld
    until = rule is not None
    state = ref.initial_state(seq0, hep0, W, P, until)
    state = [_t(a) for a in state]
    users = _t(np.repeat(usr0, W))
    arrays = [torch.zeros((B, W, ld), dtype=dt, device=DEV) for dt in (torch.float32, torch.float32, torch.int32)]
    done = torch.zeros(B, dtype=torch.int32, device=DEV) if until else None
    status = torch.zeros(B, dtype=torch.int32, device=DEV)
    for i in range(P):
        rows_seq, rows_hep = state[0].view(B * W, L), state[1].view(B * W)
        _, xr, _ = eng.decode(rows_seq, users, want_x=False, pos=rows_hep)
        mx, sm, ts, rk = eng.score_target_trace(xr, rows_seq, rows_hep)
        if W > 1:
            val, ids, _, lmax, lsum = eng.score_topk_lse(xr, k, IRS_SWEEP_BF16)
            lse = (lmax, lsum)
        else:
            val, ids, _ = eng.score_topk(xr, k, IRS_SWEEP_BF16)
            lse = None
        out = [torch.empty_like(t) for t in state]
        done_in = _n(done).copy() if until else None
        link, link_val = eng.beam_step_linked(state, val, ids, lse, i, out, status, done=done,
                                              stop_rule=rule if until else IRS_BEAM_STOP_BEST)
        before = [_n(a).copy() for a in arrays] if record is not None else None
        eng.beam_trace_carry(link, link_val, mx, sm, ts, rk, i, *arrays)
        if record is not None:
            record.append(dict(state_in=[_n(t) for t in state], done_in=done_in, val=_n(val), ids0=_n(ids),
                               lse=None if lse is None else (_n(lmax), _n(lsum)), logits=_n(eng.score_dense(xr)),
                               state_out=[_n(t) for t in out], done_out=_n(done).copy() if until else None, link=_n(link),
                               link_val=_n(link_val), before=before, after=[_n(a).copy() for a in arrays]))
        state = out
    fin = _n(state[4]) if until else None
    return _n(state[3]), _n(state[2]), _n(status), fin, tuple(_n(a) for a in arrays)


def _assert_equal_runs(got, want):
    assert np.array_equal(_bits(got[0]), _bits(want[0])), "paths"
    assert np.array_equal(_bits(got[1]), _bits(want[1])), "scores"
    assert np.array_equal(got[2], want[2]), "status"
    assert (got[3] is None) == (want[3] is None) and (got[3] is None or np.array_equal(got[3], want[3])), "fin"
    assert _same_bits(got[4], want[4]), [np.argwhere(_bits(a) != _bits(b)).tolist()[:5] for a, b in zip(got[4], want[4])]


def _ranks_agree(a, b):
    """Two runs of the same search whose decodes saw other batches (a compacted until loop, users in another order): where the
    recorded lp_target has the same bits the decoder row was the same, and the rank must be; elsewhere it may move at a near
    tie, in few entries."""
    (_, lt_a, rk_a), (_, lt_b, rk_b) = a, b
    differ = rk_a != rk_b
    print("rank entries that differ between the two runs:", np.argwhere(differ).tolist())
    assert not (differ & (_bits(lt_a) == _bits(lt_b))).any() and differ.sum() <= 0.05 * max(1, int((rk_a > 0).sum()))


def _sane(run, W, P):
    """What every trace must look like: dead beams read zero, live columns hold log-probabilities and ranks."""
    paths, scores, _, fin, (lp_i, lp_t, rk) = run
    assert lp_i.dtype == np.float32 and lp_t.dtype == np.float32 and rk.dtype == np.int32 and lp_i.shape == paths.shape[:2] + (lp_i.shape[2],)
    dead = ~(scores > -np.inf)
    assert not lp_i[dead].any() and not lp_t[dead].any() and not rk[dead].any()
    live_cols = (paths > 0) & ~dead[:, :, None]
    assert (lp_i[:, :, :P][live_cols] < 0).all() and (lp_t[:, :, :P][live_cols] < 0).all() and (rk[:, :, :P][live_cols] >= 1).all()
    assert not lp_i[:, :, :P][~live_cols].any() and not rk[:, :, :P][~live_cols].any() and not lp_t[:, :, :P][~live_cols].any()


# ============================================================================ 1. the loop equals the composition, bit for bit
@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("rule", [None, IRS_BEAM_STOP_ALL, IRS_BEAM_STOP_BEST])
def test_loop_equals_composition(golden, W, rule):
    g = golden("irn_tiny")
    eng = _engine()
    seq, usr, hep = _inputs(g, USERS6)
    want = _compose(eng, seq, usr, hep, W, P8, rule)
    got = _loop(eng, seq, usr, hep, W, P8, rule, check_every=P8)  # (nothing is compacted: the same launches on the same bytes)
    _assert_equal_runs(got, want)
    _sane(got, W, P8)
    if rule is None:
        graph = _loop(eng, seq, usr, hep, W, P8, use_graph=True)
        _assert_equal_runs(graph, got)
        plain = eng.beam_search(_t(seq), _t(usr), _t(hep), P8, W, k=100, sweep=IRS_SWEEP_BF16)
    else:
        assert got[3].any(), "somebody arrives"
        plain = eng.beam_search_until(_t(seq), _t(usr), _t(hep), P8, W, k=100, sweep=IRS_SWEEP_BF16, stop_rule=rule, check_every=P8)
        assert np.array_equal(_n(plain[3]), got[3])
    # the trace changes nothing the search returns
    assert np.array_equal(_bits(_n(plain[0])), _bits(got[0])) and np.array_equal(_bits(_n(plain[1])), _bits(got[1]))
    assert np.array_equal(_n(plain[2]), got[2])


# ============================================================================ 2. W = 1 is the greedy trace, bit for bit
def test_one_beam_equals_the_greedy_trace(golden):
    g = golden("irn_tiny")
    eng = _engine()
    seq, usr, hep = _inputs(g, USERS6)
    got = _loop(eng, seq, usr, hep, 1, P8)
    paths, status, tr = eng.generate_paths(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16, trace=True)
    assert np.array_equal(got[0][:, 0], _n(paths)) and not got[2].any() and not _n(status).any()
    assert _same_bits([a[:, 0] for a in got[4]], [_n(a) for a in tr])
    # and the until forms: zero behind the arrival on both sides
    got_u = _loop(eng, seq, usr, hep, 1, P8, IRS_BEAM_STOP_BEST, check_every=P8)
    paths_u, _, _, _, tr_u = eng.generate_paths_until(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16, check_every=P8, trace=True)
    assert np.array_equal(got_u[0][:, 0], _n(paths_u)) and got_u[3].sum() >= 3
    assert _same_bits([a[:, 0] for a in got_u[4]], [_n(a) for a in tr_u])
    _sane(got_u, 1, P8)


# ============================================================================ 3. grow, then shift: the CPU statement on the engine's logits
def _grown(g, src):
    """Windows with two free slots in front of the target: hep0 = L - 4, two growing steps, then shifting ones."""
    s = g["seqs"][np.asarray(src)]
    L = s.shape[1]
    out = np.zeros_like(s)
    out[:, :L - 3] = s[:, 2:L - 1]
    out[:, L - 1] = s[:, L - 1]
    return out, g["users"][np.asarray(src)], np.full(len(src), L - 4, dtype=np.int32)


def _near_tie(logits, window, target):
    hidden = set(int(v) - 1 for v in window if v > 0) | {int(target) - 1}
    others = np.array([j for j in range(len(logits)) if j not in hidden])
    lg = logits.astype(np.float64)
    return bool((np.abs(lg[others] - lg[int(target) - 1]) < TAU).any())


def test_grow_then_shift_against_the_cpu_statement(golden):
    g = golden("irn_tiny")
    eng = _engine()
    src = [2, 6, 10, 0, 4]
    W, k, P, rule = 4, 3, 6, IRS_BEAM_STOP_ALL
    seq, usr, hep = _grown(g, src)
    rec = []
    want = _compose(eng, seq, usr, hep, W, P, rule, k=k, record=rec)
    got = _loop(eng, seq, usr, hep, W, P, rule, check_every=P, k=k)
    _assert_equal_runs(got, want)
    moved, dead_slots = set(), set()
    for i, r in enumerate(rec):
        out, state_out, done_out, status, link, link_val = ref.traced_step(r["before"], r["state_in"], r["done_in"], r["val"], r["ids0"],
                                                                           *(r["lse"]), lambda row: r["logits"][row], i, P, rule)
        for c, (a, b) in enumerate(zip(state_out, r["state_out"])):  # (cum: the device's log() may differ from libm's in the last bit)
            assert np.allclose(a, b, rtol=0, atol=1e-9) if c == 2 else np.array_equal(a, b), (i, c)
        assert np.array_equal(done_out, r["done_out"]) and np.array_equal(link, r["link"]), (i, link, r["link"])
        assert np.array_equal(_bits(link_val), _bits(r["link_val"]))
        assert np.array_equal(out[2], r["after"][2]), (i, np.argwhere(out[2] != r["after"][2]).tolist())
        for c in (0, 1):
            print(f"step {i} array {c}: max |device - statement| {np.abs(out[c] - r['after'][c]).max():.3g}")
            assert np.allclose(r["after"][c], out[c], rtol=1e-5, atol=2e-5) and np.array_equal(r["after"][c] == 0, out[c] == 0)
        B = len(src)
        moved |= {b for b in range(B) for t in range(W) if link[b, t] >= COPY and (link[b, t] & (COPY - 1)) != t}
        dead_slots |= {(b, t) for b in range(B) for t in range(W) if link[b, t] == DEAD}
        if i == 0:
            live = r["state_out"][2] > -np.inf
            assert live[:, :2].all() and (r["state_out"][1][live] == hep[0] + 1).all()  # grown
        if i == 2:
            open_beams = (r["state_out"][2] > -np.inf) & (r["state_out"][4] == 0)
            assert open_beams.any() and (r["state_out"][1][open_beams] == seq.shape[1] - 2).all()  # shifting
    assert moved >= {0, 1, 2} and dead_slots >= {(b, 3) for b in range(len(src))}, (moved, dead_slots)
    _sane(got, W, P)


# ============================================================================ 4. the carry kernel's bounds
@pytest.mark.parametrize("W,P,ld", [(32, 4, 4), (3, 64, 64), (3, 5, 64)])
def test_bounds_of_the_carry_kernel(golden, W, P, ld):
    """W = 32 fills every row of the LDS images; P = ld = 64 every column; ld above P leaves columns that must stay zero."""
    g = golden("irn_tiny")
    eng = _engine()
    seq, usr, hep = _inputs(g, [2, 6, 10, 0][:128 // (W * 2)] if W == 32 else [2, 6, 10])
    B = len(seq)
    want = _compose(eng, seq, usr, hep, W, P, IRS_BEAM_STOP_BEST, ld=ld)
    held = eng.bind_beam_trace(B + 1, W, ld)
    try:
        for a in held[:3]:
            a[B] = 7  # the row of a user beyond B
        out = eng.beam_search_until(_t(seq), _t(usr), _t(hep), P, W, k=100, sweep=IRS_SWEEP_BF16, check_every=P)
        got = (_n(out[0]), _n(out[1]), _n(out[2]), _n(out[3]), tuple(_n(a)[:B] for a in held[:3]))
        assert all((_n(a)[B] == 7).all() for a in held[:3]), "rows of users beyond B are untouched"
    finally:
        eng.unbind_beam_trace()
    _assert_equal_runs(got, want)
    assert not any(a[:, :, P:].any() for a in got[4])


def test_long_window_form(golden):
    """max_len 320: the window image of the linked step takes 16 registers per lane."""
    g = golden("irn_tiny")
    eng = _engine(16, max_len=320)
    src = [2, 6, 10]
    s12 = g["seqs"][src]
    seq = np.zeros((len(src), 320), dtype=np.int64)
    seq[:, -s12.shape[1]:] = s12
    usr, hep = g["users"][src], np.full(len(src), 318, dtype=np.int32)
    W, P = 3, 4
    want = _compose(eng, seq, usr, hep, W, P, IRS_BEAM_STOP_ALL)
    got = _loop(eng, seq, usr, hep, W, P, IRS_BEAM_STOP_ALL, check_every=P)
    _assert_equal_runs(got, want)
    _sane(got, W, P)


# ============================================================================ 5. the until loop and its compaction
def test_until_loop_writes_retired_users_at_their_own_rows(golden):
    g = golden("irn_tiny")
    eng = _engine()
    src = [0, 2, 3, 6, 10, 11]  # users 2, 6, 10 are done early under BEST: the others are compacted
    seq, usr, hep = _inputs(g, src)
    W = 4
    runs = {ce: _loop(eng, seq, usr, hep, W, P8, IRS_BEAM_STOP_BEST, check_every=ce) for ce in (1, 3, P8)}
    base = runs[P8]
    assert base[3][:, 0].sum() >= 3
    for ce in (1, 3):
        got = runs[ce]
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[3], base[3]) and np.array_equal(got[2], base[2]), ce
        _ranks_agree(got[4], base[4])
        for c in (0, 1):
            print(f"check_every {ce} array {c}: max difference {np.abs(got[4][c] - base[4][c]).max():.3g}")
            assert np.allclose(got[4][c], base[4][c], rtol=1e-5, atol=2e-5) and np.array_equal(got[4][c] == 0, base[4][c] == 0)
        _sane(got, W, P8)
    # every user's rows are its own: the same search on the users in another order gives the same rows, permuted
    perm = [5, 0, 4, 1, 3, 2]
    other = _loop(eng, seq[perm], usr[perm], hep[perm], W, P8, IRS_BEAM_STOP_BEST, check_every=1)
    assert np.array_equal(other[0], runs[1][0][perm]) and np.allclose(other[4][0], runs[1][4][0][perm], rtol=1e-5, atol=2e-5)
    _ranks_agree(other[4], tuple(a[perm] for a in runs[1][4]))


# ============================================================================ 6. against float64, the replay and the score
def _walk(run, seq, hep):
    """Every recorded (user, beam, column) of a run with the window its ancestor had there: rebuilt from the beam's own path."""
    paths, scores = run[0], run[1]
    rows = []
    for b in range(paths.shape[0]):
        for j in range(paths.shape[1]):
            if not scores[b, j] > -np.inf:
                continue
            win, he = seq[b].copy(), int(hep[b])
            for i in range(paths.shape[2]):
                item = int(paths[b, j, i])
                if item == 0:
                    break
                rows.append((b, j, i, win.copy(), he, item))
                win, he = path_ref.advance(win, he, item)
    return rows


ACCEPTED_RANKS_VS_FLOAT64 = set()  # (user, beam, column) whose rank differs from float64's, all near ties: recorded from the GPU


def test_against_float64_replay_and_scores(golden, oracle):
    g = golden("irn_tiny")
    cfg = synth.make_config("tiny")
    sd = synth.irn_state_dict(cfg, 1234)
    eng = _engine()
    src = [0, 2]
    seq, usr, hep = _inputs(g, src)
    W = 4
    run = _loop(eng, seq, usr, hep, W, P8, IRS_BEAM_STOP_ALL, check_every=P8)
    paths, scores, _, fin, (lp_i, lp_t, rk) = run
    rows = _walk(run, seq, hep)
    assert len(rows) >= 24 and fin.any()
    Wt, bias = sd["project.weight"].astype(np.float64), sd["project.bias"].astype(np.float64)
    differ = set()
    for b, j, i, win, he, item in rows:
        x, _ = oracle.decode(sd, cfg, win, int(usr[b]), dtype=np.float64)
        logits = Wt @ x[he] + bias
        w_i, w_t, w_r = path_trace_ref.step_values(logits.astype(np.float32), win[:he + 1], win[-1], item)
        assert np.allclose(lp_i[b, j, i], w_i, rtol=1e-5, atol=2e-5) and np.allclose(lp_t[b, j, i], w_t, rtol=1e-5, atol=2e-5), (b, j, i)
        if rk[b, j, i] != w_r:
            assert _near_tie(logits, win[:he + 1], win[-1]), (b, j, i, rk[b, j, i], w_r)
            differ.add((b, j, i))
    print("rank entries that differ from float64:", sorted(differ))
    assert differ == ACCEPTED_RANKS_VS_FLOAT64
    # the replay of the returned beams: every (beam row, step) decoded again
    R = len(rows)
    ru = np.array([b * W + j for b, j, *_ in rows], dtype=np.int32)
    rs = np.array([i for _, _, i, *_ in rows], dtype=np.int32)
    rp = eng.replay_paths(_lib.IRS_REPLAY_SLOT, _t(np.repeat(seq, W, axis=0)), _t(paths.reshape(-1, P8).astype(np.int64)), _t(ru), _t(rs),
                          hep0=_t(np.repeat(hep, W)), users=_t(np.repeat(usr, W)))
    r_i, r_t, r_r, r_st = (_n(a) for a in rp)
    assert not r_st.any() and R == len(r_i)
    mine = [np.array([a[b, j, i] for b, j, i, *_ in rows]) for a in (lp_i, lp_t, rk)]
    assert np.allclose(mine[0], r_i, rtol=1e-5, atol=2e-5) and np.allclose(mine[1], r_t, rtol=1e-5, atol=2e-5)
    print("rank entries that differ from the replay:", np.where(mine[2] != r_r)[0].tolist())
    assert not ((mine[2] != r_r) & (_bits(mine[1]) == _bits(r_t))).any() and (mine[2] != r_r).sum() <= 0.05 * R
    # lp_item is not the score's term, but it sums to the score within the two log-sum-exps' tolerance
    for b in range(len(src)):
        for j in range(W):
            if scores[b, j] > -np.inf:
                n = int((paths[b, j] > 0).sum())
                assert abs(float(lp_i[b, j, :n].astype(np.float64).sum()) - scores[b, j]) <= n * 2e-5, (b, j)


# ============================================================================ 7. with exclusions, no_repeat and exact candidates
def test_with_exclusions_no_repeat_and_exact_candidates(golden):
    g = golden("irn_tiny")
    eng = _engine()
    src = [2, 6, 10, 0]
    seq, usr, hep = _inputs(g, src)
    B, W, P = len(src), 4, 5
    # every user's list: the 120 best items of its first row -- the whole top-100 is excluded, so step 0 is rescued for sure
    _, xr, _ = eng.decode(_t(seq), _t(usr), want_x=False, pos=_t(hep))
    first = _n(eng.score_dense(xr))
    excl = np.argsort(-first.astype(np.float64), axis=1, kind="stable")[:, :120].astype(np.int64)
    kw = dict(exact_candidates=True, exclude=_t(excl), no_repeat=True)
    run = _loop(eng, seq, usr, hep, W, P, None, **kw)
    paths, scores, status, _, (lp_i, lp_t, rk) = run
    assert (status & IRS_ROW_RESCUED).all() and (scores > -np.inf).all()
    plain = eng.beam_search(_t(seq), _t(usr), _t(hep), P, W, k=100, sweep=IRS_SWEEP_BF16, **kw)
    assert np.array_equal(_bits(_n(plain[0])), _bits(paths)) and np.array_equal(_bits(_n(plain[1])), _bits(scores))
    rows = _walk(run, seq, hep)
    assert len(rows) == B * W * P
    # the rows' logits from the engine itself, all windows of a step in one decode
    differ = 0
    for i in range(P):
        at = [r for r in rows if r[2] == i]
        _, xr, _ = eng.decode(_t(np.stack([r[3] for r in at])), _t(np.array([usr[r[0]] for r in at])), want_x=False,
                              pos=_t(np.array([r[4] for r in at], dtype=np.int32)))
        logits = _n(eng.score_dense(xr))
        for (b, j, _, win, he, item), lg in zip(at, logits):
            assert item - 1 not in excl[b] and item not in paths[b, j, :i], "the search honoured the list and its own path"
            w_i, w_t, w_r = path_trace_ref.step_values(lg, win[:he + 1], win[-1], item)  # (the statement knows no list)
            assert np.allclose(lp_i[b, j, i], w_i, rtol=1e-5, atol=2e-5) and np.allclose(lp_t[b, j, i], w_t, rtol=1e-5, atol=2e-5)
            if i == 0:  # the rewritten list's value is the exact score of the item: the sweep's row is this very row
                assert lp_i[b, j, i] < np.float32(np.sort(first[b])[-100] - path_trace_ref.lse64(first[b])), "below the whole top-100"
            if rk[b, j, i] != w_r:
                assert _near_tie(lg, win[:he + 1], win[-1]), (b, j, i, rk[b, j, i], w_r)
                differ += 1
    assert differ <= 0.05 * len(rows)
    # the rank ignores the list: hiding the list's items as well would rank somebody's target higher than the trace says
    assert any(path_trace_ref.target_rank(first[b], list(seq[b, :hep[b] + 1]) + list(excl[b] + 1), seq[b, -1]) < rk[b, 0, 0]
               for b in range(B))


# ============================================================================ 8. refusals while bound, and the unbind
def test_refusals_while_bound_and_unbind_restores_everything(golden):
    g = golden("irn_tiny")
    eng = _engine()
    seq, usr, hep = _inputs(g, USERS6)
    B, W = len(seq), 4
    cfg = synth.make_config("tiny")
    fresh = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=128, max_seqs=128)
    want = [_n(t) for t in fresh.beam_search(_t(seq), _t(usr), _t(hep), P8, W, k=100, sweep=IRS_SWEEP_BF16, use_graph=True)]
    before = [_n(t) for t in eng.beam_search(_t(seq), _t(usr), _t(hep), P8, W, k=100, sweep=IRS_SWEEP_BF16, use_graph=True)]
    greedy = [_n(t) for t in eng.generate_paths(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16)]
    held = eng.bind_beam_trace(B, W, P8)
    try:
        for call in (lambda: eng.generate_paths(_t(seq), _t(usr), _t(hep), P8),
                     lambda: eng.generate_paths_until(_t(seq), _t(usr), _t(hep), P8),
                     lambda: eng.beam_search(_t(seq), _t(usr), _t(hep), P8, 2),            # another width than the bound one
                     lambda: eng.beam_search(_t(seq), _t(usr), _t(hep), P8 + 1, W),        # a longer path than ld
                     lambda: eng.beam_search_until(_t(np.tile(seq, (2, 1))), _t(np.tile(usr, 2)), _t(np.tile(hep, 2)), P8, W)):
            with pytest.raises(IrsError, match=r"irs_bind_beam_trace|the beam trace is bound for \[6, 4, 8\]"):
                call()
        with pytest.raises(IrsError, match=r"error -1\b.*W=2.*the beam trace is bound for"):
            eng.beam_search(_t(seq), _t(usr), _t(hep), P8, 2)
        with pytest.raises(IrsError, match=r"error -4\b.*irs_generate_paths: a beam trace is bound"):
            eng.generate_paths(_t(seq), _t(usr), _t(hep), P8)
        assert not any(_n(a).any() for a in held[:3]), "a refused call launches nothing"
        # bound by hand, the loops record into the bound arrays; a captured step bakes them in
        out = eng.beam_search(_t(seq), _t(usr), _t(hep), P8, W, k=100, sweep=IRS_SWEEP_BF16, use_graph=True)
        assert np.array_equal(_bits(_n(out[0])), _bits(before[0])) and (_n(held[2])[:, 0] >= 1).all()
    finally:
        eng.unbind_beam_trace()
    again = [_n(t) for t in eng.generate_paths(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16)]
    assert all(np.array_equal(a, b) for a, b in zip(greedy, again))
    after = [_n(t) for t in eng.beam_search(_t(seq), _t(usr), _t(hep), P8, W, k=100, sweep=IRS_SWEEP_BF16, use_graph=True)]
    for a, b, c in zip(before, after, want):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(b), _bits(c))
    snapshot = [_n(a).copy() for a in held[:3]]
    eng.beam_search(_t(seq), _t(usr), _t(hep), P8, W)
    assert all(np.array_equal(_n(a), s) for a, s in zip(held[:3], snapshot)), "unbound: the arrays are no longer written"


# ============================================================================ 9. the front end
def test_front_end_fills_last_beam_trace_and_picks_by_target(golden):
    g = golden("irn_tiny")
    cfg = synth.make_config("tiny")
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    net.to(DEV)
    irn = IRSNN(cfg, net, DEV).eval()
    seq, usr, tgt = (torch.from_numpy(g[k]).to(DEV) for k in ("seqs", "users", "targets"))
    B, W, P = seq.shape[0], 4, P8
    with torch.no_grad():
        plain = irn.get_seq_in_batch(seq, usr, tgt, P, 0, beam_width=W)
        assert not hasattr(irn, "last_beam_trace")
        traced = irn.get_seq_in_batch(seq, usr, tgt, P, 0, beam_width=W, beam_trace=True)
        bt = irn.last_beam_trace
        picked = irn.get_seq_in_batch(seq, usr, tgt, P, 0, beam_width=W, beam_trace=True, beam_pick="target")
        bt2 = irn.last_beam_trace
    # the default return is unchanged, with the trace or without
    assert np.array_equal(plain[0], traced[0]) and plain[3] == traced[3] and np.array_equal(plain[1], traced[1])
    assert sorted(bt) == ["lp_item", "lp_target", "n_steps", "paths", "picked", "rank_target", "scores"]
    for k in ("lp_item", "lp_target", "rank_target"):
        assert bt[k].shape == (B, W, P) and np.array_equal(bt[k], bt2[k])
    assert bt["n_steps"].shape == (B, W) and not bt["picked"].any()
    targets = g["targets"]
    for b in range(B):
        for j in range(W):
            n = bt["n_steps"][b, j]
            assert not bt["lp_item"][b, j, n:].any() and not bt["rank_target"][b, j, n:].any()
            assert (bt["lp_item"][b, j, :n] < 0).all() and (bt["rank_target"][b, j, :n] >= 1).all()
            pos = np.where(bt["paths"][b, j] == targets[b])[0]
            assert n == (pos[0] + 1 if len(pos) else P)
    want = pick_beam(bt["paths"], bt["scores"], bt["lp_target"], bt["n_steps"], targets, "target")
    assert np.array_equal(bt2["picked"], want) and np.array_equal(want, ref.pick_beam_ref(bt["paths"], bt["scores"], bt["lp_target"],
                                                                                           bt["n_steps"], targets))
    print("beam_pick=target picks:", want.tolist())
    assert want.any(), "for somebody another beam than beam 0 reaches the target first (the CPU statement: users 0, 3, 4, 6, 8, 10)"
    cut = bt["paths"][np.arange(B), want].copy()
    for b in range(B):
        pos = np.where(cut[b] == targets[b])[0]
        if len(pos):
            cut[b, pos[0] + 1:] = 0
    assert np.array_equal(picked[0], cut) and len(picked) == 4 and picked[0].shape == plain[0].shape
    assert picked[3] >= plain[3]  # nobody arrives later by the pick
