"""-m gpu: the beam search with an end symbol (irs_beam_step_until, irs_beam_search_until, Engine.beam_search_until,
IRSNN.get_seq_in_batch(beam_width=W, beam_stop=...)) against the plain restatement of tests/beam_until_ref.py, against
irs_beam_step, against the reference's goldens (W == 1) and against itself at other check intervals.

The step alone is compared EXACTLY, cum as raw 64-bit patterns: its inputs are multiples of 1/8 with lse_sum = 1, so every
float64 sum is exact and log(1) = 0 on both sides.  The whole search is compared with the CPU restatement by the rule of
tests/test_gpu_beam.py: scores within 2e-4 (float32 log-sum-exp against float64), ids and fin on the prefix of beams whose
reference scores are more than 1e-4 apart.

What the CPU restatement gives on the users chosen below (checked on the CPU, asserted again in the tests), per
(config, W, P): users as indices into the golden file.
  tiny    W 4  P 8  users 2, 6, 10, 0   ALL: 16 / 16 beams in the compared prefixes, 3 of 4 users end with a finished beam;
                                        BEST: 16 / 16, 3 of 4, done after 5, 5, 3 steps (user 0 never: 8)
  tiny    W 32 P 6  users 2, 8, 10, 0   ALL: 128 / 128, 3 of 4;  BEST: 127 / 128, 3 of 4, done after 5, 6, 4, 6 steps
  default W 4  P 8  users 2, 14, 22, 0  ALL: 16 / 16, 3 of 4;    BEST: 16 / 16, 3 of 4, done after 7, 7, 5, 8 steps
  default W 32 P 5  users 10, 22, 30, 1 ALL: 128 / 128, 3 of 4;  BEST: 128 / 128, 3 of 4, done after 3, 2, 3, 5 steps
Under ALL nobody is done before step P on these inputs (a user keeps unfinished beams to the end)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import beam_until_ref
import path_ref
from gpu_util import make_engine, path_only_engine
from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_BEAM_STOP_ALL, IRS_BEAM_STOP_BEST, IRS_SWEEP_BF16, IRS_SWEEP_F32
from influentialrs_amd.engine import IrsError
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NO_CAND = path_ref.NO_CANDIDATE
RULES = [IRS_BEAM_STOP_ALL, IRS_BEAM_STOP_BEST]
KINDS = (np.int64, np.int32, np.float64, np.float32, np.int32)
SENTINELS = (-4242, 77777, 12345.678, -555.0, 9)  # values no step output holds (items >= 0, hep < L, cum in eighths, fin 0 / 1)


@functools.lru_cache(maxsize=None)
def _path_engine(L):
    return path_only_engine(L)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.cpu().numpy()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# --------------------------------------------------------------------------------------------- 1. the step alone
def _eighths(g, lo, hi, size):
    return g.integers(lo * 8, hi * 8 + 1, size=size).astype(np.float64) * 0.125


def _step_case(W, k, L, P, step, seed):
    """Ten users.  Window items come from 6001.., candidates from 1..5000, so a candidate is a survivor unless it is put
    into a window on purpose, and a target is hit only where it is set on purpose.
      0 the target is the first survivor of beam 0              5 every beam finished
      1 the target is the W-th survivor of the last beam        6 fewer than W candidates in all
      2 the target is the (W+1)-th survivor: not chosen (k > W) 7 done on entry, with lists that would change it
      3 finished beams (NaN val / lse rows, negative ids,       8, 9 random: candidates inside the windows, dead and
        paths filled to P) between live and dead ones                finished beams, a hole
      4 a finished beam ties a fresh candidate exactly: beam 0 finished against beam 1's first (the finished one wins, index 0),
        and, W >= 4, beam 2's first against finished beam 3 (the fresh one wins, index 2 W < 3 W)"""
    g = np.random.default_rng(seed)
    B = 10
    seq = g.integers(6001, 9000, size=(B, W, L)).astype(np.int64)
    hep = g.choice(np.array([0, max(0, (L - 2) // 2), max(0, L - 3), L - 2], dtype=np.int32), size=(B, W))
    cum = -_eighths(g, 0, 20, (B, W))
    paths = g.integers(1, 5000, size=(B, W, P)).astype(np.float32)
    paths[:, :, step:] = 0
    fin = np.zeros((B, W), dtype=np.int32)
    done = np.zeros(B, dtype=np.int32)
    ids0 = np.stack([g.permutation(5000)[:k] for _ in range(B * W)]).astype(np.int64)
    val = np.stack([np.sort(g.permutation(4 * k)[:k].astype(np.float32) * 0.125 - 7.0)[::-1] for _ in range(B * W)])
    lmax = _eighths(g, 0, 8, B * W).astype(np.float32)
    lsum = np.ones(B * W, dtype=np.float32)

    def finish(b, j):
        fin[b, j] = 1
        paths[b, j] = 7000 + np.arange(P) + j  # every entry is told apart: a finished beam is copied whole
        row = b * W + j
        val[row], ids0[row], lmax[row], lsum[row] = np.nan, -5, np.nan, np.nan

    for b, j in ((0, 0), (1, W - 1), (2, 0)):  # one beam far ahead of the user's others: the W output beams are its children
        cum[b] -= 100.0
        cum[b, j] = 0.0
    seq[0, 0, L - 1] = ids0[0 * W + 0, 0] + 1
    seq[1, W - 1, L - 1] = ids0[1 * W + W - 1, W - 1] + 1
    if k > W:
        seq[2, 0, L - 1] = ids0[2 * W + 0, W] + 1
    for j in range(W):
        if W >= 3 and j % 3 == 2:
            cum[3, j] = -np.inf
        elif j % 3 == 0 and W > 1:
            finish(3, j)
    cum[4, (4 if W >= 4 else 2):] = -np.inf  # user 4: the beams set here and no others
    if W >= 2:
        finish(4, 0)
        cum[4, 0], cum[4, 1] = -1.0, -0.5
        lmax[4 * W + 1], val[4 * W + 1, 0] = 1.0, 0.5  # -0.5 + (0.5 - 1.0) = -1.0, the finished beam's score
        val[4 * W + 1, 1:] = np.minimum(val[4 * W + 1, 1:], 0.0) - 64.0
    if W >= 4:
        finish(4, 3)
        cum[4, 3], cum[4, 2] = -3.0, -1.0
        lmax[4 * W + 2], val[4 * W + 2, 0] = 2.0, 0.0  # -1.0 + (0.0 - 2.0) = -3.0
        val[4 * W + 2, 1:] = np.minimum(val[4 * W + 2, 1:], 0.0) - 64.0
    for j in range(W):
        finish(5, j)
    cum[6, 1:] = -np.inf
    ids0[6 * W, W // 2] = -1
    done[7] = 1
    paths[7, :, step:] = 4321.0  # garbage at and behind `step` travels too
    if W > 1:
        finish(7, W - 1)
    for b in (8, 9):
        for j in range(W):
            row = b * W + j
            c = int(g.integers(0, min(k, hep[b, j] + 1) + 1))
            seq[b, j, :c] = ids0[row, :c] + 1
            r = g.random()
            if r < 0.2:
                cum[b, j] = -np.inf
            elif r < 0.4 and W > 1:
                finish(b, j)
        if k > 2:
            ids0[b * W + int(g.integers(0, W)), int(g.integers(1, k))] = -1
        seq[b, 0, L - 1] = ids0[b * W, min(k - 1, 1)] + 1
    status = np.array([0, 1, 4, 5, 0, 1, 4, 5, 0, 1], dtype=np.int32)
    return dict(state=(seq, hep, cum, paths, fin), done=done, val=val, ids0=ids0, lse=(lmax, lsum), status=status,
                step=step, P=P)


def _run_step(eng, case, rule, guard=1):
    """irs_beam_step_until on sentinel-filled outputs that carry `guard` more users; checks that inputs and guards are
    untouched and returns (state_out, done, status)."""
    seq = case["state"][0]
    B, W, L = seq.shape
    P = case["P"]
    d_in = tuple(_t(a) for a in case["state"])
    shapes = ((B + guard, W, L), (B + guard, W), (B + guard, W), (B + guard, W, P), (B + guard, W))
    outs = tuple(torch.full(sh, s, dtype=torch.from_numpy(np.zeros(1, dtype=kd)).dtype, device=DEV)
                 for sh, s, kd in zip(shapes, SENTINELS, KINDS))
    d_done = _t(np.concatenate([case["done"], np.full(guard, 6, dtype=np.int32)]))
    d_st = _t(np.concatenate([case["status"], np.full(guard, 8, dtype=np.int32)]))
    d_val, d_ids = _t(case["val"]), _t(case["ids0"])
    lse = tuple(_t(a) for a in case["lse"]) if W > 1 else None
    eng.beam_step_until(d_in, d_val, d_ids, lse, case["step"], rule, tuple(o[:B] for o in outs), d_done[:B], d_st[:B])
    torch.cuda.synchronize()
    for t, a in zip(d_in, case["state"]):
        assert np.array_equal(_bits(_n(t)), _bits(a))  # the input state is read-only
    assert np.array_equal(_bits(_n(d_val)), _bits(case["val"])) and np.array_equal(_n(d_ids), case["ids0"])
    for o, s in zip(outs, SENTINELS):
        assert (_n(o[B:]) == s).all()
    assert (_n(d_done[B:]) == 6).all() and (_n(d_st[B:]) == 8).all()
    return tuple(_n(o[:B]) for o in outs), _n(d_done[:B]), _n(d_st[:B])


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("k_is_w", [True, False])
@pytest.mark.parametrize("W", [1, 2, 4, 17, 32])
@pytest.mark.parametrize("L", [5, 64, 200])
def test_step_equals_the_restatement_exactly(L, W, k_is_w, rule):
    k = W if k_is_w else 100
    P = [1, 5, 64][(W + L) % 3]
    step = [0, P // 2, P - 1][(W + k) % 3]
    case = _step_case(W, k, L, P, step, seed=L * 1000 + W * 10 + k)
    lmax, lsum = case["lse"] if W > 1 else (None, None)
    want, w_done, w_st = beam_until_ref.beam_step_until(case["state"], case["done"], case["val"], case["ids0"], lmax, lsum,
                                                        step, P, rule, case["status"])
    got, g_done, g_st = _run_step(_path_engine(L), case, rule)
    for name, a, b in zip(("seq", "hep", "cum", "paths", "fin"), want, got):
        assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), (name, np.argwhere(a != b)[:8])
    assert np.array_equal(w_done, g_done) and np.array_equal(w_st, g_st)
    _check_scenarios(case, rule, got, g_done, g_st)


def _check_scenarios(case, rule, got, g_done, g_st):
    """The users of _step_case show what its docstring says they show."""
    seq, hep, cum, paths, fin = case["state"]
    o_seq, o_hep, o_cum, o_paths, o_fin = got
    W, step = seq.shape[1], case["step"]
    item = lambda row, c: float(case["ids0"][row, c] + 1)
    assert list(o_fin[0]) == [1] + [0] * (W - 1) and o_paths[0, 0, step] == item(0, 0)
    assert list(o_fin[1]) == [0] * (W - 1) + [1] and o_paths[1, W - 1, step] == item(1 * W + W - 1, W - 1)
    assert not o_fin[2].any() and g_done[2] == 0 and o_paths[2, W - 1, step] == item(2 * W, W - 1)
    assert g_done[0] == (1 if W == 1 or rule == IRS_BEAM_STOP_BEST else 0) and g_done[1] == (1 if W == 1 else 0)
    if W > 1:
        assert (o_paths[3][o_fin[3] == 1][:, -1] >= 7000).all()  # finished beams of user 3 keep their whole path
        t0 = list(o_cum[4]).index(-1.0)
        assert o_cum[4, t0] == o_cum[4, t0 + 1] == -1.0 and o_fin[4, t0] == 1 and o_fin[4, t0 + 1] == 0
        assert np.array_equal(o_paths[4, t0], paths[4, 0]) and o_paths[4, t0 + 1, step] == item(4 * W + 1, 0)
    if W >= 4:
        t1 = list(o_cum[4]).index(-3.0)
        assert o_cum[4, t1 + 1] == -3.0 and o_fin[4, t1] == 0 and o_fin[4, t1 + 1] == 1
        assert o_paths[4, t1, step] == item(4 * W + 2, 0) and np.array_equal(o_paths[4, t1 + 1], paths[4, 3])
    assert (o_fin[5] == 1).all() and g_done[5] == 1 and (np.diff(o_cum[5]) <= 0).all()
    assert sorted(map(tuple, o_paths[5])) == sorted(map(tuple, paths[5]))
    assert np.isfinite(o_cum[6]).sum() == W // 2 and bool(g_st[6] & NO_CAND) == (W == 1)
    for a, b in zip(case["state"], got):  # done on entry: copied through
        assert np.array_equal(_bits(a[7]), _bits(b[7]))
    assert g_done[7] == 1 and g_st[7] == case["status"][7]
    assert not np.isnan(o_cum).any()
    live_open = np.isfinite(o_cum) & (o_fin == 0)
    expect = ~live_open.any(axis=1) | ((o_fin[:, 0] == 1) if rule == IRS_BEAM_STOP_BEST else False)
    expect[7] = True
    assert np.array_equal(g_done, expect.astype(np.int32))


# --------------------------------------------------------------------------------------------- 2. reduction to the plain step
@pytest.mark.parametrize("W,k,L,P,step", [(1, 100, 64, 5, 2), (2, 2, 5, 1, 0), (4, 65, 200, 64, 63), (17, 100, 64, 5, 0),
                                          (32, 100, 200, 7, 3), (32, 32, 5, 5, 4)])
def test_step_without_a_target_hit_is_the_plain_step_bit_for_bit(W, k, L, P, step):
    g = np.random.default_rng(W * 31 + k + L)
    B = 5
    seq = g.integers(6001, 9000, size=(B, W, L)).astype(np.int64)
    hep = g.choice(np.array([0, max(0, (L - 2) // 2), max(0, L - 3), L - 2], dtype=np.int32), size=(B, W))
    cum = -g.random((B, W)) * 20.0
    cum[g.random((B, W)) < 0.25] = -np.inf
    paths = g.integers(1, 5000, size=(B, W, P)).astype(np.float32)
    paths[:, :, step:] = 12345.0
    ids0 = np.stack([g.permutation(5000)[:k] for _ in range(B * W)]).astype(np.int64)
    val = np.stack([np.sort((g.random(k) * 14 - 7).astype(np.float32))[::-1] for _ in range(B * W)])
    for row in range(B * W):
        b, j = divmod(row, W)
        c = int(g.integers(0, min(k, hep[b, j] + 1) + 1))
        seq[b, j, :c] = ids0[row, :c] + 1
    if k > 2:
        ids0[g.integers(0, B * W, size=3), g.integers(1, k, size=3)] = -1
    lse = ((g.random(B * W) * 8).astype(np.float32), (1 + g.random(B * W) * 500).astype(np.float32))
    status = np.array([0, 1, 4, 5, 0], dtype=np.int32)
    eng = _path_engine(L)
    d_in = tuple(_t(a) for a in (seq, hep, cum, paths))
    d_val, d_ids = _t(val), _t(ids0)
    d_lse = tuple(_t(a) for a in lse) if W > 1 else None
    plain = tuple(torch.full_like(t, 3) for t in d_in)
    st_plain = _t(status)
    eng.beam_step(d_in, d_val, d_ids, d_lse, step, plain, st_plain)
    for rule in RULES:
        outs = tuple(torch.full_like(t, 5) for t in d_in) + (torch.full((B, W), 9, dtype=torch.int32, device=DEV),)
        done, st = torch.zeros(B, dtype=torch.int32, device=DEV), _t(status)
        eng.beam_step_until(d_in + (torch.zeros((B, W), dtype=torch.int32, device=DEV),), d_val, d_ids, d_lse, step, rule, outs,
                            done, st)
        torch.cuda.synchronize()
        for a, b in zip(plain, outs[:4]):
            assert np.array_equal(_bits(_n(a)), _bits(_n(b)))
        assert not _n(outs[4]).any() and np.array_equal(_n(st), _n(st_plain))
        assert np.array_equal(_n(done), (~np.isfinite(_n(plain[2])).any(axis=1)).astype(np.int32))


# --------------------------------------------------------------------------------------------- the whole search
_ENG = {}


def _engine(cfgname, rows=128):
    key = (cfgname, rows)
    if key not in _ENG:
        _ENG.clear()  # one catalog resident at a time
        cfg = synth.make_config(cfgname)
        _ENG[key] = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=rows, max_seqs=rows)
    return _ENG[key]


def _inputs(g, src):
    src = np.asarray(src)
    seq = torch.from_numpy(g["seqs"][src]).to(DEV)
    usr = torch.from_numpy(g["users"][src]).to(DEV)
    hep = torch.full((len(src),), g["seqs"].shape[1] - 2, dtype=torch.int32, device=DEV)  # the goldens' gap_len is 0
    return seq, usr, hep


def _search(eng, g, src, W, P, rule, check_every, sweep=IRS_SWEEP_F32):
    """beam_search_until into sentinel-filled outputs; every entry must have been written.  Scores are sums of
    log-probabilities where W > 1; at W == 1 no log-sum-exp is taken and they are sums of raw scores, as irs_beam_search's."""
    seq, usr, hep = _inputs(g, src)
    B = len(src)
    paths = torch.full((B, W, P), -555.0, dtype=torch.float32, device=DEV)
    scores = torch.full((B, W), float("nan"), dtype=torch.float64, device=DEV)
    fin = torch.full((B, W), 9, dtype=torch.int32, device=DEV)
    status = torch.full((B,), 1 << 20, dtype=torch.int32, device=DEV)
    out = eng.beam_search_until(seq, usr, hep, P, W, k=100, sweep=sweep, stop_rule=rule, check_every=check_every,
                                paths=paths, scores=scores, status=status, fin=fin)
    torch.cuda.synchronize()
    paths, scores, status, fin = (_n(t) for t in out[:4])
    assert (paths >= 0).all() and not np.isnan(scores).any() and np.isin(fin, (0, 1)).all() and (status < (1 << 20)).all()
    assert W == 1 or (scores <= 0).all()
    return paths, scores, status, fin, out[4], out[5]


def _finish_step(g, u):
    pos = np.where(g["paths"][u] == g["targets"][u])[0]
    return int(pos[0]) if len(pos) else None


# --------------------------------------------------------------------------------------------- 3. W == 1 through the whole loop
@pytest.mark.parametrize("check_every", [1, 3])
@pytest.mark.parametrize("name,cfgname", [("irn_tiny", "tiny"), ("irn_default", "default"), ("irn_c4d", "c4d")])
def test_one_beam_walks_the_reference_goldens(golden, name, cfgname, check_every):
    g = golden(name)
    B = g["seqs"].shape[0]
    P = int(g["meta"][2])
    live = [P if _finish_step(g, u) is None else _finish_step(g, u) + 1 for u in range(B)]
    for rule in RULES:
        paths, scores, status, fin, steps, window_steps = _search(_engine(cfgname), g, np.arange(B), 1, P, rule, check_every,
                                                                  sweep=IRS_SWEEP_BF16)
        assert np.array_equal(paths[:, 0].view(np.uint32), g["paths"].view(np.uint32))
        assert sorted(np.where(fin[:, 0] == 1)[0].tolist()) == sorted(int(u) for u in g["early_users"])
        assert not status.any() and np.isfinite(scores).all()
        # a user is decoded until the first check at or behind the step that chose its target
        assert window_steps == sum(min(-(-n // check_every) * check_every, P) for n in live)
        assert steps == P  # somebody never arrives
        if check_every == 1:
            assert window_steps == sum(live) < B * P


# --------------------------------------------------------------------------------------------- 4. W > 1 against the CPU restatement
CASES = {("tiny", 4): (8, [2, 6, 10, 0]), ("tiny", 32): (6, [2, 8, 10, 0]),
         ("default", 4): (8, [2, 14, 22, 0]), ("default", 32): (5, [10, 22, 30, 1])}
_REF, _LISTS = {}, {}


def _reference(oracle, golden, cfgname, W, rule):
    """The CPU restatement on the case's users, computed once (the two rules share the decoded windows)."""
    key = (cfgname, W, rule)
    if key not in _REF:
        P, users = CASES[(cfgname, W)]
        g = golden("irn_" + cfgname)
        cfg = synth.make_config(cfgname)
        _REF[key] = beam_until_ref.beam_search_until(oracle, synth.irn_state_dict(cfg, 1234), cfg, g["seqs"][users],
                                                     g["users"][users], P, W, rule, cache=_LISTS.setdefault((cfgname, W), {}))
    return _REF[key]


def _safe_prefix(ref_scores_row):
    nb = int(np.isfinite(ref_scores_row).sum())
    gaps = np.abs(np.diff(ref_scores_row[:nb]))
    return nb if len(gaps) == 0 or gaps.min() > 1e-4 else int(np.argmax(gaps <= 1e-4)) + 1


def _compare(ref, got, rows=None):
    r_paths, r_scores, r_fin = ref[:3]
    paths, scores, _, fin = got[:4]
    rows = range(len(paths)) if rows is None else rows
    for i, b in enumerate(rows):
        assert np.array_equal(np.isfinite(scores[i]), np.isfinite(r_scores[b]))
        ok = np.isfinite(r_scores[b])
        assert np.abs(scores[i][ok] - r_scores[b][ok]).max() <= 2e-4, (b, scores[i], r_scores[b])
        n = _safe_prefix(r_scores[b])
        assert np.array_equal(paths[i, :n], r_paths[b, :n]), (b, paths[i], r_paths[b])
        assert np.array_equal(fin[i, :n], r_fin[b, :n]), (b, fin[i], r_fin[b])


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("cfgname,W", sorted(CASES))
def test_search_matches_the_cpu_restatement(oracle, golden, cfgname, W, rule):
    P, users = CASES[(cfgname, W)]
    ref = _reference(oracle, golden, cfgname, W, rule)
    r_paths, r_scores, r_fin, r_steps = ref
    # what the reference alone must give on these users (module docstring)
    assert sum(_safe_prefix(r_scores[b]) for b in range(len(users))) >= 0.9 * len(users) * W
    assert 2 * int((r_fin.sum(axis=1) > 0).sum()) >= len(users)
    if rule == IRS_BEAM_STOP_BEST:
        assert (r_steps < P).any()
    got = _search(_engine(cfgname), golden("irn_" + cfgname), users, W, P, rule, 1)
    _compare(ref, got)
    assert not got[2].any()
    assert got[4] == int(r_steps.max()) and got[5] == W * int(r_steps.sum())
    assert np.isfinite(got[1]).all() and (np.diff(got[1], axis=1) <= 0).all()  # beam 0 is the best


# --------------------------------------------------------------------------------------------- 5. independence of the checks
@pytest.mark.parametrize("cfgname,W,rows", [("tiny", 4, [0, 1, 2]), ("default", 32, [0, 1, 2])])
def test_result_does_not_depend_on_the_check_interval(oracle, golden, cfgname, W, rows):
    """The users of the case that are done before step P under BEST (module docstring): at check_every = 1 the search ends
    early; at check_every = P nothing is retired before the last step."""
    P, users = CASES[(cfgname, W)]
    ref = _reference(oracle, golden, cfgname, W, IRS_BEAM_STOP_BEST)
    assert (ref[3][rows] < P).all()
    src = [users[r] for r in rows]
    B = len(src)
    g = golden("irn_" + cfgname)
    runs = {ce: _search(_engine(cfgname), g, src, W, P, IRS_BEAM_STOP_BEST, ce) for ce in (1, 2, P)}
    for ce, got in runs.items():
        _compare(ref, got, rows)
        assert np.array_equal(got[2], runs[1][2]), ce
        for i, b in enumerate(rows):
            n = _safe_prefix(ref[1][b])
            assert np.array_equal(got[0][i, :n], runs[1][0][i, :n]) and np.array_equal(got[3][i, :n], runs[1][3][i, :n]), ce
        assert np.abs(got[1] - runs[1][1]).max() <= 2e-4
    assert runs[1][4] <= runs[2][4] <= runs[P][4] and runs[1][5] <= runs[2][5] <= runs[P][5]
    assert (runs[P][4], runs[P][5]) == (P, B * W * P)
    assert runs[1][4] < P and runs[1][5] < B * W * P
    assert runs[1][4] == int(ref[3][rows].max()) and runs[1][5] == W * int(ref[3][rows].sum())


# --------------------------------------------------------------------------------------------- 6. argument checks
def test_bad_arguments_are_refused_before_any_launch(golden):
    g = golden("irn_tiny")
    B, W, P = 3, 4, 5
    seq, usr, hep = _inputs(g, np.arange(B))
    paths = torch.full((B, W, P), -7.0, dtype=torch.float32, device=DEV)
    scores = torch.full((B, W), 2.5, dtype=torch.float64, device=DEV)
    fin = torch.full((B, W), 9, dtype=torch.int32, device=DEV)
    status = torch.full((B,), 1 << 20, dtype=torch.int32, device=DEV)

    def rc(eng, rule=IRS_BEAM_STOP_BEST, ce=1):
        with torch.cuda.device(eng.device):
            r = eng.lib.irs_beam_search_until(eng.h, _ptr(seq), _ptr(usr), _ptr(hep), B, W, P, 100, IRS_SWEEP_BF16, rule, ce,
                                              _ptr(paths), _ptr(scores), _ptr(fin), None, _ptr(status), None, _stream())
        torch.cuda.synchronize()
        return r

    def untouched():
        return (bool((paths == -7.0).all()) and bool((scores == 2.5).all()) and bool((fin == 9).all())
                and bool((status == (1 << 20)).all()))

    eng = _engine("tiny")
    assert rc(eng, rule=2) == -1 and untouched()
    assert rc(eng, rule=-1) == -1 and untouched()
    assert rc(eng, ce=0) == -1 and untouched()
    with pytest.raises(IrsError, match=r"error -1\b.*check_every"):
        eng.beam_search_until(seq, usr, hep, P, W, check_every=0, paths=paths, scores=scores, status=status, fin=fin)
    cfg = synth.make_config("tiny")
    shard = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=32, max_seqs=32, rank=0, world=2)
    assert rc(shard) == -4 and untouched()
    assert rc(eng) == 0 and not untouched()
    # the step: a bad rule and null flags
    L = 10
    pe = _path_engine(L)
    case = _step_case(2, 5, L, 4, 1, seed=3)
    d_in = [_t(a) for a in case["state"]]
    d_out = [torch.full_like(t, 9) for t in d_in]
    d_val, d_ids, d_st, d_done = _t(case["val"]), _t(case["ids0"]), _t(case["status"]), _t(case["done"])
    lmax, lsum = (_t(a) for a in case["lse"])

    def step_rc(rule=0, fin_in=d_in[4], fin_out=d_out[4], done=d_done, lm=lmax):
        r = pe.lib.irs_beam_step_until(pe.h, *(_ptr(t) for t in d_in[:4]), _ptr(fin_in), _ptr(d_val), _ptr(d_ids), _ptr(lm),
                                       _ptr(lsum), 10, 2, 5, 1, 4, rule, *(_ptr(t) for t in d_out[:4]), _ptr(fin_out),
                                       _ptr(done), _ptr(d_st), _stream())
        torch.cuda.synchronize()
        return r
    assert step_rc(rule=2) == -1 and step_rc(fin_in=None) == -1 and step_rc(fin_out=None) == -1
    assert step_rc(done=None) == -1 and step_rc(lm=None) == -1
    assert all((_n(t) == 9).all() for t in d_out) and np.array_equal(_n(d_done), case["done"])
    assert step_rc() == 0


# --------------------------------------------------------------------------------------------- 7. neighbours
def test_captured_beam_graph_and_greedy_until_survive_the_loop(golden):
    g = golden("irn_tiny")
    B, W, P = 4, 4, 6
    src = [2, 6, 10, 0]
    eng = _engine("tiny")
    seq, usr, hep = _inputs(g, src)

    def plain():
        out = eng.beam_search(seq, usr, hep, P, W, use_graph=True, want_windows=True)
        torch.cuda.synchronize()
        return [_n(t) for t in out]
    before = plain()
    first = _search(eng, g, src, W, P, IRS_BEAM_STOP_BEST, 1, sweep=IRS_SWEEP_BF16)
    after = plain()
    for a, b in zip(before, after):
        assert np.array_equal(_bits(a), _bits(b))
    s2, u2, h2 = _inputs(g, np.arange(g["seqs"].shape[0]))
    gp, gst, _, _ = eng.generate_paths_until(s2, u2, h2, int(g["meta"][2]), check_every=1)
    torch.cuda.synchronize()
    assert np.array_equal(_n(gp), g["paths"]) and not _n(gst).any()
    again = _search(eng, g, src, W, P, IRS_BEAM_STOP_BEST, 1, sweep=IRS_SWEEP_BF16)
    for a, b in zip(first[:4], again[:4]):
        assert np.array_equal(_bits(a), _bits(b))
    # users were retired in between (user 0 never arrives, so every step runs: 4 * (5 + 5 + 3 + 6) windows, module docstring)
    assert first[4:] == again[4:] == (P, 76) and first[5] < B * W * P


# --------------------------------------------------------------------------------------------- 8. front end
def test_front_end_returns_beam_zero_and_records_the_stop(golden):
    g = golden("irn_tiny")
    src = [2, 6, 10, 0]
    cfg = synth.make_config("tiny")
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    net.to(DEV)
    irn = IRSNN(cfg, net, DEV).eval()
    seq, usr, _ = _inputs(g, src)
    tgt = torch.from_numpy(g["targets"][src]).to(DEV)
    W, P = 4, 8
    with torch.no_grad():
        plain, _, _, _ = irn.get_seq_in_batch(seq, usr, tgt, P, 0, beam_width=W)
        assert not hasattr(irn, "last_beam_stop")
        paths, tt, hist, early = irn.get_seq_in_batch(seq, usr, tgt, P, 0, beam_width=W, beam_stop="best")
        with pytest.raises(ValueError, match="stop_at_target is not built for beam search"):
            irn.get_seq_in_batch(seq, usr, tgt, P, 0, beam_width=W, stop_at_target=True)
    e_paths, e_scores, _, e_fin, e_steps, e_windows = _search(_engine("tiny"), g, src, W, P, IRS_BEAM_STOP_BEST, 1,
                                                              sweep=IRS_SWEEP_BF16)
    assert paths.dtype == np.float32 and np.array_equal(paths, e_paths[:, 0])
    allp, alls = irn.last_beams
    assert np.array_equal(allp, e_paths) and np.abs(alls - e_scores).max() <= 2e-4
    stop = irn.last_beam_stop
    assert sorted(stop) == ["finished", "steps", "window_steps"]
    assert np.array_equal(stop["finished"], e_fin) and (stop["steps"], stop["window_steps"]) == (e_steps, e_windows)
    assert early == int(e_fin[:, 0].sum()) == 3 and len(hist) == len(src) and np.array_equal(tt, g["targets"][src])
    for b in range(len(src)):  # a finished best beam ends with its target and zeros
        if e_fin[b, 0]:
            pos = int(np.where(paths[b] == g["targets"][src[b]])[0][0])
            assert (paths[b, :pos + 1] > 0).all() and not paths[b, pos + 1:].any()
    assert plain.shape == paths.shape
