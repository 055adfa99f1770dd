"""-m gpu: the admissible rank (include/irs_hip.h, "admissible rank"): irs_score_target_rank_admissible alone against
tests/admissible_ref.py on the oracle's chain, the slate position of irs_recommend, the loops (stream, captured, until), the
arrival rule on the admissible rank, and the compositions.

Bounds.  The standalone call is compared EXACTLY with the statement evaluated on the oracle's chain for the same x rows; so are
ids, status words and slate positions, and float bits wherever both sides run the same launches on the same bytes.  A value a loop
recorded is compared with the value of another decode of the same window (the until loop compacts; the replay decodes again) by
the until-vs-plain rule of tests/test_gpu_path_trace.py: its _bounds, a rank equal unless the target stands within LOGIT of a
neighbour in the dense logits, at most 5 % of the steps excused -- no looser.

The seed.  arrival_ref.batch(B, 3) with admissible_ref.ml1m_lists(B, 500, seed), no_repeat and exact candidates was walked on the
CPU (oracle_np.decode + score_chain, the best admissible item per step) for the list seeds 0 .. 9, 11 and 12 before one was kept.  The
share of (user, step) cells whose target stands within LOGIT = 1.4e-4 of a neighbour -- the cells the statement alone COULD
excuse -- lies between 3 / 64 and 9 / 64 at B = 8 and between 50 / 768 and 63 / 768 at B = 96: with 500 items that close
together no seed comes to half the 5 % cap.  Seed 2 is kept (3 / 64 = 4.7 % and 55 / 768 = 7.2 %, the smallest larger share).  What
the tests hold to the cap is therefore not that share but the cells that DO differ, each of which must also be such a cell."""
import numpy as np
import pytest
import torch

import admissible_ref as ref
import arrival_ref
import offer_set_ref
import path_ref
import path_trace_ref
from gpu_util import make_engine, path_only_engine
from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_ROW_OFFERED, IRS_SWEEP_BF16
from influentialrs_amd.engine import IrsError, _ptr
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
from test_gpu_path_trace import _bounds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, LIST_SEED = 3, 2
P = arrival_ref.P
NAN = float("nan")


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


# ============================================================================ 1. the kernel alone
N1 = 500
T0, T_LO, T_HI = 250, 100, 400  # 0-based: the twin target and the catalog rows made identical to it, at a lower and a higher id
Z_LO, Z_T, Z_HI = 10, 11, 12    # biases -0, +0, -0: under a zero x row the three tie at zero
ROWS = 9
_ALONE = {}


def _alone(oracle, L, n_item=N1):
    """path_only_engine(L) with the twins and the zero biases written into its catalog, nine x rows (the last one zero, with both
    zeros) and their chain scores over the whole catalog, computed once."""
    key = (L, n_item)
    if key not in _ALONE:
        _ALONE.clear()
        eng = path_only_engine(L, n_item=n_item, max_k=128)
        tw, tb = eng._weights["project.weight"], eng._weights["project.bias"]
        W, b = _n(tw).copy(), _n(tb).copy()
        W[T_LO], W[T_HI], b[T_LO], b[T_HI] = W[T0], W[T0], b[T0], b[T0]
        b[Z_LO], b[Z_T], b[Z_HI] = -0.0, 0.0, -0.0
        tw.copy_(_t(W))
        tb.copy_(_t(b))
        eng.finalize()
        x = np.random.default_rng(L + n_item).standard_normal((ROWS, W.shape[1])).astype(np.float32)
        x[8] = 0.0
        x[8, ::2] = -0.0
        logits = np.stack([oracle.score_chain(x[m], W, b) for m in range(ROWS)])
        _ALONE[key] = (eng, x, logits)
    return _ALONE[key]


def _case(L, M, n_excl, seed, logits, n_item=N1):
    """M <= 9 rows.  Row 0: the twin target, its high twin listed; 1: the target in the list; 2: in the window (a deep slot);
    3: on the path; 4: t = 0; 5: t > n_item; 6: the best item of the catalog; 7: the twin target, its low twin listed; 8: the
    zero x row, its target and the listed item tied at zero.  Lists with -1 holes, repeats (adjacent and far apart once sorted)
    and an id outside the catalog; windows with leading pads, a duplicate and a window that ends early; paths with zeros in
    between and a repeat; one item in the list, the window and the path at once."""
    g = np.random.default_rng(seed)
    seq = np.zeros((M, L), dtype=np.int64)
    seq[:, :L - 1] = g.integers(1, n_item + 1, (M, L - 1))
    seq[:, :3] = 0
    seq[:, 5] = seq[:, 4]
    hep = np.full(M, L - 2, dtype=np.int32)
    hep[min(3, M - 1)] = L // 2
    t = g.integers(1, n_item + 1, M)
    paths = g.integers(1, n_item + 1, (M, 64)).astype(np.float32)
    paths[:, 1::3] = 0
    paths[:, 3] = paths[:, 0]
    paths[:, 6] = seq[:, 8]
    excl = None
    if n_excl:
        excl = g.integers(0, n_item, (M, n_excl)).astype(np.int64)
        if n_excl >= 8:
            excl[:, ::7] = -1
            excl[:, 2] = excl[:, 1]
            excl[:, -1] = excl[:, 1]
            excl[:, 4] = n_item + 3
            paths[:, 9] = excl[:, 1] + 1
            seq[:, 10] = excl[:, 1] + 1
        own = 1 if n_excl >= 8 else 0  # a slot the patterns above leave alone
        for r, j in ((0, T_HI), (7, T_LO), (8, Z_LO)):
            if r < M:
                excl[r, own if r else min(3, n_excl - 1)] = j
        if M > 1:
            t[1] = excl[1, own] + 1
    deep = L - 5
    for r, tr in ((0, T0 + 1), (4, 0), (5, n_item + 1), (6, int(np.argmax(logits[6])) + 1), (7, T0 + 1), (8, Z_T + 1)):
        if r < M:
            t[r] = tr
    seq[:, L - 1] = t
    if M > 2:
        seq[2, deep] = t[2]
    if M > 3:
        paths[3, 0] = t[3]
    return seq, hep, excl, paths


def _run(eng, x, seq, hep, excl, paths, step, no_repeat=False, offer_raw=None):
    """The standalone call under the case's bindings, twice; returns the five arrays of the first call."""
    M = len(seq)
    keep = eng.bind_exclusions(_t(excl), no_repeat=no_repeat) if excl is not None else None
    held = None
    if offer_raw is not None:  # (bound as the C caller binds it: the array as it is, holes and all)
        t_raw = _t(offer_raw)
        held = torch.empty(eng.offer_set_scratch_bytes(len(offer_raw), M), dtype=torch.uint8, device=DEV)
        eng._call_null(eng.lib.irs_bind_offer_set, _ptr(t_raw), len(offer_raw), _ptr(held), held.numel(), tensors=(t_raw, held))
    try:
        args = (_t(x[:M]), _t(seq), _t(hep), None if paths is None else _t(paths), step)
        out = [_n(v) for v in eng.score_target_rank_admissible(*args)]
        again = [_n(v) for v in eng.score_target_rank_admissible(*args)]
        trace = [_n(v) for v in eng.score_target_trace(*args[:3])]
    finally:
        if offer_raw is not None:
            eng.unbind_offer_set()
        if keep is not None:
            eng.unbind_exclusions()
    del keep, held
    assert _same_bits(out, again)
    assert _same_bits(out[:4], trace)  # irs_score_target_trace's launches, with its results
    return out


def _check(out, logits, seq, hep, excl, paths, step, offer=None):
    M, L = seq.shape
    mx, sm, ts, rank, adm = out
    assert adm.dtype == np.int32 and adm.shape == (M,)
    want_rank = np.array([path_trace_ref.target_rank(logits[m], seq[m, :hep[m] + 1], seq[m, L - 1]) for m in range(M)], dtype=np.int32)
    assert np.array_equal(rank, want_rank)
    want = ref.rows(logits[:M], seq, hep, excl, paths, step, offer)
    assert np.array_equal(adm, want), (adm, want)
    assert ((adm == 0) == (want_rank == 0)).all()
    if offer is None:
        assert (adm <= rank).all()
    return want, want_rank


# (L, M, list length, step): every M, list length and step of the issue at both window lengths
ALONE = [(L, M, n, s) for L in (50, 320) for M, n, s in ((1, 0, 0), (4, 1, 1), (5, 63, 63), (9, 64, 0), (9, 65, 1), (9, 257, 63), (9, 0, 63))]


@pytest.mark.parametrize("L,M,n_excl,step", ALONE)
def test_kernel_alone(oracle, L, M, n_excl, step):
    eng, x, logits = _alone(oracle, L)
    seq, hep, excl, paths = _case(L, M, n_excl, 7 * L + M + n_excl, logits)
    out = _run(eng, x, seq, hep, excl, paths, step, no_repeat=bool(n_excl & 1))
    want, want_rank = _check(out, logits, seq, hep, excl, paths, step)
    if M == ROWS:
        assert want[4] == 0 and want[5] == 0 and want[6] == 1  # no target twice, and the best of the catalog (nothing is scored)
        if n_excl >= 8:
            assert (want < want_rank).sum() >= 3
            # the twins: the listed low twin no longer stands before the target, the listed high twin never did
            for r, twin, gain in ((7, T_LO, 1), (0, T_HI, 0)):
                less = excl.copy()
                less[r][less[r] == twin] = -1
                if twin + 1 not in seq[r, :hep[r] + 1] and not (step and twin + 1 in paths[r, :step]):
                    assert ref.rows(logits[:M], seq, hep, less, paths, step)[r] == want[r] + gain, r
        if L > 256:  # hidden items in window slots >= 256 count
            short = ref.rows(logits[:M], seq, np.minimum(hep, 255), excl, paths, step)
            assert (short != want).any()
    if step == 63 and M > 3:  # the path enters H, `step` entries of it
        assert not np.array_equal(ref.rows(logits[:M], seq, hep, excl, None, 0), want)


def test_kernel_alone_longest_list(oracle):
    n_item = 5000
    eng, x, logits = _alone(oracle, 50, n_item)
    seq, hep, excl, paths = _case(50, 4, 4096, 99, logits, n_item)
    assert len(set(excl[0][(excl[0] >= 0) & (excl[0] < n_item)].tolist())) > 2048
    out = _run(eng, x, seq, hep, excl, paths, 63, no_repeat=True)
    want, want_rank = _check(out, logits, seq, hep, excl, paths, 63)
    assert (want[:4] < want_rank[:4]).sum() >= 3


OFFERS = [(50, 1, False), (50, 64, True), (320, 65, True), (50, 65, False)]


@pytest.mark.parametrize("L,C,holes", OFFERS)
def test_kernel_alone_with_an_offer_set(oracle, L, C, holes):
    eng, x, logits = _alone(oracle, L)
    M, step = ROWS, 1
    seq, hep, excl, paths = _case(L, M, 65, 1000 + C + L, logits)
    # the twin target stays outside the set (rows 0 and 7); members of H, the low twin and the zero trio go inside
    inside = ({int(excl[3, 1]), int(seq[3, 12]) - 1, T_LO, Z_LO, Z_T, Z_HI} - {T0}) if C > 1 else set()
    pool = np.array([j for j in range(N1) if j != T0 and j not in inside])
    raw = np.array(sorted(inside | set(np.random.default_rng(C).permutation(pool)[:C - len(inside)].tolist())), dtype=np.int64)
    assert len(raw) == C
    if holes:
        raw[5], raw[20], raw[41] = -1, raw[19], N1 + 7  # a hole, a repeat, and an id outside the catalog (its successor falls too)
    san, n_holes = offer_set_ref.sanitise(raw, N1)
    assert (n_holes > 0) == holes and T0 not in san.tolist()
    out = _run(eng, x, seq, hep, excl, paths, step, offer_raw=raw)
    valid = san[san >= 0]
    want, _ = _check(out, logits, seq, hep, excl, paths, step, offer=valid)
    members = [{int(v) - 1 for v in seq[m, :hep[m] + 1]} | set(excl[m].tolist()) for m in range(M)]
    assert any(h - set(valid.tolist()) for h in members)  # union members outside the set ...
    assert C == 1 or any(h & set(valid.tolist()) for h in members)  # ... and inside it
    assert want[0] >= 1 and want[7] >= 1  # a target outside the set still has its rank


def test_poisoned_outputs_and_untouched_inputs(oracle):
    eng, x, logits = _alone(oracle, 50)
    M, extra = 5, 3
    seq, hep, excl, paths = _case(50, M + extra, 65, 5, logits)
    poison_f = np.array([0xDEADBEEF], dtype=np.uint32).view(np.float32)[0]
    f = [torch.full((M + extra,), float(poison_f), device=DEV) for _ in range(3)]
    i = [torch.full((M + extra,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) for _ in range(2)]
    tx, ts, th, tp = _t(x[:M + extra]), _t(seq), _t(hep), _t(paths)
    before = [_n(v).copy() for v in (tx, ts, th, tp)]
    t_scr = torch.empty(eng.path_trace_scratch_bytes(M), dtype=torch.uint8, device=DEV)
    scr = torch.empty(eng.admissible_scratch_bytes(M), dtype=torch.uint8, device=DEV)
    keep = eng.bind_exclusions(_t(excl))
    try:
        eng._call_null(eng.lib.irs_score_target_rank_admissible, _ptr(tx), _ptr(ts), _ptr(th), M, _ptr(tp), 64, 63, _ptr(t_scr),
                       t_scr.numel(), _ptr(scr), scr.numel(), _ptr(f[0]), _ptr(f[1]), _ptr(f[2]), _ptr(i[0]), _ptr(i[1]),
                       tensors=(tx, ts, th, tp, t_scr, scr, *f, *i))
        got = [_n(v) for v in f + i]
    finally:
        eng.unbind_exclusions()
    del keep
    for a in got[:3]:
        assert (a[M:].view(np.uint32) == 0xDEADBEEF).all()
    for a in got[3:]:
        assert (a[M:] == 0x5A5A5A5A).all()
    assert _same_bits([_n(v) for v in (tx, ts, th, tp)], before)
    _check([a[:M] for a in got], logits, seq[:M], hep[:M], excl[:M], paths[:M], 63)


# ============================================================================ 2. the slate position
@pytest.mark.parametrize("L,with_offer", [(50, False), (320, False), (50, True)])
def test_slate_position_is_rank_minus_one(oracle, L, with_offer):
    eng, x, logits = _alone(oracle, L)
    M, n = ROWS, 128
    seq, hep, excl, _ = _case(L, M, 257, 31 + L, logits)
    valid = np.sort(np.random.default_rng(5).permutation(N1)[:300]).astype(np.int64) if with_offer else None
    seq[2, L - 5] = seq[2, L - 6]
    for m in (1, 2, 3, 6):  # targets that are admissible, at four depths of the slate
        gone = {int(v) for v in seq[m, :hep[m] + 1]} | ref.hidden(excl[m], N1)
        order = [int(j) + 1 for j in np.argsort(-logits[m].astype(np.float64), kind="stable")]
        ok = [i for i in order if i not in gone and (valid is None or i - 1 in set(valid.tolist()))]
        seq[m, L - 1] = ok[(0, 127, 20, 128, 0, 0, 60)[m]]
    keep = eng.bind_exclusions(_t(excl))
    try:
        if with_offer:
            eng.bind_offer_set(_t(valid), M, prepared=True)
        adm = _n(eng.score_target_rank_admissible(_t(x[:M]), _t(seq), _t(hep))[4])
        ids = _n(eng.recommend(_t(x[:M]), n, seqs=_t(seq), hep=_t(hep), k=n)[1])
    finally:
        if with_offer:
            eng.unbind_offer_set()
        eng.unbind_exclusions()
    del keep
    assert np.array_equal(adm, ref.rows(logits[:M], seq, hep, excl, None, 0, valid))
    checked = 0
    for m in range(M):
        pos = ref.slate_position(logits[m], seq[m, :hep[m] + 1], seq[m, L - 1], ref.hidden(excl[m], N1), valid)
        if pos is None:
            assert int(seq[m, L - 1]) - 1 not in ids[m].tolist(), m  # an inadmissible target is on no slate
        elif adm[m] <= n:
            assert pos == adm[m] - 1 and ids[m, adm[m] - 1] == seq[m, L - 1] - 1, m
            checked += 1
    assert checked >= 3 and adm[1] == 128 and adm[3] == 129 and adm[2] == 21 and adm[6] == 61


# ============================================================================ the model of the loop tests
_ENG, _RUNS = {}, {}


def _sd():
    cfg = arrival_ref.model_config()
    return cfg, synth.irn_state_dict(cfg, arrival_ref.WEIGHT_SEED)


def _engine():
    if "e" not in _ENG:
        _ALONE.clear()
        cfg, sd = _sd()
        _ENG["e"] = make_engine(cfg, sd, max_rows=128, max_seqs=128)
    return _ENG["e"]


def _plain(eng, seq, usr, hep, **kw):
    out = eng.generate_paths(_t(seq), _t(usr), _t(hep), P, k=100, sweep=IRS_SWEEP_BF16, **kw)
    return (_n(out[0]), _n(out[1])) + tuple(tuple(_n(a) for a in o) for o in out[2:])


def _until(eng, seq, usr, hep, check_every=1, **kw):
    out = eng.generate_paths_until(_t(seq), _t(usr), _t(hep), P, k=100, sweep=IRS_SWEEP_BF16, check_every=check_every, **kw)
    return (_n(out[0]), _n(out[1]), out[2], out[3]) + tuple(tuple(_n(a) for a in o) for o in out[4:])


def _n_steps(paths, targets):
    return np.array([(np.where(paths[b] == targets[b])[0].tolist() + [paths.shape[1] - 1])[0] + 1 for b in range(len(paths))])


def _verify_cells(eng, seq, usr, hep, paths, rank_adm, n_steps, excl=None, no_repeat=False, offer=None, standalone=False):
    """Every live cell of rank_adm against the statement on the dense logits of a fresh decode of the rebuilt window (and, with
    `standalone`, against irs_score_target_rank_admissible on the same rows, exactly equal to the statement): the module
    docstring's rule.  Returns (live, excused, close)."""
    cfg, sd = _sd()
    B = len(seq)
    win, he = [np.array(r) for r in seq], [int(h) for h in hep]
    live = excused = close_n = 0
    keep = eng.bind_exclusions(_t(excl)) if (standalone and excl is not None) else None
    if standalone and offer is not None:
        eng.bind_offer_set(_t(np.asarray(offer, dtype=np.int64)), B)
    try:
        for i in range(paths.shape[1]):
            rows = [b for b in range(B) if i < n_steps[b]]
            if not rows:
                break
            w, h = np.stack(win), np.array(he, dtype=np.int32)
            _, xr, _ = eng.decode(_t(w), _t(usr), want_x=False, pos=_t(h))
            lg = _n(eng.score_dense(xr))
            want = ref.rows(lg, w, h, excl, paths if no_repeat else None, i, offer)
            if standalone:
                alone = _n(eng.score_target_rank_admissible(xr, _t(w), _t(h), _t(paths) if no_repeat else None, i)[4])
                assert np.array_equal(alone, want), i
            LOGIT, _ = _bounds(sd, 1.0)
            for b in rows:
                live += 1
                t0 = int(seq[b, -1]) - 1
                close = np.abs(np.delete(lg[b].astype(np.float64), t0) - float(lg[b, t0])).min() <= LOGIT
                close_n += close
                if rank_adm[b, i] != want[b]:
                    print(f"user {b} step {i}: rank_adm {rank_adm[b, i]} / {want[b]}")
                    assert close, (b, i, rank_adm[b, i], want[b])
                    excused += 1
                win[b], he[b] = path_ref.advance(win[b], he[b], int(paths[b, i])) if paths[b, i] != 0 else (win[b], he[b])
    finally:
        if standalone and offer is not None:
            eng.unbind_offer_set()
        if keep is not None:
            eng.unbind_exclusions()
    del keep
    print(f"live {live} excused {excused} close {close_n}")
    assert excused <= 0.05 * live
    return live, excused, close_n


def _bound_run(B):
    """The plain loop with ml-1m-shaped lists, no_repeat and exact candidates, trace and admissible rank: once per B."""
    if B not in _RUNS:
        eng = _engine()
        seq, usr, hep = arrival_ref.batch(B, SEED)
        excl = ref.ml1m_lists(B, 500, LIST_SEED)
        kw = dict(exclude=_t(excl), no_repeat=True, exact_candidates=True, trace=True, rank_admissible=True)
        _RUNS[B] = dict(seq=seq, usr=usr, hep=hep, excl=excl, kw=kw, stream=_plain(eng, seq, usr, hep, **kw))
    return _RUNS[B]


# ============================================================================ 3. the loops
@pytest.mark.parametrize("B", [8, 96])  # either side of the 64-row hand-over of the step counter
def test_loops(B):
    """The statement alone could excuse 3 of 64 cells (4.7 %) at B = 8 and 55 of 768 (7.2 %) at B = 96 (module docstring, CPU walk);
    the cells that differ are held to the 5 % cap, and each of them must be one of those."""
    eng = _engine()
    o = _bound_run(B)
    seq, usr, hep, excl, kw = o["seq"], o["usr"], o["hep"], o["excl"], o["kw"]
    stream = o["stream"]
    graph = _plain(eng, seq, usr, hep, use_graph=True, **kw)
    assert np.array_equal(stream[0], graph[0]) and np.array_equal(stream[1], graph[1]) and _same_bits(stream[2], graph[2])
    assert len(stream[2]) == 4
    rank_t, rank_a = stream[2][2], stream[2][3]
    assert rank_a.dtype == np.int32 and rank_a.shape == (B, P)
    assert (rank_a >= 1).all() and (rank_a <= rank_t).all() and (rank_a < rank_t).any()
    # only the trace bound: the two ranks agree in every cell
    bare = _plain(eng, seq, usr, hep, trace=True, rank_admissible=True)
    assert np.array_equal(bare[2][3], bare[2][2]) and (bare[2][2] >= 1).all()
    assert _same_bits(bare[:2] + bare[2][:3], (lambda p: p[:2] + p[2])(_plain(eng, seq, usr, hep, trace=True)))
    # the recorded values replayed: rebuilt windows, a decode, the standalone call
    live, excused, close = _verify_cells(eng, seq, usr, hep, stream[0], rank_a, np.full(B, P), excl, True, standalone=True)
    assert live == B * P
    # the until loop equals the plain loop on the kept steps, and is zero behind them
    targets = seq[:, -1]
    for check_every in (1, 3):
        got = _until(eng, seq, usr, hep, check_every, **kw)
        n = _n_steps(got[0], targets)
        LOGIT, _ = _bounds(_sd()[1], 1.0)
        diff = 0
        for b in range(B):
            assert np.array_equal(got[0][b, :n[b]], stream[0][b, :n[b]]) and not got[0][b, n[b]:].any()
            assert not got[4][3][b, n[b]:].any() and not got[4][2][b, n[b]:].any()
            diff += int((got[4][3][b, :n[b]] != rank_a[b, :n[b]]).sum())
        assert diff <= 0.05 * int(n.sum())
        _verify_cells(eng, seq, usr, hep, got[0], got[4][3], n, excl, True)


# ============================================================================ 4. the rule
def test_rank_one_among_the_admissible_is_the_greedy_choice():
    eng = _engine()
    o = _bound_run(96)
    seq, usr, hep, excl = o["seq"], o["usr"], o["hep"], o["excl"]
    # arrivals by construction: every third user lists what outscores its target at step 0 (every sixth keeps the best of them, to
    # be chosen first), so that the target is the best admissible item there or soon after
    _, xr, _ = eng.decode(_t(seq), _t(usr), want_x=False, pos=_t(hep))
    lg = _n(eng.score_dense(xr))
    more = np.full((len(seq), 500), -1, dtype=np.int64)
    made = []
    for b in range(0, len(seq), 3):
        t0 = int(seq[b, -1]) - 1
        if t0 + 1 in seq[b, :hep[b] + 1]:
            continue
        key = path_ref.order_key(lg[b])
        before = sorted((j for j in range(500) if j != t0 and (key[j] > key[t0] or (key[j] == key[t0] and j < t0))
                         and j + 1 not in seq[b, :hep[b] + 1] and j not in excl[b]), key=lambda j: (-int(key[j]), j))
        excl[b][excl[b] == t0] = -1
        more[b, :len(before)] = before
        if b % 6 and before:
            more[b, 0] = -1
        else:
            made.append(b)
    excl = np.concatenate([excl, more], axis=1)
    kw = dict(o["kw"], exclude=_t(excl))
    off = _until(eng, seq, usr, hep, **kw)
    one = _until(eng, seq, usr, hep, arrive_rank=1, arrive_among="admissible", **kw)
    assert np.array_equal(one[0], off[0]) and one[2:4] == off[2:4]
    assert np.array_equal(one[1] & ~IRS_ROW_OFFERED, off[1])
    arrived = (off[0] == seq[:, -1:]).any(axis=1)
    print(f"{int(arrived.sum())} of {len(seq)} users arrive")
    assert len(made) >= 8 and all(off[0][b, 0] == seq[b, -1] for b in made)
    assert np.array_equal((one[1] & IRS_ROW_OFFERED) != 0, arrived)  # offered exactly at the arrival steps
    n = _n_steps(one[0], seq[:, -1])
    assert all(one[4][3][b, n[b] - 1] == 1 for b in np.where(arrived)[0])
    # the window's rank at 1 fires no later and, with lists bound, somewhere else: there the listed items outscore the target
    assert (one[4][3] <= one[4][2]).all()


@pytest.mark.parametrize("B", [8, 96])
def test_every_decision_replays_from_the_recorded_rank(B):
    eng = _engine()
    o = _bound_run(B)
    seq, usr, hep, excl, kw = o["seq"], o["usr"], o["hep"], o["excl"], o["kw"]
    off = o["stream"]
    r = arrival_ref.thresholds((off[2][0], off[2][1], off[2][3]))[0]
    assert r >= 2
    got = _until(eng, seq, usr, hep, 1, arrive_rank=r, arrive_among="admissible", **kw)
    w_paths, w_tr, n, arrived, offered = ref.replay(seq, hep, off[0], off[2][:3], off[2][3], r, NAN, 500, excl=excl, no_repeat=True)
    assert np.array_equal(got[0], w_paths), np.where(got[0] != w_paths)
    assert np.array_equal((got[1] & IRS_ROW_OFFERED) != 0, offered)
    assert got[2:4] == arrival_ref.until_stats(n, arrived, P, 1)
    mid = int((offered & (n >= 2)).sum())
    print(f"B {B}: rank_max {r}: {mid} users fire at a step in [1, {P - 1}], {int((~offered).sum())} never")
    assert offered.any() and (~offered).any()
    diff = 0
    for b in range(B):
        for a in got[4]:
            assert not a[b, n[b]:].any(), "exactly zero behind the arrival"
        diff += int((got[4][3][b, :n[b]] != w_tr[3][b, :n[b]]).sum())
        if offered[b]:
            assert got[4][3][b, n[b] - 1] <= r
    assert diff <= 0.05 * int(n.sum())
    _verify_cells(eng, seq, usr, hep, got[0], got[4][3], n, excl, True)
    # the window's rank under the same r decides otherwise somewhere: the two kinds are two rules
    win = _until(eng, seq, usr, hep, 1, arrive_rank=r, arrive_among="window", **kw)
    assert ((win[1] & IRS_ROW_OFFERED) != 0).sum() <= offered.sum()
    # kind WINDOW is irs_set_arrival_rule's rule, bit for bit, whether or not the admissible rank is recorded
    kw3 = {k: v for k, v in kw.items() if k != "rank_admissible"}
    old = _until(eng, seq, usr, hep, 1, arrive_rank=r, **kw3)
    assert _same_bits(win[:2], old[:2]) and win[2:4] == old[2:4] and _same_bits(win[4][:3], old[4])


def test_an_admissible_rule_needs_the_binding_and_a_new_trace_drops_it():
    eng = _engine()
    seq, usr, hep = arrival_ref.batch(8, SEED)
    want = _until(eng, seq, usr, hep, 1, trace=True, rank_admissible=True, arrive_rank=5, arrive_among="admissible")
    eng.set_arrival_rule(5, None, "admissible")
    try:
        for call in (lambda: eng.generate_paths(_t(seq), _t(usr), _t(hep), P, trace=True),
                     lambda: eng.generate_paths_until(_t(seq), _t(usr), _t(hep), P, trace=True)):
            with pytest.raises(IrsError, match=r"error -2\b.*irs_bind_trace_admissible"):
                call()
        with pytest.raises(IrsError, match=r"error -2\b.*irs_bind_path_trace"):
            eng.generate_paths(_t(seq), _t(usr), _t(hep), P)
        keep = eng.bind_path_trace(8, P)
        held = eng.bind_trace_admissible(8, P)
        with pytest.raises(IrsError, match=r"error -1\b.*irs_bind_trace_admissible"):
            eng.bind_trace_admissible(8, P + 1)
        got = _until(eng, seq, usr, hep, 1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(_n(held[0]), want[4][3]) and np.array_equal(_n(keep[2]), want[4][2])
        keep2 = eng.bind_path_trace(8, P)  # a new trace: the admissible binding went with the old one
        with pytest.raises(IrsError, match=r"error -2\b.*irs_bind_trace_admissible"):
            eng.generate_paths(_t(seq), _t(usr), _t(hep), P)
        eng.set_arrival_rule(5, None)  # kind WINDOW needs no binding
        eng.generate_paths(_t(seq), _t(usr), _t(hep), P)
        del keep, keep2, held
    finally:
        eng.set_arrival_rule(None, None)
        eng.unbind_path_trace()
    with pytest.raises(ValueError, match="rank_admissible=True"):
        eng.generate_paths(_t(seq), _t(usr), _t(hep), P, trace=True, arrive_rank=5, arrive_among="admissible")


# ============================================================================ 5. compositions
def _small_lists(B):
    return ref.ml1m_lists(B, 500, LIST_SEED + 1, longest=40)


@pytest.mark.parametrize("what", ["guide", "lookahead", "sampled"])
def test_compositions_against_the_statement(what):
    eng = _engine()
    B = 8
    seq, usr, hep = arrival_ref.batch(B, SEED)
    excl = _small_lists(B)
    kw = dict(exclude=_t(excl), no_repeat=True, trace=True, rank_admissible=True)
    if what == "guide":
        kw.update(guide=_t(np.random.default_rng(9).integers(0, 2, (501, 18)).astype(np.uint8)), guide_k=5)
    elif what == "lookahead":
        kw.update(lookahead=3)
    else:
        kw.update(sample=True, sample_k=3, seed=4711)
    base = _plain(eng, seq, usr, hep, exclude=_t(excl), no_repeat=True, trace=True, rank_admissible=True)
    got = _plain(eng, seq, usr, hep, **kw)
    assert not np.array_equal(got[0], base[0])  # the choice rule did choose otherwise
    assert (got[2][3] <= got[2][2]).all() and (got[2][3] >= 1).all()
    live, excused, _ = _verify_cells(eng, seq, usr, hep, got[0], got[2][3], np.full(B, P), excl, True)
    assert live == B * P
    until = _until(eng, seq, usr, hep, 1, **kw)
    n = _n_steps(until[0], seq[:, -1])
    _verify_cells(eng, seq, usr, hep, until[0], until[4][3], n, excl, True)


def test_an_offer_set_equals_its_complement_as_an_exclusion_list():
    eng = _engine()
    B = 8
    seq, usr, hep = arrival_ref.batch(B, SEED)
    S = np.sort(np.random.default_rng(21).permutation(500)[:180]).astype(np.int64)
    comp = np.array(sorted(set(range(500)) - set(S.tolist())), dtype=np.int64)
    common = dict(exact_candidates=True, no_repeat=True, trace=True, rank_admissible=True)
    a = _plain(eng, seq, usr, hep, offer=_t(S), **common)
    b = _plain(eng, seq, usr, hep, exclude=_t(np.tile(comp, (B, 1))), **common)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[2][3], b[2][3]) and np.array_equal(a[2][2], b[2][2])
    assert (a[2][3] < a[2][2]).any()
    live, excused, _ = _verify_cells(eng, seq, usr, hep, a[0], a[2][3], np.full(B, P), None, True, offer=S, standalone=True)
    assert live == B * P
    # and with a list on top of the set, in the until loop under the rule
    excl = _small_lists(B)
    r = arrival_ref.thresholds((a[2][0], a[2][1], a[2][3]))[0]
    ua = _until(eng, seq, usr, hep, 1, offer=_t(S), exclude=_t(excl), arrive_rank=r, arrive_among="admissible", **common)
    ub = _until(eng, seq, usr, hep, 1, exclude=_t(np.concatenate([np.tile(comp, (B, 1)), excl], axis=1)), arrive_rank=r,
                arrive_among="admissible", **common)
    assert np.array_equal(ua[0], ub[0]) and np.array_equal(ua[4][3], ub[4][3])
    tin = np.isin(seq[:, -1] - 1, S)
    assert not ((ua[1] & IRS_ROW_OFFERED) != 0)[~tin].any()  # a target outside the set is never offered ...
    assert np.array_equal((ub[1] & IRS_ROW_OFFERED) != 0, (ua[1] & IRS_ROW_OFFERED) != 0)  # ... like a listed one


# ============================================================================ 6. the front end
def test_front_end():
    cfg, sd = _sd()
    o = _bound_run(8)
    seq, usr, excl = o["seq"], o["usr"], o["excl"]
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.to(DEV)
    irn = IRSNN(cfg, net, DEV)
    irn.eval()
    s, u, t = _t(seq), _t(usr), _t(seq[:, -1].copy())
    lists = [(row[row >= 0] + 1) for row in excl]  # the front end takes 1-based ids
    kw = dict(exclude=lists, no_repeat=True, exact_candidates=True)
    with torch.no_grad():
        plain = irn.get_seq_in_batch(s, u, t, P, 0, False, 3, trace=True, rank_admissible=True, **kw)
        tr = irn.last_trace
        ruled = irn.get_seq_in_batch(s, u, t, P, 0, False, 3, stop_at_target=True, rank_admissible=True, arrive_rank=3,
                                     arrive_among="admissible", **kw)
        tr_r = irn.last_trace
        irn.get_seq_in_batch(s, u, t, P, 0, False, 3, trace=True)
        assert "rank_adm" not in irn.last_trace
        with pytest.raises(ValueError, match="rank_admissible=True"):
            irn.get_seq_in_batch(s, u, t, P, 0, False, 3, arrive_rank=3, arrive_among="admissible")
    n = tr["n_steps"]
    # (the front end's no_repeat also lists the initial window: exclusion_ids0)
    ids0 = np.concatenate([excl, seq[:, :-1] - 1], axis=1)
    eng_run = _plain(_engine(), seq, usr, o["hep"], **dict(o["kw"], exclude=_t(ids0)))
    want = eng_run[2][3].copy()
    for b in range(len(seq)):
        want[b, n[b]:] = 0
    assert np.array_equal(tr["rank_adm"], want) and np.array_equal(plain[0][:, 0], eng_run[0][:, 0])
    first = tr["slate_step"](3)
    assert first.shape == (len(seq),) and all((first[b] == -1) == (not ((want[b] > 0) & (want[b] <= 3)).any()) for b in range(len(seq)))
    # under the rule a user is retired at its slate step
    for b in range(len(seq)):
        if tr_r["offered"][b]:
            assert tr_r["slate_step"](3)[b] == tr_r["n_steps"][b] - 1 and tr_r["rank_adm"][b, tr_r["n_steps"][b] - 1] <= 3
