"""-m gpu: the lookahead choice (include/irs_hip.h, "lookahead choice": irs_bind_lookahead, irs_lookahead_expand,
irs_lookahead_choose; lookahead= in the engine and the front end), against the numpy statement of tests/lookahead_ref.py.

Ids, windows, hep, status words and choices are compared exactly everywhere.  The two kernels alone run on synthetic lists built
to sit on their edges.  The loops are compared with a HOST-STEPPED loop made of the engine's own public calls (decode at hep,
score_topk, lookahead_expand, decode of the children, score_lse, score_gather, lookahead_choose, path_step), so both sides score
the same rows with the same kernels and only the order of the launches is the loop's: bit for bit.

Float bounds.  The emitted lp against the stated double expression: 1 float32 ulp.  The meaning test and the until test use the
bound tests/test_gpu_path_trace.py derives for a log-probability where the launches differ: both decoder rows are within 2e-5 per
element of the truth, so a logit moves by at most LOGIT = 4e-5 max_j ||W_j||_1 and a log-probability by at most
LP = 2 LOGIT + 4e-6 max(1, |lse|)."""
import functools

import numpy as np
import pytest
import torch

import lookahead_ref as ref
import path_ref
from gpu_util import make_engine, path_only_engine
from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_ROW_NO_CANDIDATE, IRS_ROW_OFFERED, IRS_ROW_RESCUED, IRS_SWEEP_BF16
from influentialrs_amd.engine import IrsError
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
from long_window_cases import BY_ID

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_STEP = 600  # catalog of the step-only engines
NINF = np.float32(-np.inf)
L_LONG = BY_ID["tiny_L1024_b3"].config().max_len  # the longest window: the 16-register window image
# Users of the tiny golden for the loop tests.  Chosen on the CPU oracle's float64 child log-probabilities (oracle_np.decode in
# float64, the lookahead search of tests/lookahead_ref.py stepped on it, P = 8) so that the margin rule of the until test excuses
# nobody on the reference alone: the smallest margin between the best and the runner-up child over a user's live steps is
#   k_c = 5:  user 0: 1.1e-2   2: 3.1e-1   3: 6.4e-2   6: 1.8e-1   8: 2.5e-1   11: 2.7e-2
#   k_c = 3:  user 0: 1.2e-1   2: 3.3e-1   3: 7.5e-2   6: 4.6e-2   8: 1.5e-2   11: 2.4e-1
# against 2 LP = 4.9e-4 (LOGIT = 1.1e-4, |lse| <= 5.9).  Under k_c = 5 users 2, 6, 8 and 11 arrive at steps 4, 2, 3 and 3 (counted
# from 1), users 0 and 3 never: the until loop compacts twice.  The other six users have margins between 1.2e-2 and 1.6e-1.
USERS6 = [0, 2, 3, 6, 8, 11]
P8 = 8


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want, names):
    for name, a, b in zip(names, got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(_bits(a), _bits(b)), (name, np.argwhere(a != b)[:8])


# ============================================================================ 1. expand alone
EXPAND_NAMES = ("child_seq", "child_hep", "child_user", "child_target0", "cand_ids0", "cand_val")


@functools.lru_cache(maxsize=None)
def _step_engine(L):
    return path_only_engine(L, n_item=N_STEP)  # (L > 256: the engine opens a long-window context)


def _expand_case(L, M, k, k_c, seed):
    """Rows cycle through hep (first slot, middle, last grow, shift), through the number of leading candidates the window hides
    (0, 1, 2, k_c, 70 -- a second ballot round where the window is long enough --, the whole window), through lists that end early
    at a negative id (before k_c survivors, or before any), and through the target: none, one of the survivors, any item.  A
    window with room holds a pad and a duplicate of a hidden candidate; a slot behind hep holds the first survivor (not window)."""
    g = np.random.default_rng(seed)
    heps = sorted({0, max(0, (L - 2) // 2), max(0, L - 3), L - 2})
    seq = g.integers(6001, 9000, size=(M, L)).astype(np.int64)  # filler: no item of the catalog
    hep = np.zeros(M, dtype=np.int32)
    val = np.zeros((M, k), dtype=np.float32)
    ids0 = np.zeros((M, k), dtype=np.int64)
    info = []
    for r in range(M):
        he = heps[r % len(heps)]
        wl = he + 1
        ids0[r] = g.permutation(N_STEP)[:k]
        val[r] = np.sort(g.permutation(4 * k)[:k].astype(np.float32) * 0.125 - 7.0)[::-1]
        c = int(min([0, 1, 2, k_c, 70, wl][(r // len(heps)) % 6], wl, k))
        end = k
        if r % 7 == 3:
            end = min(k, c + int(g.integers(0, k_c + 2)))
        elif r % 7 == 5:
            end = c
        if end < k:
            ids0[r, end] = -1  # (valid ids follow the end mark: they must not be read)
        free = [int(p) for p in g.permutation(wl)]
        seq[r, free[:c]] = ids0[r, :c] + 1
        rest = free[c:]
        if rest:
            seq[r, rest[0]] = 0
        if c >= 1 and len(rest) >= 2:
            seq[r, rest[1]] = ids0[r, 0] + 1
        surv = [int(i) + 1 for i in ids0[r, c:end]][:k_c]
        if surv and he + 1 <= L - 2:
            seq[r, int(g.integers(he + 1, L - 1))] = surv[0]
        tm = r % 4
        t = 0 if tm == 0 else (surv[int(g.integers(0, len(surv)))] if (tm == 1 and surv) else int(g.integers(1, N_STEP + 1)))
        seq[r, L - 1] = t
        hep[r] = he
        info.append(dict(he=he, c=c, n_surv=len(surv), far=(c >= 64 and len(surv) > 0)))
    users = (np.arange(M, dtype=np.int64) * 3) % 2
    return seq, hep, users, val, ids0, info


def _expand(eng, seq, hep, users, val, ids0, k_c, **kw):
    opt = {n: (_t(a) if isinstance(a, np.ndarray) else a) for n, a in kw.items()}
    d_val, d_ids = _t(val), _t(ids0)
    out = tuple(_n(a) for a in eng.lookahead_expand(_t(seq), _t(hep), _t(users), d_val, d_ids, k_c, **opt))
    assert np.array_equal(_bits(_n(d_val)), _bits(val)) and np.array_equal(_n(d_ids), ids0), "expand only reads the lists"
    return out


@pytest.mark.parametrize("k_c", [1, 5, 32])
@pytest.mark.parametrize("L", [4, 12, L_LONG])
def test_expand_equals_the_statement(L, k_c):
    eng = _step_engine(L)
    M, k = 70, 100  # 70 rows: 17 full workgroups of four waves and a half-empty one
    seq, hep, users, val, ids0, info = _expand_case(L, M, k, k_c, 1000 * L + k_c)
    want = ref.expand(seq, hep, users, val, ids0, k_c)
    got = _expand(eng, seq, hep, users, val, ids0, k_c)
    _same(got, want, EXPAND_NAMES)
    _same(_expand(eng, seq, hep, users, val, ids0, k_c), got, EXPAND_NAMES)
    c_seq, c_hep = got[0].reshape(M, k_c, L), got[1].reshape(M, k_c)
    for r, d in enumerate(info):
        n = d["n_surv"]
        assert (got[4][r, :n] >= 0).all() and (got[4][r, n:] == -1).all() and (got[5][r, n:] == NINF).all(), (r, d)
        for j in range(k_c):
            if j < n:  # the window irs_path_step would leave behind for this item
                w, h = path_ref.advance(seq[r], int(hep[r]), int(got[4][r, j]) + 1)
                assert np.array_equal(c_seq[r, j], w) and c_hep[r, j] == h
            else:
                assert np.array_equal(c_seq[r, j], seq[r]) and c_hep[r, j] == hep[r]
    # every kind of row did occur
    assert any(d["n_surv"] == 0 for d in info) and any(d["n_surv"] == k_c for d in info)
    assert k_c == 1 or any(0 < d["n_surv"] < k_c for d in info)
    assert any(d["he"] < L - 2 and d["n_surv"] for d in info) and any(d["he"] == L - 2 and d["n_surv"] for d in info)
    assert any(d["c"] >= 1 for d in info)
    if L == L_LONG:
        assert any(d["far"] for d in info), "survivors beyond position 64: a second ballot round"


@pytest.mark.parametrize("L", [4, 12, L_LONG])
def test_expand_with_exclusions_no_repeat_fin_and_a_row_map(L):
    eng = _step_engine(L)
    M, k, k_c, step, path_ld, bound, n_excl = 70, 100, 5, 2, 6, 80, 80
    seq, hep, users, val, ids0, info = _expand_case(L, M, k, k_c, 77 * L + 1)
    g = np.random.default_rng(L)
    row_map = g.permutation(bound)[:M].astype(np.int32)
    excl = np.full((bound, n_excl), -1, dtype=np.int64)
    excl[:, 70:] = g.integers(0, N_STEP, size=(bound, 10))
    paths = np.zeros((bound, path_ld), dtype=np.float32)
    paths[:, 2:] = 5.0  # entries from `step` on are not path yet
    fin = (np.arange(M) % 10 == 6).astype(np.int32)
    far = []
    for r in range(M):
        u, c = int(row_map[r]), info[r]["c"]
        lead = [int(i) for i in ids0[r, c:] if i >= 0][:70] if not (ids0[r, c:c + 70] < 0).any() else []
        if r % 9 == 4 and len(lead) == 70:
            excl[u, :66] = lead[:66]  # 66 leading survivors go through the list: the first admissible sits beyond position 64
            far.append(r)
        elif len(lead) >= 8:
            excl[u, :2] = [lead[0], lead[2]]
            paths[u, 0], paths[u, 1] = lead[1] + 1, lead[4] + 1  # the row's own earlier choices: gone under no_repeat
    want = ref.expand(seq, hep, users, val, ids0, k_c, excl, N_STEP, paths, step, True, user_of=row_map, fin=fin)
    unbound = ref.expand(seq, hep, users, val, ids0, k_c)
    scratch = eng.bind_exclusions(_t(excl), bound, True)
    try:
        got = _expand(eng, seq, hep, users, val, ids0, k_c, fin=fin, paths=paths, step=step, row_map=row_map)
        again = _expand(eng, seq, hep, users, val, ids0, k_c, fin=fin, paths=paths, step=step, row_map=row_map)
    finally:
        torch.cuda.synchronize()
        eng.unbind_exclusions()
    _same(got, want, EXPAND_NAMES)
    _same(again, got, EXPAND_NAMES)
    assert (want[4] != unbound[4]).any(), "the lists were meant to move a candidate"
    assert far and all(got[4][r, 0] == ids0[r, info[r]["c"] + 66] for r in far if not fin[r])
    assert fin.any() and (got[4][fin != 0] == -1).all()
    for r in np.where(fin != 0)[0]:
        assert np.array_equal(got[0].reshape(M, k_c, L)[r], np.repeat(seq[r][None], k_c, axis=0))
    _same(_expand(eng, seq, hep, users, val, ids0, k_c), unbound, EXPAND_NAMES)  # unbound again


# ============================================================================ 2. choose alone
def _ulps(a, b):
    """Distance in float32 steps; equal infinities and two NaNs are 0 apart."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)

    def key(x):
        u = x.view(np.uint32).astype(np.int64)
        return np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)
    d = np.abs(key(a) - key(b))
    d[np.isnan(a) & np.isnan(b)] = 0
    d[np.isnan(a) != np.isnan(b)] = 1 << 40
    return d


def _choose_case(M, k, k_c, seed):
    """The first rows are the rule cases of the host test (k_c permitting), the rest random: candidates 0 .. k_c, lp with exact
    ties (target scores on a grid under max = 0, sumexp = 1), NaN, rows without a target (every lp -inf), the target among the
    candidates, rows without a candidate, finished rows."""
    g = np.random.default_rng(seed)
    L = 6
    seq = g.integers(1, N_STEP + 1, size=(M, L)).astype(np.int64)
    c_ids = np.full((M, k_c), -1, dtype=np.int64)
    c_val = np.full((M, k_c), NINF, dtype=np.float32)
    ts = g.standard_normal((M, k_c)).astype(np.float32)
    mx = (g.standard_normal((M, k_c)) * 2 + 3).astype(np.float32)
    sm = (1 + g.random((M, k_c)) * 200).astype(np.float32)
    fin = np.zeros(M, dtype=np.int32)
    for r in range(M):
        n = [k_c, k_c, max(k_c - 1, 0), 1, 0, k_c // 2][r % 6]
        items = g.permutation(N_STEP)[:n]
        c_ids[r, :n] = items
        c_val[r, :n] = np.sort(g.standard_normal(n).astype(np.float32))[::-1]
        kind = r % 9
        if kind in (1, 2):  # exact ties: lp = ts on a grid of three values
            mx[r], sm[r] = 0.0, 1.0
            ts[r] = g.integers(-2, 1, size=k_c).astype(np.float32) * 0.5
        if kind == 3 and n:
            ts[r, g.integers(0, n)] = np.nan
        if kind == 4:
            ts[r, 0] = np.nan  # a NaN first survivor
        if kind == 5:
            ts[r] = np.nan
        if kind == 6:
            seq[r, L - 1] = 0  # no target: the gather gives -inf on every child
            ts[r] = NINF
        if kind == 7 and n:
            seq[r, L - 1] = items[g.integers(0, n)] + 1  # the target among the candidates, its lp whatever
        if kind == 8:
            fin[r] = 1
    val = np.sort(g.standard_normal((M, k)).astype(np.float32), axis=1)[:, ::-1].copy()
    ids0 = np.stack([g.permutation(N_STEP)[:k] for _ in range(M)]).astype(np.int64)
    return seq, c_ids, c_val, ts, mx, sm, fin, val, ids0


@pytest.mark.parametrize("k,k_c", [(100, 1), (100, 5), (100, 32), (1, 1), (7, 5)])
def test_choose_equals_the_statement(k, k_c):
    M = 70
    eng_L = 6
    eng = _step_engine(eng_L)
    seq, c_ids, c_val, ts, mx, sm, fin, val, ids0 = _choose_case(M, k, k_c, 31 * k + k_c)
    assert seq.shape[1] == eng_L

    def run():
        d_val, d_ids = _t(val), _t(ids0)
        lp, choice = eng.lookahead_choose(_t(seq), _t(c_ids), _t(c_val), _t(mx), _t(sm), _t(ts), d_val, d_ids, fin=_t(fin))
        return _n(lp), _n(choice), _n(d_val), _n(d_ids)
    lp, choice, o_val, o_ids = run()
    _same(run(), (lp, choice, o_val, o_ids), ("lp", "choice", "val", "ids0"))
    assert lp.dtype == np.float32 and choice.dtype == np.int32 and lp.shape == (M, k_c)
    want_lp = ref.lp_values(ts, mx, sm, c_ids)
    assert _ulps(lp, want_lp).max() <= 1, "the emitted lp is the stated double expression within 1 float32 ulp"
    assert (lp[c_ids < 0] == NINF).all() and (lp[seq[:, -1] == 0] == NINF).all()
    # the choice from the EMITTED lp, exactly; the lists rewritten as the statement rewrites them
    w_val, w_ids, w_choice = ref.choose(seq, c_ids, c_val, lp, val, ids0, fin)
    assert np.array_equal(choice, w_choice), np.where(choice != w_choice)
    assert np.array_equal(o_ids, w_ids) and np.array_equal(_bits(o_val), _bits(w_val))
    live = fin == 0
    assert np.array_equal(o_ids[~live], ids0[~live]) and np.array_equal(_bits(o_val[~live]), _bits(val[~live])), "finished rows stay untouched"
    assert (choice[~live] == -1).all() and (choice[live & (c_ids[:, 0] < 0)] == -1).all()
    has = live & (c_ids[:, 0] >= 0)
    assert (choice[has] >= 0).all() and (o_ids[has, 0] == c_ids[has, choice[has]]).all()
    assert np.array_equal(_bits(o_val[has, 0]), _bits(c_val[has, choice[has]])), "entry 0 keeps the candidate's original score"
    if k > 1:
        assert (o_ids[has, 1] == -1).all() and (o_val[has, 1] == NINF).all() and np.array_equal(o_ids[has, 2:], ids0[has, 2:])
    for r in np.where(has & (seq[:, -1] == 0))[0]:
        assert choice[r] == 0, "all -inf: the first survivor, the greedy choice"
    for r in np.where(has)[0]:
        at = np.where((c_ids[r] >= 0) & (c_ids[r] + 1 == seq[r, -1]))[0]
        if len(at):
            assert choice[r] == at[0], "the target among the candidates is chosen outright"
    if k_c > 1:
        assert (choice[has] > 0).any() and (choice[has] == 0).any()
        tied = [r for r in np.where(has)[0] if (lp[r] == lp[r, choice[r]]).sum() > 1]
        assert tied and all(choice[r] == int(np.argmax(lp[r] == lp[r, choice[r]])) for r in tied
                            if not ((c_ids[r] >= 0) & (c_ids[r] + 1 == seq[r, -1])).any()), "ties go to the better rank"
        assert any(np.isnan(lp[r]).any() and not np.isnan(lp[r, choice[r]]) for r in np.where(has)[0])


# ============================================================================ 3. the loops against a host-stepped loop
_TINY = {}


def _tiny(golden):
    if not _TINY:
        cfg = synth.make_config("tiny")
        sd = synth.irn_state_dict(cfg, 1234)
        g = golden("irn_tiny")
        _TINY.update(cfg=cfg, sd=sd, eng=make_engine(cfg, sd, max_rows=64, max_seqs=64), seqs=g["seqs"].astype(np.int64),
                     users=g["users"].astype(np.int64))
        assert (cfg.n_item, cfg.emb_dim, cfg.max_len, cfg.n_layers) == (257, 16, 12, 2)
    return _TINY


def _inputs(t, src):
    seq = t["seqs"][np.asarray(src)]
    return seq, t["users"][np.asarray(src)], np.full(len(seq), seq.shape[1] - 2, dtype=np.int32)  # the golden's gap_len is 0


def _host_stepped(eng, seq, usr, hep, P, k_c, k=100, trace=False, arrive_rank=None, exact=False, excl=None, no_repeat=False):
    """The bound loop made of public calls, one step at a time.  Returns dict(paths, seq, hep, status, items, lp, choice,
    trace=(lp_item, lp_target, rank) or None).  After every step the window must equal the chosen child's."""
    B = len(seq)
    seq, usr, hep = _t(seq), _t(usr), _t(hep)
    paths = torch.zeros((B, P), dtype=torch.float32, device=DEV)
    status = torch.zeros(B, dtype=torch.int32, device=DEV)
    items, lps = np.zeros((B, P, k_c), dtype=np.int32), np.zeros((B, P, k_c), dtype=np.float32)
    choices = np.zeros((B, P), dtype=np.int32)
    lp_item, lp_target = np.zeros((B, P), dtype=np.float32), np.zeros((B, P), dtype=np.float32)
    rank = np.zeros((B, P), dtype=np.int32)
    need_trace = trace or arrive_rank is not None
    scratch = eng.bind_exclusions(None if excl is None else _t(excl), B, no_repeat) if (excl is not None or no_repeat) else None
    try:
        for i in range(P):
            _, xr, _ = eng.decode(seq, usr, want_x=False, pos=hep)
            val, ids, _ = eng.score_topk(xr, k, IRS_SWEEP_BF16, carry=i > 0)
            if exact:
                eng.ensure_survivors(xr, seq, hep, val, ids, status, want=k_c)
            if need_trace:
                mx, sm, ts, rk = eng.score_target_trace(xr, seq, hep)
            if arrive_rank is not None:
                eng.arrival_offer(seq, hep, mx, sm, ts, rk, val, ids, status, rank_max=arrive_rank, paths=paths, step=i)
            c_seq, c_hep, c_user, c_tgt, c_ids, c_val = eng.lookahead_expand(seq, hep, usr, val, ids, k_c, paths=paths, step=i)
            _, cx, _ = eng.decode(c_seq, c_user, want_x=False, pos=c_hep)
            cmx, csm = eng.score_lse(cx)
            cts = eng.score_gather(cx, c_tgt.reshape(-1, 1))
            lp, choice = eng.lookahead_choose(seq, c_ids, c_val, cmx, csm, cts, val, ids)
            eng.path_step(seq, hep, val, ids, i, paths, status)
            n_choice, n_seq, n_cseq = _n(choice), _n(seq), _n(c_seq).reshape(B, k_c, -1)
            for b in range(B):
                assert n_choice[b] >= 0 and np.array_equal(n_seq[b], n_cseq[b, n_choice[b]]), "the window is the chosen child's"
            assert np.array_equal(_n(hep), _n(c_hep).reshape(B, k_c)[np.arange(B), n_choice])
            items[:, i], lps[:, i], choices[:, i] = (_n(c_ids) + 1).astype(np.int32), _n(lp), n_choice
            if need_trace:
                n_val, n_ids, chosen = _n(val), _n(ids), _n(paths)[:, i]
                lse = _n(mx).astype(np.float64) + np.log(_n(sm).astype(np.float64))
                for b in range(B):
                    lp_target[b, i] = np.float32(np.float64(_n(ts)[b]) - lse[b])
                    at = np.where(n_ids[b] == int(chosen[b]) - 1)[0]
                    assert chosen[b] != 0 and len(at) >= 1 and at[0] == 0, "the chosen item stands in entry 0"
                    lp_item[b, i] = np.float32(np.float64(n_val[b, 0]) - lse[b])
                rank[:, i] = _n(rk)
    finally:
        if scratch is not None:
            torch.cuda.synchronize()
            eng.unbind_exclusions()
    return dict(paths=_n(paths), seq=_n(seq), hep=_n(hep), status=_n(status), items=items, lp=lps, choice=choices,
                trace=(lp_item, lp_target, rank) if need_trace else None)


def _loop(eng, seq, usr, hep, P, k_c, k=100, until=False, **kw):
    """generate_paths / generate_paths_until with lookahead=k_c and a record: the same dict as _host_stepped (no choice)."""
    d_seq, d_hep = _t(seq), _t(hep)
    trace = kw.get("trace", False)
    if until:
        out = eng.generate_paths_until(d_seq, _t(usr), d_hep, P, k=k, sweep=IRS_SWEEP_BF16, lookahead=k_c, lookahead_record=True, **kw)
        paths, status, rest = out[0], out[1], out[4:]
    else:
        out = eng.generate_paths(d_seq, _t(usr), d_hep, P, k=k, sweep=IRS_SWEEP_BF16, lookahead=k_c, lookahead_record=True, **kw)
        paths, status, rest = out[0], out[1], out[2:]
    tr = tuple(_n(a) for a in rest[0]) if trace else None
    items, lp = rest[-1]
    return dict(paths=_n(paths), seq=_n(d_seq), hep=_n(d_hep), status=_n(status), items=_n(items), lp=_n(lp), trace=tr)


def _equal_runs(got, want, what):
    keys = ("paths", "seq", "hep", "status", "items", "lp")
    _same([got[k] for k in keys], [want[k] for k in keys], [f"{what}: {k}" for k in keys])
    if want["trace"] is not None:
        _same(got["trace"], want["trace"], [f"{what}: lp_item", f"{what}: lp_target", f"{what}: rank_target"])


@pytest.mark.parametrize("k_c", [1, 3, 5])
def test_loops_equal_the_host_stepped_loop(golden, k_c):
    t = _tiny(golden)
    eng = t["eng"]
    seq, usr, hep = _inputs(t, USERS6)
    want = _host_stepped(eng, seq, usr, hep, P8, k_c, trace=True)
    stream = _loop(eng, seq, usr, hep, P8, k_c, trace=True)
    _equal_runs(stream, want, "stream")
    graph = _loop(eng, seq, usr, hep, P8, k_c, trace=True, use_graph=True)
    _equal_runs(graph, want, "captured")
    _equal_runs(_loop(eng, seq, usr, hep, P8, k_c, trace=True), stream, "again")  # no atomics: identical bytes
    assert not (want["status"] & IRS_ROW_NO_CANDIDATE).any() and (want["paths"] != 0).all()
    assert (want["items"][:, :, :k_c] > 0).all() and (want["lp"] < 0).all()
    # the record replays every decision
    for b in range(len(seq)):
        for i in range(P8):
            c = ref.choose_index(want["lp"][b, i], [int(x) for x in want["items"][b, i]], int(seq[b, -1]))
            assert c == want["choice"][b, i] and want["paths"][b, i] == want["items"][b, i, c]
    d_seq, d_hep = _t(seq), _t(hep)
    plain = eng.generate_paths(d_seq, _t(usr), d_hep, P8, k=100, sweep=IRS_SWEEP_BF16)
    if k_c == 1:  # the greedy search, id for id
        assert np.array_equal(_n(plain[0]), stream["paths"]) and np.array_equal(_n(d_seq), stream["seq"])
        assert np.array_equal(_n(d_hep), stream["hep"]) and np.array_equal(_n(plain[1]), stream["status"])
        assert (want["choice"] == 0).all()
    else:
        assert (_n(plain[0]) != stream["paths"]).any() and (want["choice"] > 0).any()


def test_loop_above_the_small_plan_switch(golden):
    """70 users: beyond the 64 rows of the single-workgroup plan, so the step counter moves by its own launch behind the step, and
    the 140 children cross the switch as well."""
    t = _tiny(golden)
    eng = make_engine(t["cfg"], t["sd"], max_rows=160, max_seqs=160)
    seq, usr, hep = _inputs(t, np.arange(70) % 12)
    want = _host_stepped(eng, seq, usr, hep, 3, 2, trace=True)
    _equal_runs(_loop(eng, seq, usr, hep, 3, 2, trace=True), want, "stream")
    _equal_runs(_loop(eng, seq, usr, hep, 3, 2, trace=True, use_graph=True), want, "captured")
    _same([want[k][12:24] for k in ("paths", "items", "lp")], [want[k][:12] for k in ("paths", "items", "lp")],
          ("paths", "items", "lp"))  # equal users, equal rows


# ============================================================================ 4. meaning, against the float64 oracle
def _bounds(sd, lse_abs):
    logit = 4e-5 * float(np.abs(sd["project.weight"]).sum(axis=1).max())
    return logit, 2 * logit + 4e-6 * max(1.0, lse_abs)


def _oracle_lp(oracle, t, child, user, he, target):
    """(log-probability of `target` at slot he of the child window, |lse|) in float64."""
    x, _ = oracle.decode(t["sd"], t["cfg"], child, int(user), dtype=np.float64)
    lg = t["sd"]["project.weight"].astype(np.float64) @ x[he] + t["sd"]["project.bias"].astype(np.float64)
    m = lg.max()
    lse = m + np.log(np.exp(lg - m).sum())
    return lg[int(target) - 1] - lse, abs(lse)


def test_recorded_lp_is_the_targets_next_step_log_probability(golden, oracle):
    """Teacher-forced on the device's own path: every child window is rebuilt on the host from the path and the record, and the
    target's log-probability under the float64 oracle is held against the recorded value."""
    t = _tiny(golden)
    k_c = 3
    seq, usr, hep = _inputs(t, USERS6)
    run = _loop(t["eng"], seq, usr, hep, P8, k_c)
    worst, lse_abs, rows = 0.0, 0.0, []
    for b in range(len(seq)):
        w, h = seq[b].copy(), int(hep[b])
        for i in range(P8):
            for j in range(k_c):
                item = int(run["items"][b, i, j])
                assert item > 0
                cw, ch = path_ref.advance(w, h, item)
                lp64, la = _oracle_lp(oracle, t, cw, usr[b], ch, seq[b, -1])
                lse_abs = max(lse_abs, la)
                rows.append((b, i, j, abs(float(run["lp"][b, i, j]) - lp64)))
            w, h = path_ref.advance(w, h, int(run["paths"][b, i]))
        assert np.array_equal(w, run["seq"][b]) and h == run["hep"][b]
    LOGIT, LP = _bounds(t["sd"], lse_abs)
    worst = max(r[3] for r in rows)
    print(f"max |lp - float64| {worst:.3g} over {len(rows)} children, bound {LP:.3g} (LOGIT {LOGIT:.3g}, |lse| <= {lse_abs:.3g})")
    assert worst <= LP, [r for r in rows if r[3] > LP][:8]
    # the rule did choose: a candidate other than the first, somewhere
    first = run["items"][:, :, 0].astype(np.float32)
    assert (run["paths"] != first).any()


# ============================================================================ 5. the until loop, arrival rule, exact candidates, exclusions
def _cut(paths, targets, arrays):
    n = np.full(len(paths), paths.shape[1])
    out = [np.array(a) for a in arrays]
    for b in range(len(paths)):
        pos = np.where(paths[b] == targets[b])[0]
        if len(pos):
            n[b] = pos[0] + 1
            for a in out:
                a[b, n[b]:] = 0
    return n, out


@pytest.mark.parametrize("check_every", [1, 3])
def test_until_loop_equals_the_plain_loop_cut_on_the_host(golden, check_every):
    t = _tiny(golden)
    eng, k_c = t["eng"], 5
    seq, usr, hep = _inputs(t, USERS6)
    targets = seq[:, -1].copy()
    plain = _loop(eng, seq, usr, hep, P8, k_c)
    n, (w_paths, w_items, w_lp) = _cut(plain["paths"], targets, [plain["paths"], plain["items"], plain["lp"]])
    assert 2 <= (n < P8).sum() < len(seq) and len(set(n[n < P8].tolist())) >= 2, n  # more than one compaction, not everybody
    _, LP = _bounds(t["sd"], 8.0)  # (|lse| of the tiny model stays below 6: the meaning test prints it)
    compared, excused = [], []
    for b in range(len(seq)):
        margins = []
        for i in range(n[b]):
            if (plain["items"][b, i] == targets[b]).any():
                continue  # the target is chosen outright: no comparison decides this step
            lp = np.sort(plain["lp"][b, i].astype(np.float64))[::-1]
            margins.append(lp[0] - lp[1])
        print(f"user {USERS6[b]}: live steps {n[b]}, smallest margin {min(margins) if margins else float('inf'):.3g}, 2 LP {2 * LP:.3g}")
        (compared if (not margins or min(margins) > 2 * LP) else excused).append(b)
    assert len(excused) <= len(seq) // 4 and len(compared) >= 4, (compared, excused)
    got = _loop(eng, seq, usr, hep, P8, k_c, until=True, check_every=check_every)
    for b in compared:
        assert np.array_equal(got["paths"][b], w_paths[b]), (b, got["paths"][b], w_paths[b])
        assert np.array_equal(got["items"][b], w_items[b]), b
        assert not got["lp"][b, n[b]:].any() and not got["items"][b, n[b]:].any(), "exactly zero behind the arrival"
        assert np.abs(got["lp"][b, :n[b]].astype(np.float64) - w_lp[b, :n[b]].astype(np.float64)).max() <= LP
    # targets that never arrive (the last item of the history: the window holds it for all 8 steps): nothing is compacted, the
    # same launches on the same bytes
    far = seq.copy()
    far[:, -1] = far[:, -2]
    assert (far[:, -1] > 0).all()
    want = _loop(eng, far, usr, hep, P8, k_c)
    assert not (want["paths"] == far[:, -1:]).any()
    got = _loop(eng, far, usr, hep, P8, k_c, until=True, check_every=check_every)
    _same([got[k] for k in ("paths", "status", "items", "lp")], [want[k] for k in ("paths", "status", "items", "lp")],
          ("paths", "status", "items", "lp"))


def test_arrival_rule_composes(golden):
    t = _tiny(golden)
    seq, usr, hep = _inputs(t, USERS6)
    want = _host_stepped(t["eng"], seq, usr, hep, P8, 3, arrive_rank=10)
    got = _loop(t["eng"], seq, usr, hep, P8, 3, trace=True, arrive_rank=10)
    _equal_runs(got, want, "arrive_rank")
    offered = (got["status"] & IRS_ROW_OFFERED) != 0
    assert offered.any() and not offered.all()
    for b in np.where(offered)[0]:
        i = int(np.where(got["paths"][b] == seq[b, -1])[0][0])
        assert got["items"][b, i].tolist() == [int(seq[b, -1]), 0, 0], "an offered row expands to the target alone"
        assert got["trace"][0][b, i] == got["trace"][1][b, i]


def test_exact_candidates_ask_for_k_c(golden):
    t = _tiny(golden)
    seq, usr, hep = _inputs(t, USERS6)
    k = k_c = 5  # five candidates: a window that hides one of them starves the row of its fifth survivor
    want = _host_stepped(t["eng"], seq, usr, hep, P8, k_c, k=k, exact=True)
    got = _loop(t["eng"], seq, usr, hep, P8, k_c, k=k, exact_candidates=True)
    _equal_runs(got, want, "exact_candidates")
    assert (got["status"] & IRS_ROW_RESCUED).any() and (got["items"] > 0).all(), "every step had its k_c candidates"
    bare = _loop(t["eng"], seq, usr, hep, P8, k_c, k=k)
    assert (bare["items"] == 0).any(), "without the pass a starved row looks ahead from fewer candidates"


def test_exclusions_and_no_repeat_compose(golden):
    t = _tiny(golden)
    seq, usr, hep = _inputs(t, USERS6)
    k_c = 3
    free = _loop(t["eng"], seq, usr, hep, P8, k_c)
    excl = np.full((len(seq), 6), -1, dtype=np.int64)
    excl[:, :3] = free["paths"][:, [0, 2, 5]].astype(np.int64) - 1  # what the free search chose goes on the list
    want = _host_stepped(t["eng"], seq, usr, hep, P8, k_c, excl=excl, no_repeat=True)
    got = _loop(t["eng"], seq, usr, hep, P8, k_c, exclude=_t(excl), no_repeat=True)
    _equal_runs(got, want, "exclude + no_repeat")
    for b in range(len(seq)):
        listed = set((excl[b, :3] + 1).tolist())
        assert not listed & set(got["items"][b].reshape(-1).tolist()), "a listed item is never a candidate"
        assert len(set(got["paths"][b].tolist())) == P8, "no_repeat: nothing is offered twice"
        for i in range(1, P8):
            assert not set(got["paths"][b, :i].tolist()) & set(got["items"][b, i].tolist())
    assert (got["paths"][:, 0] != free["paths"][:, 0]).all()


# ============================================================================ 6. refusals and state
def test_refusals_with_codes_and_messages(golden):
    t = _tiny(golden)
    eng = t["eng"]
    seq, usr, hep = _inputs(t, USERS6)

    def refused(code, *words):
        def check(fn):
            with pytest.raises(IrsError) as e:
                fn()
            torch.cuda.synchronize()
            msg = str(e.value)
            assert f"error {code}:" in msg and all(w in msg for w in words), msg
        return check
    INVALID, UNSUPPORTED = -1, -4
    refused(INVALID, "irs_bind_lookahead", "k_c")(lambda: eng.bind_lookahead(33, 6, 8))
    refused(INVALID, "irs_bind_lookahead")(lambda: eng.bind_lookahead(3, 6, 0))
    table = torch.zeros((t["cfg"].n_item + 1, 4), device=DEV)
    eng.bind_guide(table, 3)
    try:
        refused(UNSUPPORTED, "irs_bind_lookahead", "irs_bind_guide")(lambda: eng.bind_lookahead(3, 6, 8))
    finally:
        eng.unbind_guide()
    eng.bind_lookahead(5, 6, 8, record=True)
    try:
        refused(UNSUPPORTED, "irs_bind_guide", "irs_bind_lookahead")(lambda: eng.bind_guide(table, 3))
        gp = lambda **kw: eng.generate_paths(_t(seq), _t(usr), _t(hep), kw.pop("P", P8), sweep=IRS_SWEEP_BF16, **kw)  # noqa: E731
        refused(UNSUPPORTED, "irs_generate_paths", "sample")(lambda: gp(sample=True))
        refused(INVALID, "irs_generate_paths", "k=4 < k_c=5")(lambda: gp(k=4))
        refused(INVALID, "irs_generate_paths", "8 steps")(lambda: gp(P=9))
        seq7, usr7, hep7 = _inputs(t, USERS6 + [1])
        refused(INVALID, "6 users")(lambda: eng.generate_paths(_t(seq7), _t(usr7), _t(hep7), P8))
        refused(UNSUPPORTED, "irs_generate_paths_until", "sample")(
            lambda: eng.generate_paths_until(_t(seq), _t(usr), _t(hep), P8, sample=True))
        refused(UNSUPPORTED, "irs_beam_search", "greedy loops only")(lambda: eng.beam_search(_t(seq), _t(usr), _t(hep), 3, 2))
        refused(UNSUPPORTED, "irs_beam_search_until", "irs_bind_lookahead")(lambda: eng.beam_search_until(_t(seq), _t(usr), _t(hep), 3, 2))
    finally:
        eng.unbind_lookahead()
    # B k_c beyond the context: both numbers in the message
    seq14, usr14, hep14 = _inputs(t, list(range(12)) + [0, 1])
    refused(INVALID, "B*k_c=70", "max_seqs=64", "max_rows=64")(
        lambda: eng.generate_paths(_t(seq14), _t(usr14), _t(hep14), 2, lookahead=5))
    # nothing stayed bound
    eng.generate_paths(_t(seq), _t(usr), _t(hep), 2, sample=True, sample_k=3, seed=5)
    torch.cuda.synchronize()


def test_unbind_restores_a_fresh_engines_bytes_and_binding_drops_the_captured_step(golden):
    t = _tiny(golden)
    eng = t["eng"]
    seq, usr, hep = _inputs(t, USERS6)

    def plain(e, **kw):
        d_seq, d_hep = _t(seq), _t(hep)
        paths, status = e.generate_paths(d_seq, _t(usr), d_hep, P8, k=100, sweep=IRS_SWEEP_BF16, **kw)
        return _n(paths), _n(status), _n(d_seq), _n(d_hep)
    fresh = plain(make_engine(t["cfg"], t["sd"], max_rows=64, max_seqs=64))
    names = ("paths", "status", "seq", "hep")
    captured = plain(eng, use_graph=True)  # a captured unbound step ...
    _same(captured, fresh, names)
    want = _host_stepped(eng, seq, usr, hep, P8, 3)
    rec = eng.bind_lookahead(3, len(seq), P8, record=True)  # ... a binding of the caller's own drops it ...
    try:
        d_seq, d_hep = _t(seq), _t(hep)
        paths, status = eng.generate_paths(d_seq, _t(usr), d_hep, P8, k=100, sweep=IRS_SWEEP_BF16, use_graph=True)
        bound = (_n(paths), _n(status), _n(d_seq), _n(d_hep))
        _same(bound, [want[k] for k in names], names)
        _same((_n(rec[0]), _n(rec[1])), (want["items"], want["lp"]), ("items", "lp"))
        d_seq, d_hep = _t(seq), _t(hep)
        paths, status = eng.generate_paths(d_seq, _t(usr), d_hep, P8, k=100, sweep=IRS_SWEEP_BF16, use_graph=True)  # replayed
        _same((_n(paths), _n(status), _n(d_seq), _n(d_hep)), bound, names)
    finally:
        torch.cuda.synchronize()
        eng.unbind_lookahead()
    _same(plain(eng, use_graph=True), fresh, names)  # ... and the unbound call is a fresh engine's again, captured and on the stream
    _same(plain(eng), fresh, names)
    assert (bound[0] != fresh[0]).any()


# ============================================================================ 7. the front end
def test_front_end_lookahead(golden):
    t = _tiny(golden)
    cfg = t["cfg"]
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in t["sd"].items()})
    net.to(DEV)
    irn = IRSNN(cfg, net, DEV)
    irn.eval()
    seq, usr, hep = _inputs(t, USERS6)
    targets = seq[:, -1].copy()
    want = _loop(t["eng"], seq, usr, hep, P8, 5)
    n, (w_paths, w_items, w_lp) = _cut(want["paths"], targets, [want["paths"], want["items"], want["lp"]])
    _, LP = _bounds(t["sd"], 8.0)
    with torch.no_grad():
        paths, tg, hist, early = irn.get_seq_in_batch(_t(seq), _t(usr), _t(targets), P8, 0, lookahead=5, lookahead_record=True)
        greedy = irn.get_seq_in_batch(_t(seq), _t(usr), _t(targets), P8, 0)[0]
        one = irn.get_seq_in_batch(_t(seq), _t(usr), _t(targets), P8, 0, lookahead=1)[0]
        until = irn.get_seq_in_batch(_t(seq), _t(usr), _t(targets), P8, 0, stop_at_target=True, lookahead=5)[0]
    # (the front end's engine is sized for B k_c = 30 rows, this module's for 64: ids exactly -- USERS6's margins are far above
    #  LP --, the values within LP)
    assert np.array_equal(paths, w_paths) and early == int((n < P8).sum()) and np.array_equal(tg, targets)
    rec = irn.last_lookahead
    assert rec["items"].shape == (len(seq), P8, 5) and np.array_equal(rec["items"], w_items)
    assert np.abs(rec["lp"].astype(np.float64) - w_lp.astype(np.float64)).max() <= LP
    for b in range(len(seq)):
        assert not rec["items"][b, n[b]:].any() and not rec["lp"][b, n[b]:].any(), "cut after the arrival"
    assert np.array_equal(one, greedy) and (paths != greedy).any() and np.array_equal(until, paths)
