"""-m gpu: the offer set -- search and recommend inside a bound subset of the catalog (irs_bind_offer_set, irs_score_topk_offer,
Engine.bind_offer_set / score_topk_offer, offer= of the search methods and the front ends).

Every comparison is id for id or bit for bit.  The kernel alone is held against tests/offer_set_ref.py (oracle.score_chain over the
whole catalog, restricted to the set, in the library's order) and against irs_score_gather.  The loops and irs_recommend are held
against code that exists: binding the COMPLEMENT of the set as every user's exclusion list, with exact candidates, must give the
same search.  The one tolerance is lp's, the log-sum-exp bound of tests/test_gpu_recommend.py.

Shapes of the kernel as built (csrc/offer_set.hip): 64 ids per workgroup tile, 16 per wave; row groups of 64 rows (32 for d > 128),
at most 64 row-group workgroups per tile; the selection looks at 1024 scores between two compactions of a 2048-key buffer."""
import numpy as np
import pytest
import torch

import offer_set_ref as ref
from gpu_util import make_engine, scoring_only_engine
from influentialrs_amd import synth
from influentialrs_amd._lib import (IRS_ROW_FEWER_THAN_K, IRS_ROW_NO_CANDIDATE, IRS_ROW_OFFERED, IRS_SWEEP_BF16, IRS_SWEEP_F32)
from influentialrs_amd.engine import IrsError, _ptr
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LSE_TOL = 4e-6  # tests/test_gpu_scoring.py: max + log(sum) against the oracle
M_MAX = 65      # one row beyond a 64-row group


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    torch.cuda.synchronize()
    return None if t is None else t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ============================================================================ the engines of the kernel tests
class _Case:
    """An engine, its catalog, M_MAX random rows and their chain scores over the whole catalog (computed once)."""

    def __init__(self, oracle, name):
        if name in ("tiny", "default"):
            cfg = synth.make_config(name)
            sd = synth.irn_state_dict(cfg, seed=1234)
            self.eng = make_engine(cfg, sd, max_rows=80, max_seqs=1, max_k=1024)
            self.W, self.b = sd["project.weight"], sd["project.bias"]
        else:  # ("d64", 300), ("d128", 3415), ("d256", 300): a scoring-only engine on a random catalog
            d, n_item = {"d64": (64, 300), "d128": (128, 3415), "d256": (256, 300)}[name]
            g = np.random.default_rng(d)
            self.W = (g.standard_normal((n_item, d)) / np.sqrt(d)).astype(np.float32)
            self.b = (0.1 * g.standard_normal(n_item)).astype(np.float32)
            self.eng = scoring_only_engine(n_item, d, self.W, self.b, max_rows=80, max_k=1024)
        self.N, self.d = self.W.shape
        self.x = np.random.default_rng(7 + self.d).standard_normal((M_MAX, self.d)).astype(np.float32)
        self.scores = np.stack([oracle.score_chain(self.x[m], self.W, self.b) for m in range(M_MAX)])
        self.tx = _t(self.x)

    def subset(self, C, seed=0):
        return np.sort(np.random.default_rng(1000 * seed + C).permutation(self.N)[:C]).astype(np.int64)


_CASES = {}


@pytest.fixture(scope="module")
def case(oracle):
    def get(name):
        if name not in _CASES:
            _CASES[name] = _Case(oracle, name)
        return _CASES[name]
    yield get
    _CASES.clear()
    torch.cuda.empty_cache()


def _check_lists(c, S, M, k, val, ids, st, what):
    """Rows [0, M) of a call against the statement, and the values against irs_score_gather's on the same rows."""
    val, ids, st = _n(val), _n(ids), _n(st)
    assert val.shape == (M, k) and ids.shape == (M, k) and st.shape == (M,)
    for m in range(M):
        e_val, e_ids, fewer = ref.topk(c.scores[m], S, k)
        assert np.array_equal(ids[m], e_ids), (what, m)
        assert np.array_equal(_bits(val[m]), _bits(e_val)), (what, m)
        assert st[m] == (IRS_ROW_FEWER_THAN_K if fewer else 0), (what, m)
    gathered = _n(c.eng.score_gather(c.tx[:M], _t(ids)))  # (-1 gathers -inf: the list's own fill)
    assert np.array_equal(_bits(gathered), _bits(val)), what


def _ks(C):
    return sorted({k for k in (1, 100, C - 1, C, C + 1, 1024) if 1 <= k <= 1024})


# ============================================================================ 1. the kernel alone
C_SMALL = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
C_LARGE = (1023, 1024, 1025, 2047, 2048, 2049, 3415)  # the selection's chunk and buffer edges, and N


@pytest.mark.parametrize("name", ["tiny", "default", "d128", "d64", "d256"])
def test_kernel_alone_equals_the_statement_and_the_gather(case, name):
    c = case(name)
    sizes = [C for C in C_SMALL + (c.N,) + (C_LARGE if name in ("default", "d128") else ()) if C <= c.N]
    if name in ("d64", "d256"):
        sizes = [1, 17, 64, 65, 257, c.N]
    for C in dict.fromkeys(sizes):
        S = c.subset(C)
        c.eng.bind_offer_set(_t(S), 80)
        try:
            for k in _ks(C):  # every k on 33 rows ...
                _check_lists(c, S, 33, k, *c.eng.score_topk_offer(c.tx[:33], k), (name, C, k))
            for M in (1, 15, 16, 17, 64, M_MAX):  # ... every row count at one k
                k = min(100, C)
                _check_lists(c, S, M, k, *c.eng.score_topk_offer(c.tx[:M], k), (name, C, "M", M))
        finally:
            c.eng.unbind_offer_set()


def test_a_scratch_for_fewer_rows_takes_several_passes(case):
    c = case("default")
    S = c.subset(300)
    for rows in (16, 1, 64):  # 33 rows: three passes (the last of one row), 33 passes, one pass
        c.eng.bind_offer_set(_t(S), rows)
        try:
            _check_lists(c, S, 33, 100, *c.eng.score_topk_offer(c.tx[:33], 100), ("passes", rows))
        finally:
            c.eng.unbind_offer_set()


def test_more_row_groups_than_workgroups_per_tile(oracle):
    """4097 rows are 65 row groups of 64: a tile's 64 workgroups walk them, the first one twice."""
    cfg = synth.make_config("tiny")
    sd = synth.irn_state_dict(cfg, seed=1234)
    M = 4097
    eng = make_engine(cfg, sd, max_rows=M, max_seqs=1, max_k=8)
    x = np.random.default_rng(3).standard_normal((M, cfg.emb_dim)).astype(np.float32)
    S = np.array([0, 5, 77, 200, 256], dtype=np.int64)
    eng.bind_offer_set(_t(S), M)
    val, ids, st = (_n(a) for a in eng.score_topk_offer(_t(x), 3))
    eng.unbind_offer_set()
    for m in list(range(0, M, 61)) + [4031, 4032, 4095, 4096]:
        e_val, e_ids, _ = ref.topk(oracle.score_chain(x[m], sd["project.weight"], sd["project.bias"]), S, 3)
        assert np.array_equal(ids[m], e_ids) and np.array_equal(_bits(val[m]), _bits(e_val)), m
    assert not st.any()


def test_two_identical_calls_give_identical_bits(case):
    c = case("d128")
    S = c.subset(2049)
    c.eng.bind_offer_set(_t(S), 80)
    try:
        a = [_n(t).copy() for t in c.eng.score_topk_offer(c.tx, 1024)]
        b = [_n(t) for t in c.eng.score_topk_offer(c.tx, 1024)]
    finally:
        c.eng.unbind_offer_set()
    assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(a, b))


# ============================================================================ 2. C = n_item: irs_score_topk's answer
@pytest.mark.parametrize("name", ["tiny", "default", "d128"])
def test_the_whole_catalog_as_a_set_equals_score_topk(case, name):
    c = case(name)
    c.eng.bind_offer_set(torch.arange(c.N, device=DEV), 80)
    try:
        for k in (1, 100, min(c.N, 1024)):
            got = [_n(t) for t in c.eng.score_topk_offer(c.tx[:33], k)]
            for sweep in (IRS_SWEEP_F32, IRS_SWEEP_BF16):
                want = [_n(t) for t in c.eng.score_topk(c.tx[:33], k, sweep)]
                assert np.array_equal(got[1], want[1]), (name, k, sweep)
                assert np.array_equal(_bits(got[0]), _bits(want[0])), (name, k, sweep)
                assert np.array_equal(got[2], want[2]), (name, k, sweep)
    finally:
        c.eng.unbind_offer_set()


# ============================================================================ 3. ties
def test_copied_catalog_rows_come_out_in_id_order(oracle):
    """Two, then three, project rows and biases are copies; the set places them inside one id tile and across two (local
    positions 63 | 64).  Equal scores: the lower id first, which the statement's order is."""
    d, n_item = 30, 400
    g = np.random.default_rng(21)
    W = (g.standard_normal((n_item, d)) / np.sqrt(d)).astype(np.float32)
    b = (0.1 * g.standard_normal(n_item)).astype(np.float32)
    S = np.arange(10, 10 + 130, dtype=np.int64) * 2  # local j <-> id 20 + 2 j
    inside2, across2, three = (S[5], S[9]), (S[63], S[64]), (S[62], S[65], S[100])
    for grp in (inside2, across2, three):
        for j in grp[1:]:
            W[j], b[j] = W[grp[0]], b[grp[0]]
    eng = scoring_only_engine(n_item, d, W, b, max_rows=16, max_k=256)
    x = g.standard_normal((9, d)).astype(np.float32)
    eng.bind_offer_set(_t(S), 16)
    val, ids, _ = (_n(a) for a in eng.score_topk_offer(_t(x), len(S)))
    eng.unbind_offer_set()
    for m in range(9):
        e_val, e_ids, _ = ref.topk(oracle.score_chain(x[m], W, b), S, len(S))
        assert np.array_equal(ids[m], e_ids) and np.array_equal(_bits(val[m]), _bits(e_val)), m
        row = ids[m].tolist()
        for grp in (inside2, across2, three):
            at = [row.index(int(j)) for j in grp]
            assert at == list(range(at[0], at[0] + len(grp))), (m, grp, at)  # adjacent, ascending by id


# ============================================================================ 4. prepare
def test_prepare_turns_bad_entries_into_holes_that_are_never_listed(case):
    c = case("default")
    N = c.N
    raw = np.array([3, 9, 9, 8, 40, N, -3, 50, 49, N - 1, 2 ** 40, 60] + list(range(100, 170)), dtype=np.int64)
    san, holes = ref.sanitise(raw, N)
    assert holes == 7 and (san >= 0).sum() == len(raw) - 7  # (60 follows 2 ** 40: not greater than its predecessor)
    eng = c.eng
    scratch = torch.empty(eng.offer_set_scratch_bytes(len(raw), 80), dtype=torch.uint8, device=DEV)
    t_raw = _t(raw)
    eng._call_null(eng.lib.irs_bind_offer_set, _ptr(t_raw), len(raw), _ptr(scratch), scratch.numel(), tensors=(t_raw, scratch))
    try:
        assert int(_n(scratch[:4].view(torch.int32))[0]) == holes
        got_ids = _n(scratch[256:256 + 8 * 128].view(torch.int64))
        assert np.array_equal(got_ids[:len(raw)], san) and (got_ids[len(raw):] == -1).all()
        k = len(raw)
        val, ids, st = (_n(a) for a in eng.score_topk_offer(c.tx[:17], k))
        n_valid = len(raw) - holes
        valid = set(san[san >= 0].tolist())
        for m in range(17):
            e_val, e_ids, _ = ref.topk(c.scores[m], san, k)
            assert np.array_equal(ids[m], e_ids) and np.array_equal(_bits(val[m]), _bits(e_val)), m
            assert set(ids[m, :n_valid].tolist()) == valid and (ids[m, n_valid:] == -1).all()
        assert (st == IRS_ROW_FEWER_THAN_K).all()
    finally:
        eng.unbind_offer_set()
    for prepared in (False, True):  # (sorted and made unique first, the entries outside the catalog remain)
        with pytest.raises(IrsError, match="bind_offer_set"):
            eng.bind_offer_set(_t(raw), 80, prepared=prepared)
    with pytest.raises(IrsError, match="no offer set is bound"):
        eng.score_topk_offer(c.tx[:1], 1)


# ============================================================================ 5. the loops, against the complement as an exclusion list
B5, P5, K5 = 8, 6, 100


class _Loops:
    def __init__(self, golden, max_len=None):
        self.cfg = synth.make_config("tiny") if max_len is None else synth.make_config("tiny", max_len=max_len)
        self.sd = synth.irn_state_dict(self.cfg, 1234)
        self.eng = make_engine(self.cfg, self.sd, max_rows=64, max_seqs=64, max_k=K5)
        self.N, self.L = self.cfg.n_item, self.cfg.max_len
        g = golden("irn_tiny")
        if max_len is None:
            self.seqs = g["seqs"][:B5].astype(np.int64)
        else:  # long windows over a 257-item catalog: most of it is in the window, every row is starved at every step
            r = np.random.default_rng(max_len)
            self.seqs = r.integers(1, self.N + 1, (B5, self.L)).astype(np.int64)
        self.users = g["users"][:B5].astype(np.int64)
        self.hep = np.full(B5, self.L - 2, dtype=np.int32)

    def state(self):
        return _t(self.seqs).clone(), _t(self.users), _t(self.hep).clone()

    def sets(self, C, with_targets=True):
        """A set of C ids0 (the users' targets first where asked, so that paths can arrive) and its complement as [B, E] lists."""
        perm = np.random.default_rng(50 + C).permutation(self.N)
        if C == self.N:
            S = np.arange(self.N)
        elif with_targets and C >= 40:
            tg = np.unique(self.seqs[:, -1] - 1)
            S = np.concatenate([tg, perm[~np.isin(perm, tg)][:C - len(tg)]])
        else:
            S = perm[:C]
        S = np.sort(S).astype(np.int64)
        assert len(np.unique(S)) == C
        comp = ref.complement(S, self.N)
        return S, (np.tile(comp, (B5, 1)) if len(comp) else None)


@pytest.fixture(scope="module")
def loops(golden):
    lp = _Loops(golden)
    yield lp
    torch.cuda.empty_cache()


def _same(a, b, what):
    a, b = _n(a), _n(b)
    assert np.array_equal(a, b), (what, a, b)


def _excl(lists, extra=None):
    """exclude= for the comparison run: the complement lists, with `extra` [B, E2] appended."""
    parts = [p for p in (lists, extra) if p is not None]
    return None if not parts else _t(np.concatenate(parts, axis=1))


@pytest.mark.parametrize("C", [1, 5, 40, 150, 257])
def test_greedy_loops_equal_the_complement_exclusion(loops, C):
    m = loops
    S, comp = m.sets(C)
    ts = _t(S)
    for kw in (dict(), dict(use_graph=True), dict(sample=True, sample_k=3, seed=11)):
        p1, s1 = m.eng.generate_paths(*m.state(), P5, k=K5, exact_candidates=True, offer=ts, **kw)
        p2, s2 = m.eng.generate_paths(*m.state(), P5, k=K5, exact_candidates=True, exclude=_excl(comp), **kw)
        _same(p1, p2, ("generate_paths", C, kw))
        _same(s1 & IRS_ROW_NO_CANDIDATE, s2 & IRS_ROW_NO_CANDIDATE, ("status", C, kw))
        paths = _n(p1)
        assert np.isin(paths[paths > 0] - 1, S).all(), "every offered item is in the set"
        if C == 1:  # the one item is chosen at most once, then the row has nothing left to offer
            assert (_n(s1) & IRS_ROW_NO_CANDIDATE).all() and ((paths > 0).sum(axis=1) <= 1).all()
    for kw in (dict(), dict(sample=True, sample_k=3, seed=11), dict(check_every=2)):
        o1 = m.eng.generate_paths_until(*m.state(), P5, k=K5, exact_candidates=True, offer=ts, **kw)
        o2 = m.eng.generate_paths_until(*m.state(), P5, k=K5, exact_candidates=True, exclude=_excl(comp), **kw)
        _same(o1[0], o2[0], ("generate_paths_until", C, kw))
        _same(o1[1] & IRS_ROW_NO_CANDIDATE, o2[1] & IRS_ROW_NO_CANDIDATE, ("status until", C, kw))
        assert o1[2:4] == o2[2:4], "the same steps were run on the same rows"


@pytest.mark.parametrize("C", [1, 5, 40, 150, 257])
def test_beam_loops_equal_the_complement_exclusion(loops, C):
    m = loops
    S, comp = m.sets(C)
    ts = _t(S)
    for kw in (dict(), dict(use_graph=True)):
        o1 = m.eng.beam_search(*m.state(), P5, 3, k=K5, exact_candidates=True, offer=ts, **kw)
        o2 = m.eng.beam_search(*m.state(), P5, 3, k=K5, exact_candidates=True, exclude=_excl(comp), **kw)
        _same(o1[0], o2[0], ("beam_search", C, kw))
        _same(o1[2] & IRS_ROW_NO_CANDIDATE, o2[2] & IRS_ROW_NO_CANDIDATE, ("beam status", C, kw))
        paths = _n(o1[0])
        assert np.isin(paths[paths > 0] - 1, S).all()
    for rule in (0, 1):  # IRS_BEAM_STOP_ALL, IRS_BEAM_STOP_BEST
        o1 = m.eng.beam_search_until(*m.state(), P5, 3, k=K5, stop_rule=rule, exact_candidates=True, offer=ts)
        o2 = m.eng.beam_search_until(*m.state(), P5, 3, k=K5, stop_rule=rule, exact_candidates=True, exclude=_excl(comp))
        _same(o1[0], o2[0], ("beam_search_until", C, rule))
        _same(o1[3], o2[3], ("fin", C, rule))
        _same(o1[2] & IRS_ROW_NO_CANDIDATE, o2[2] & IRS_ROW_NO_CANDIDATE, ("beam until status", C, rule))
        assert o1[4:6] == o2[4:6]


def test_offer_and_exclude_together_equal_the_union(loops):
    m = loops
    S, comp = m.sets(150)
    E = np.random.default_rng(9).choice(S, (B5, 20)).astype(np.int64)  # every user loses 20 items of the set
    E[:, 0] = -1
    for no_repeat in (False, True):
        p1, s1 = m.eng.generate_paths(*m.state(), P5, k=K5, exact_candidates=True, offer=_t(S), exclude=_t(E), no_repeat=no_repeat)
        p2, s2 = m.eng.generate_paths(*m.state(), P5, k=K5, exact_candidates=True, exclude=_excl(comp, E), no_repeat=no_repeat)
        _same(p1, p2, ("offer + exclude", no_repeat))
        _same(s1 & IRS_ROW_NO_CANDIDATE, s2 & IRS_ROW_NO_CANDIDATE, "status")
        paths = _n(p1).astype(np.int64)
        for b in range(B5):
            assert not set(paths[b][paths[b] > 0] - 1) & set(E[b].tolist())


def test_guide_lookahead_trace_and_arrival_read_the_set(loops):
    m = loops
    S, comp = m.sets(150)
    ts, ex = _t(S), _excl(comp)
    table = _t(np.random.default_rng(4).standard_normal((m.N + 1, 6)).astype(np.float32))
    for kw in (dict(guide=table, guide_k=5), dict(lookahead=3), dict(lookahead=3, lookahead_record=True)):
        o1 = m.eng.generate_paths(*m.state(), P5, k=K5, exact_candidates=True, offer=ts, **kw)
        o2 = m.eng.generate_paths(*m.state(), P5, k=K5, exact_candidates=True, exclude=ex, **kw)
        _same(o1[0], o2[0], kw.keys())
        _same(o1[1] & IRS_ROW_NO_CANDIDATE, o2[1] & IRS_ROW_NO_CANDIDATE, kw.keys())
        if kw.get("lookahead_record"):
            _same(o1[2][0], o2[2][0], "the candidates a lookahead step compared")
    # trace and arrival rule: the targets are in the set (m.sets puts them there) ...
    assert np.isin(m.seqs[:, -1] - 1, S).all()
    for until in (False, True):
        fn = m.eng.generate_paths_until if until else m.eng.generate_paths
        o1 = fn(*m.state(), P5, k=K5, exact_candidates=True, offer=ts, trace=True, arrive_rank=128)
        o2 = fn(*m.state(), P5, k=K5, exact_candidates=True, exclude=ex, trace=True, arrive_rank=128)
        _same(o1[0], o2[0], ("arrival", until))
        _same(o1[1] & (IRS_ROW_NO_CANDIDATE | IRS_ROW_OFFERED), o2[1] & (IRS_ROW_NO_CANDIDATE | IRS_ROW_OFFERED), ("arrival status", until))
        _same(o1[-1][2], o2[-1][2], "rank_target is a statement about the whole catalog in both")
        assert np.abs(_n(o1[-1][1]) - _n(o2[-1][1])).max() <= 1e-5, "lp_target: the same sweep in both"
    fired = (_n(o1[1]) & IRS_ROW_OFFERED) != 0
    assert fired.any(), "the rule fires for somebody at rank <= 128"
    # ... and then out of it: nobody is offered a target that may not be shown, exactly as under the exclusion list
    S_out = np.setdiff1d(S, m.seqs[:, -1] - 1)
    comp_out = np.tile(ref.complement(S_out, m.N), (B5, 1))
    o1 = m.eng.generate_paths(*m.state(), P5, k=K5, exact_candidates=True, offer=_t(S_out), trace=True, arrive_rank=128)
    o2 = m.eng.generate_paths(*m.state(), P5, k=K5, exact_candidates=True, exclude=_t(comp_out), trace=True, arrive_rank=128)
    _same(o1[0], o2[0], "arrival, targets outside the set")
    assert not (_n(o1[1]) & IRS_ROW_OFFERED).any() and not (_n(o2[1]) & IRS_ROW_OFFERED).any()
    paths = _n(o1[0])
    assert not (paths == m.seqs[:, -1:]).any()
    _same(o1[-1][2], o2[-1][2], "rank_target")


def test_long_windows(golden):
    m = _Loops(golden, max_len=300)
    S, comp = m.sets(150)
    p1, s1 = m.eng.generate_paths(*m.state(), P5, k=K5, exact_candidates=True, offer=_t(S))
    p2, s2 = m.eng.generate_paths(*m.state(), P5, k=K5, exact_candidates=True, exclude=_excl(comp))
    _same(p1, p2, "max_len = 300")
    _same(s1 & IRS_ROW_NO_CANDIDATE, s2 & IRS_ROW_NO_CANDIDATE, "status")
    o1 = m.eng.beam_search(*m.state(), P5, 3, k=K5, exact_candidates=True, offer=_t(S))
    o2 = m.eng.beam_search(*m.state(), P5, 3, k=K5, exact_candidates=True, exclude=_excl(comp))
    _same(o1[0], o2[0], "beam, max_len = 300")


def test_the_scratch_must_serve_the_calls_rows(loops):
    """(The option's sharded refusal cannot be reached: irs_bind_offer_set refuses a sharded context, tests/test_offer_set_host.py,
    so no binding exists there.  The row is defensive.)"""
    m = loops
    S, _ = m.sets(40)
    m.eng.bind_offer_set(_t(S), 4)
    try:
        with pytest.raises(IrsError, match="8 rows, the offer set's scratch .* is sized for 4"):
            m.eng.generate_paths(*m.state(), P5, k=K5)
        with pytest.raises(IrsError, match="24 rows"):
            m.eng.beam_search(*m.state(), P5, 3, k=K5)
        x = _t(np.zeros((8, m.cfg.emb_dim), dtype=np.float32))
        with pytest.raises(IrsError, match="8 rows"):
            m.eng.recommend(x, 5)
        m.eng.score_topk_offer(x, 5)  # (the kernel alone walks passes)
        # the take is a kernel on the caller's lists: it does not look at the set, with exclusions bound as well or not
        val, ids = _t(np.zeros((8, 10), dtype=np.float32)), _t(np.tile(np.arange(10, dtype=np.int64), (8, 1)))
        plain = [_n(a) for a in m.eng.recommend_take(val, ids, 5)]
        held = m.eng.bind_exclusions(_t(np.full((8, 2), 3, dtype=np.int64)))
        try:
            taken = [_n(a) for a in m.eng.recommend_take(val, ids, 5)]
            with pytest.raises(IrsError, match="8 rows"):
                m.eng.recommend(x, 5)
        finally:
            m.eng.unbind_exclusions()
        assert plain[1][0].tolist() == [0, 1, 2, 3, 4] and taken[1][0].tolist() == [0, 1, 2, 4, 5]
    finally:
        m.eng.unbind_offer_set()


def test_score_topk_offer_argument_checks_on_a_ready_engine(loops):
    """Every refusal of irs_score_topk_offer through the raw ABI on a finalised engine, with and without a set bound: the code and
    the message.  k is the sole guard of the selection's 2048-key LDS buffer."""
    m = loops
    eng, lib = m.eng, m.eng.lib  # max_rows = 64, max_k = 100
    x = _t(np.zeros((64, m.cfg.emb_dim), dtype=np.float32))
    val = torch.empty((64, 100), dtype=torch.float32, device=DEV)
    ids = torch.empty((64, 100), dtype=torch.int64, device=DEV)
    st = torch.empty(64, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()

    def call(xp, M, k, v, i, s):
        rc = lib.irs_score_topk_offer(eng.h, xp, M, k, v, i, s)
        return rc, (lib.irs_last_error(eng.h).decode() if rc else "")

    px, pv, pi, ps = _ptr(x), _ptr(val), _ptr(ids), _ptr(st)
    S, _ = m.sets(40)
    for bound in (False, True):
        if bound:
            eng.bind_offer_set(_t(S), 64)
        try:
            assert call(None, 1, 10, pv, pi, ps) == (-1, "irs_score_topk_offer: bad arguments")
            for M in (0, -1):
                assert call(px, M, 10, pv, pi, ps) == (-1, "irs_score_topk_offer: bad arguments"), M
            assert call(px, 65, 10, pv, pi, ps) == (-1, "irs_score_topk_offer: M=65 exceeds max_rows=64")
            for k in (0, -1, 101, 1024, 1025, 2049, 1 << 20):
                assert call(px, 1, k, pv, pi, ps) == (-1, "irs_score_topk_offer: k must be in [1, 100]"), k
            for outs in ((None, pi, ps), (pv, None, ps), (pv, pi, None)):
                assert call(px, 1, 10, *outs) == (-1, "irs_score_topk_offer: null output"), outs
            if bound:  # the edges that are legal run
                for M, k in ((1, 1), (64, 100)):
                    assert call(px, M, k, pv, pi, ps) == (0, ""), (M, k)
                torch.cuda.synchronize()
                assert set(_n(ids)[:, :40].ravel().tolist()) <= set(S.tolist()) and (_n(ids)[:, 40:] == -1).all()
            else:
                assert call(px, 1, 10, pv, pi, ps) == (-2, "irs_score_topk_offer: no offer set is bound (irs_bind_offer_set)")
        finally:
            if bound:
                eng.unbind_offer_set()


def test_front_ends_take_one_based_ids(loops):
    m = loops
    net = InfluentialNet(m.cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in m.sd.items()})
    net.to(DEV)
    irn = IRSNN(m.cfg, net, DEV)
    irn.eval()
    S, comp = m.sets(150)
    seq, usr, tgt = _t(m.seqs), _t(m.users), _t(m.seqs[:, -1])
    comp1 = [ref.complement(S, m.N) + 1] * B5
    with torch.no_grad():
        for kw in (dict(), dict(stop_at_target=True), dict(beam_width=3), dict(beam_width=3, beam_stop="best"),
                   dict(beam_width=3, beam_stop="all")):
            a = irn.get_seq_in_batch(seq, usr, tgt, P5, 0, False, 3, offer=S + 1, exact_candidates=True, **kw)
            b = irn.get_seq_in_batch(seq, usr, tgt, P5, 0, False, 3, exclude=comp1, exact_candidates=True, **kw)
            assert np.array_equal(a[0], b[0]) and a[3] == b[3], kw
            assert np.isin(a[0][a[0] > 0] - 1, S).all()
        # sampled with the same seed (the front end draws it from torch's generator), the guide and the lookahead
        table = _t(np.random.default_rng(4).standard_normal((m.N + 1, 6)).astype(np.float32))
        for args, kw in (((P5, 0, True, 3), dict()), ((P5, 0, True, 3), dict(stop_at_target=True)),
                         ((P5, 0, False, 3), dict(guide=table, guide_k=5)), ((P5, 0, False, 3), dict(lookahead=3)),
                         ((P5, 0, False, 3), dict(trace=True, arrive_rank=128, stop_at_target=True))):
            torch.manual_seed(77)
            a = irn.get_seq_in_batch(seq, usr, tgt, *args, offer=S + 1, exact_candidates=True, **kw)
            torch.manual_seed(77)
            b = irn.get_seq_in_batch(seq, usr, tgt, *args, exclude=comp1, exact_candidates=True, **kw)
            assert np.array_equal(a[0], b[0]) and a[3] == b[3], kw
            assert np.isin(a[0][a[0] > 0] - 1, S).all()
        with pytest.raises(IndexError, match="offer set"):
            irn.get_seq_in_batch(seq, usr, tgt, P5, 0, False, 3, offer=[int(S[0]) + 1], exact_candidates=True)
        with pytest.raises(ValueError, match="offer"):
            irn.get_seq_in_batch(seq, usr, tgt, P5, 0, False, 3, offer=[0, 1])
        plain = irn.get_seq_in_batch(seq, usr, tgt, P5, 0, False, 3)
        again = irn.get_seq_in_batch(seq, usr, tgt, P5, 0, False, 3)
        assert np.array_equal(plain[0], again[0]), "nothing stays bound behind a call"


# ============================================================================ 6. recommend
@pytest.mark.parametrize("C", [10, 20, 128, 1000])
def test_recommend_equals_the_complement_exclusion(case, oracle, C):
    """Engine.recommend on the default config with a set bound, against the same call under the complement as everybody's
    exclusion list (N - C <= 4096 ids): ids, value bits and count; lp against the oracle's log-sum-exp of the WHOLE catalog."""
    c = case("default")
    M, L = 17, 60
    r = np.random.default_rng(C)
    S = c.subset(C, seed=6)
    comp = np.tile(ref.complement(S, c.N), (M, 1))
    seq = np.zeros((M, L), dtype=np.int64)
    hep = np.full(M, -1, dtype=np.int32)
    for mrow in range(0, M, 2):  # every other row has a window, half of it items of the set
        w = np.concatenate([r.choice(S, min(C, 10)) + 1, r.integers(1, c.N + 1, 20)])
        seq[mrow, :len(w)], hep[mrow] = w, len(w) - 1
    x = c.tx[:M]
    for n in (1, 20, 128):
        c.eng.bind_offer_set(_t(S), M)
        try:
            got = [_n(a) for a in c.eng.recommend(x, n, seqs=_t(seq), hep=_t(hep), k=min(1024, max(n, 100)))]
            bare = [_n(a) for a in c.eng.recommend(x, n, k=min(1024, max(n, 100)))]
        finally:
            c.eng.unbind_offer_set()
        held = c.eng.bind_exclusions(_t(comp))
        try:
            want = [_n(a) for a in c.eng.recommend(x, n, seqs=_t(seq), hep=_t(hep), k=min(1024, max(n, 100)))]
        finally:
            c.eng.unbind_exclusions()
        assert np.array_equal(got[1], want[1]), (C, n)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[3], want[3]), (C, n)
        for mrow in range(M):
            window = {int(v) for v in seq[mrow, :hep[mrow] + 1]}
            adm = [j for j in S if j + 1 not in window]
            assert got[3][mrow] == min(n, len(adm)) and bare[3][mrow] == min(n, C), (C, n, mrow)
            e_val, e_ids, _ = ref.topk(c.scores[mrow], np.array(adm, dtype=np.int64), n)
            assert np.array_equal(got[1][mrow], e_ids) and np.array_equal(_bits(got[0][mrow]), _bits(e_val)), (C, n, mrow)
            mx, sm = oracle.max_sumexp(c.scores[mrow])
            lse = mx + np.log(sm)
            live = e_ids >= 0
            assert (got[2][mrow][~live] == -np.inf).all()
            assert np.abs(got[2][mrow][live] - (e_val[live].astype(np.float64) - lse)).max(initial=0) <= LSE_TOL * max(1.0, abs(lse))


@pytest.mark.parametrize("gname,cfgname,C", [("irn_tiny", "tiny", 60), ("irn_default", "default", 1000), ("irn_default", "default", 15)])
def test_predict_next_takes_the_slate_from_the_set(golden, gname, cfgname, C):
    g = golden(gname)
    cfg = synth.make_config(cfgname)
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    net.to(DEV)
    irn = IRSNN(cfg, net, DEV)
    irn.eval()
    B = g["seqs"].shape[0]
    raw = [g["raw"][i, :g["raw_len"][i]] for i in range(B)]
    seq, u = _t(g["seqs"]), _t(g["users"])
    S1 = np.sort(np.random.default_rng(2).permutation(cfg.n_item)[:C]) + 1  # 1-based
    with torch.no_grad():
        got = _n(irn.predict_next(raw, seq, u, top_k=20, gap_len=0, use_h=True, offer=S1))
        rec = {k: _n(v) for k, v in irn.last_recommend.items()}
        count = rec["count"]
        comp1 = np.setdiff1d(np.arange(1, cfg.n_item + 1), S1)
        want = _n(irn.predict_next([np.concatenate([raw[i], comp1]) for i in range(B)], seq, u, top_k=20, gap_len=0, use_h=True))
        ref_rec = {k: _n(v) for k, v in irn.last_recommend.items()}
        assert np.array_equal(got, want) and np.array_equal(count, ref_rec["count"])
        assert np.array_equal(_bits(rec["scores"]), _bits(ref_rec["scores"])), "value bits"
        live = got > 0
        assert (rec["log_probs"][~live] == -np.inf).all() and (ref_rec["log_probs"][~live] == -np.inf).all()
        # lp: both calls take (max, sum exp) over the whole catalog, from two kernels whose float32 sums differ in order: twice the
        # log-sum-exp bound of tests/test_gpu_recommend.py, at the largest |lse| = |val - lp| of the batch
        lse = rec["scores"][live].astype(np.float64) - rec["log_probs"][live]
        assert np.abs(rec["log_probs"][live] - ref_rec["log_probs"][live]).max(initial=0) <= 2 * LSE_TOL * max(1.0, np.abs(lse).max(initial=0))
        for i in range(B):
            live = got[i][got[i] > 0]
            assert np.isin(live, S1).all() and not np.isin(live, raw[i]).any()
            assert count[i] == min(20, len(np.setdiff1d(S1, raw[i])))
        plain = _n(irn.predict_next(raw, seq, u, top_k=20, gap_len=0, use_h=True))
        assert not np.array_equal(plain, got), "nothing stays bound behind the call"


# ============================================================================ 7. state
def _script(eng, m, x):
    """A fixed script of calls; everything it returns, as host arrays."""
    out = []
    out += [_n(a) for a in eng.score_topk(x, 100, IRS_SWEEP_BF16)]
    out += [_n(a) for a in eng.generate_paths(*m.state(), P5, k=K5)]
    out += [_n(a) for a in eng.generate_paths(*m.state(), P5, k=K5, use_graph=True)]
    beams = eng.beam_search(*m.state(), P5, 3, k=K5, use_graph=True)
    out += [_n(beams[0]), _n(beams[2])]
    out += [_n(a) for a in eng.recommend(x, 20, log_probs=False) if a is not None]
    return out


def _equal_scripts(a, b):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), i


def test_bind_search_unbind_leaves_a_fresh_engines_answers(loops):
    m = loops
    fresh = make_engine(m.cfg, m.sd, max_rows=64, max_seqs=64, max_k=K5)
    x = _t(np.random.default_rng(1).standard_normal((8, m.cfg.emb_dim)).astype(np.float32))
    want = _script(fresh, m, x)
    S, _ = m.sets(40)
    eng = m.eng
    before = _script(eng, m, x)  # (captures the greedy and the beam step with nothing bound)
    _equal_scripts(before, want)
    eng.bind_offer_set(_t(S), 64)
    try:
        # a captured step from before the binding is not replayed after it: the same use_graph call now stays inside the set
        bound = _n(eng.generate_paths(*m.state(), P5, k=K5, use_graph=True)[0])
        assert np.isin(bound[bound > 0] - 1, S).all() and not np.array_equal(bound, before[5])
        stream = _n(eng.generate_paths(*m.state(), P5, k=K5)[0])
        assert np.array_equal(bound, stream)
        eng.beam_search(*m.state(), P5, 3, k=K5, use_graph=True)
        eng.recommend(x, 20)
    finally:
        eng.unbind_offer_set()
    _equal_scripts(_script(eng, m, x), want)  # (and a step captured under the binding is not replayed after the unbind)


def test_in_place_weight_update_needs_no_rebinding(loops):
    m = loops
    sd = {k: _t(v).clone() for k, v in m.sd.items()}
    eng = make_engine(m.cfg, sd, max_rows=64, max_seqs=64, max_k=K5)
    S, _ = m.sets(40)
    x = _t(np.random.default_rng(1).standard_normal((8, m.cfg.emb_dim)).astype(np.float32))
    eng.bind_offer_set(_t(S), 64)
    first = [_n(a).copy() for a in eng.score_topk_offer(x, 40)]
    g = torch.Generator(device="cpu").manual_seed(3)
    w = eng._weights["project.weight"]
    w.add_(0.5 * torch.randn(w.shape, generator=g).to(DEV))  # the engine's bound tensor, in place
    eng._weights["project.bias"].mul_(-1.0)
    eng.finalize()
    got = [_n(a) for a in eng.score_topk_offer(x, 40)] + [_n(a) for a in eng.generate_paths(*m.state(), P5, k=K5)]
    eng.unbind_offer_set()
    sd2 = {k: v.clone() for k, v in eng._weights.items()}
    fresh = make_engine(m.cfg, sd2, max_rows=64, max_seqs=64, max_k=K5)
    fresh.bind_offer_set(_t(S), 64)
    want = [_n(a) for a in fresh.score_topk_offer(x, 40)] + [_n(a) for a in fresh.generate_paths(*m.state(), P5, k=K5)]
    fresh.unbind_offer_set()
    _equal_scripts(got, want)
    assert not np.array_equal(first[1], got[1]), "the update changed the ranking"


# ============================================================================ 8. the other two front ends
def test_rec2inf_and_evaluator_take_the_set(golden):
    from influentialrs_amd.model.evaluator import Evaluator
    from influentialrs_amd.model.rec2inf import Rec2Inf
    from influentialrs_amd.model.uRS import SampleNet
    cfg = synth.make_config("eval_tiny")
    net = SampleNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 17, evaluator=True).items()})
    net.to(DEV)
    N, L, B, P = cfg.n_item, cfg.max_len, 12, 6
    g = np.random.default_rng(8)
    S1 = np.sort(g.permutation(N)[:200]) + 1  # 1-based
    comp1 = np.setdiff1d(np.arange(1, N + 1), S1)
    # Rec2Inf: the guided search under the set, against the complement as everybody's exclusion list
    r2i = Rec2Inf(cfg, net, DEV)
    lens = [L + 7, 1, 2, L - 2, L - 1, L]
    hist = [g.permutation(N)[:lens[b % 6]] + 1 for b in range(B)]
    targets = torch.from_numpy(g.choice(S1, B))
    table = _t(g.standard_normal((N + 1, 8)).astype(np.float32))
    for stop in (False, True):
        a = r2i.get_seq_in_batch(hist, targets, table, guide_k=5, max_path_len=P, stop_at_target=stop, exact_candidates=True, offer=S1)
        b = r2i.get_seq_in_batch(hist, targets, table, guide_k=5, max_path_len=P, stop_at_target=stop, exact_candidates=True,
                                 exclude=[comp1] * B)
        assert np.array_equal(a[0], b[0]) and a[3] == b[3], stop
        assert np.isin(a[0][a[0] > 0], S1).all()
    # Evaluator.predict_next: the slate is the set's members of the plain ranked list, in its order
    ev = Evaluator(cfg, net, DEV)
    ev.eval()
    seqs = _t(golden("eval_accuracy_tiny")["seqs"].astype(np.int64))
    for use_h in (True, False):
        with torch.no_grad():
            got = _n(ev.predict_next(seqs, top_k=20, use_h=use_h, offer=S1))
            count = _n(ev.last_recommend["count"])
            plain = _n(ev.predict_next(seqs, top_k=100, use_h=use_h))
        for i in range(got.shape[0]):
            members = [j for j in plain[i] if j in set(S1.tolist())]
            assert len(members) >= 20, "the plain top 100 holds 20 items of a set of 200 of 257"
            assert got[i].tolist() == members[:20] and count[i] == 20, (i, use_h)


# ============================================================================ 9. the survivor pass alone repairs from the set
def test_ensure_survivors_repairs_from_the_set(case):
    """Rows whose window holds the best 10 of the set show a list with no survivor; the public pass rewrites it with the best
    `want` items of the set outside the window -- never with an item outside the set, however well it scores."""
    c = case("default")  # max_len 60
    M, k, want, L = 9, 10, 4, 60
    S = c.subset(300, seed=3)
    c.eng.bind_offer_set(_t(S), 80)
    try:
        val, ids, st = c.eng.score_topk_offer(c.tx[:M], k)
        lists = _n(ids)
        seq = np.zeros((M, L), dtype=np.int64)
        hep = np.full(M, -1, dtype=np.int32)
        for m in range(0, M, 2):  # every other row is starved
            seq[m, :k], hep[m] = lists[m] + 1, k - 1
        status = torch.zeros(M, dtype=torch.int32, device=DEV)
        c.eng.ensure_survivors(c.tx[:M], _t(seq), _t(hep), val, ids, status, want=want)
        val, ids, status = _n(val), _n(ids), _n(status)
    finally:
        c.eng.unbind_offer_set()
    for m in range(M):
        if m % 2:
            assert np.array_equal(ids[m], lists[m]) and status[m] == 0, m
            continue
        rest = np.setdiff1d(S, lists[m])
        e_val, e_ids, _ = ref.topk(c.scores[m], rest, want)
        assert np.array_equal(ids[m, :want], e_ids) and np.array_equal(_bits(val[m, :want]), _bits(e_val)), m
        assert ids[m, want] == -1 and status[m] == 8, m  # IRS_ROW_RESCUED
