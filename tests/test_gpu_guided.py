"""-m gpu: the guided choice (include/irs_hip.h, "guided choice": irs_bind_guide; guide= / guide_k= in the engine and the front
ends; model/rec2inf.py), against the numpy statement of tests/guided_ref.py.

Ids, windows, hep and status words are compared exactly everywhere.  The step kernel alone runs on synthetic lists built to sit
on its edges.  The loops are compared with a HOST-STEPPED loop made of the engine's own public calls (decode at hep, score_topk)
and the statement's step, as tests/test_gpu_exclusions.py does it, so both sides score the same rows with the same kernels and
only the search logic is the statement's.

Two float bounds appear.  The trace test compares lp_item with score_gather - score_lse on the same decoder rows under the bound
tests/test_gpu_path_trace.py uses for that quantity where the launches differ: LP = 2 LOGIT + 4e-6 max(1, |lse|), LOGIT = 4e-5
max_j ||W_j||_1.  The Rec2Inf decode test uses the project's small-batch decoder tier, 2e-5 per element."""
import functools

import numpy as np
import pytest
import torch

import exclusion_ref
import guided_ref as ref
import path_ref
from gpu_util import make_engine, path_only_engine
from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_ROW_NO_CANDIDATE, IRS_ROW_RESCUED, IRS_SWEEP_BF16
from influentialrs_amd.engine import IrsError
from influentialrs_amd.model import Rec2Inf
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
from influentialrs_amd.model.rec2inf import rec2inf_windows
from influentialrs_amd.model.uRS import SampleNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BINARY, FLOAT = ref.BINARY, ref.FLOAT
NAMES4 = ("paths", "seq", "hep", "status")
N_STEP = 600  # catalog of the step-only engines: the table has 601 rows


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
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b.astype(a.dtype))), (name, np.argwhere(a != b)[:8])


class _Guide:
    """A guide bound for the time of a with-block."""

    def __init__(self, eng, table, k_c):
        self.eng, self.table, self.k_c = eng, table, k_c

    def __enter__(self):
        self.held = self.eng.bind_guide(_t(self.table), self.k_c)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.eng.unbind_guide()


def _table(g, kind, F, rows):
    """Half of the rows repeat one of six prototypes (exact ties between distinct items), the rest are their own.  Binary: any
    nonzero byte is a 1.  Float: prototypes on a dyadic grid, the other rows generic normals, so the chain rounds at every step."""
    if kind == BINARY:
        protos = g.integers(0, 2, size=(6, F))
        t = g.integers(0, 2, size=(rows, F))
        rep = g.random(rows) < 0.5
        t[rep] = protos[g.integers(0, 6, size=int(rep.sum()))]
        return (t * g.integers(1, 256, size=(rows, F))).astype(np.uint8)
    protos = (g.integers(-4, 5, size=(6, F)) * 0.5).astype(np.float32)
    t = g.standard_normal((rows, F)).astype(np.float32)
    rep = g.random(rows) < 0.5
    t[rep] = protos[g.integers(0, 6, size=int(rep.sum()))]
    return t


# ============================================================================ 1. the step kernel alone
@functools.lru_cache(maxsize=None)
def _step_engine(L):
    return path_only_engine(L, n_item=N_STEP)  # (L > 256: the engine opens a long-window context, 16-register window image)


def _step_case(L, B, k, k_c, seed):
    """Rows cycle through hep in {0, mid, L-3 (last grow), L-2 (shift)}, through the number of leading candidates the window
    hides (0 .. k), through lists that end early at a negative id, and through the target: none, one of the first k_c
    survivors, a candidate the window hides, any item."""
    g = np.random.default_rng(seed)
    heps = [0, max(0, (L - 2) // 2), max(0, L - 3), L - 2]
    hides = [0, 1, 2, k_c - 1, k_c, k - k_c, k - 1, k]
    off = int(g.integers(0, 40))
    seq = g.integers(6001, 9000, size=(B, L)).astype(np.int64)  # filler: no item of the catalog
    hep = np.zeros(B, dtype=np.int32)
    val = np.zeros((B, k), dtype=np.float32)
    ids0 = np.zeros((B, k), dtype=np.int64)
    info = []
    for r in range(B):
        q = r + off
        he = heps[q % 4]
        c = int(np.clip(hides[(q // 4) % 8], 0, min(k, he + 1)))
        ids0[r] = g.permutation(N_STEP)[:k]
        val[r] = np.sort(g.permutation(4 * k)[:k].astype(np.float32) * 0.125 - 7.0)[::-1]
        end = k
        if q % 3 == 1:  # the list ends early: sometimes before k_c survivors, sometimes before any; valid ids follow the -1
            end = min(k, c + int(g.integers(0, k_c + 2)))
            if end < k:
                ids0[r, end] = -1
        wl = he + 1
        if wl >= 3:
            seq[r, g.integers(0, wl)] = 0
        seq[r, g.permutation(wl)[:c]] = ids0[r, :c] + 1
        surv = [int(i) + 1 for i in ids0[r, c:end]][:k_c]
        if surv and he + 1 <= L - 2:
            seq[r, g.integers(he + 1, L - 1)] = surv[0]  # stale: only past hep, not window
        tm = (q // 2) % 5
        if tm == 0:
            t = 0
        elif tm == 1 and surv:
            t = surv[int(g.integers(0, len(surv)))]
        elif tm == 2 and c > 0:
            t = int(ids0[r, 0]) + 1
        else:
            t = int(g.integers(1, N_STEP + 1))
        seq[r, L - 1] = t
        hep[r] = he
        info.append(dict(he=he, c=c, n_surv=len(surv), t=t, t_offered=t in surv, t_hidden=(tm == 2 and c > 0), surv=surv))
    status = np.array([0, 1, 4, 5], dtype=np.int32)[(np.arange(B) // 2) % 4]
    return seq, hep, val, ids0, status, info


def _run_step(eng, seq, hep, val, ids0, step, paths, status, guard=3):
    """irs_path_step on the leading B rows of buffers that carry `guard` poisoned rows more; checks that those, val and ids0
    are untouched."""
    B = seq.shape[0]

    def padded(a, fill):
        return _t(np.concatenate([a, np.full((guard,) + a.shape[1:], fill, dtype=a.dtype)]))
    d_seq, d_hep, d_paths, d_st = padded(seq, 4242), padded(hep, 1), padded(paths, 555.0), padded(status, 8)
    d_val, d_ids = _t(val), _t(ids0)
    eng.path_step(d_seq[:B], d_hep[:B], d_val, d_ids, step, d_paths[:B], d_st[:B])
    assert (_n(d_seq[B:]) == 4242).all() and (_n(d_hep[B:]) == 1).all()
    assert (_n(d_paths[B:]) == 555.0).all() and (_n(d_st[B:]) == 8).all()
    assert np.array_equal(_bits(_n(d_val)), _bits(val)) and np.array_equal(_n(d_ids), ids0)
    return _n(d_seq[:B]), _n(d_hep[:B]), _n(d_paths[:B]), _n(d_st[:B])


def _step_cases():
    kinds = [(BINARY, F) for F in (1, 18, 32, 33, 1024)] + [(FLOAT, F) for F in (1, 3, 4, 64, 130, 512)]
    Ls, Bs, kcs = (8, 50, 200, 320), (1, 5, 257), (1, 5, 32)
    out = []
    for i, (kind, F) in enumerate(kinds):
        for j in range(3):
            k_c = kcs[(i + j) % 3]
            k = 100 if k_c == 32 else (10, 100)[(i + j) % 2]
            B = Bs[(i + 2 * j) % 3]
            if B == 257 and F > 64:
                B = 5  # (the statement walks F features per row in Python: the wide tables get the small batches)
            out.append((Ls[(i + j) % 4], B, k, k_c, kind, F))
    # every value is used, the partial last workgroup at both window sizes, kinds and with k_c = 32
    for col, values in ((0, Ls), (1, Bs), (2, (10, 100)), (3, kcs)):
        assert {c[col] for c in out} == set(values)
    big = [c for c in out if c[1] == 257]
    assert {c[4] for c in big} == {BINARY, FLOAT} and {c[0] > 256 for c in big} == {True, False} and {c[3] for c in big} == set(kcs)
    assert {(c[0] > 256, c[4]) for c in out} == {(a, b) for a in (True, False) for b in (BINARY, FLOAT)}
    return out


@pytest.mark.parametrize("L,B,k,k_c,kind,F", _step_cases())
def test_guided_step_equals_the_statement(L, B, k, k_c, kind, F):
    eng = _step_engine(L)
    seed = L * 10007 + B * 101 + k + 7 * k_c + F
    table = _table(np.random.default_rng(seed + 1), kind, F, N_STEP + 1)
    seq, hep, val, ids0, status, info = _step_case(L, B, k, k_c, seed)
    step, path_ld = 2, 5
    paths = np.full((B, path_ld), 777.0, dtype=np.float32)
    want = ref.path_step(seq, hep, val, ids0, step, paths, status, table, kind, k_c)
    greedy = path_ref.path_step(seq, hep, val, ids0, step, paths, status)
    with _Guide(eng, table, k_c):
        got = _run_step(eng, seq, hep, val, ids0, step, paths, status)
        again = _run_step(eng, seq, hep, val, ids0, step, paths, status)
    _same(got, want, ("seq", "hep", "paths", "status"))
    _same(again, got, ("seq", "hep", "paths", "status"))
    g_seq, g_hep, g_paths, g_st = got
    assert (g_paths[:, [0, 1, 3, 4]] == 777.0).all() and ((g_st & 5) == status).all()
    for r, d in enumerate(info):
        assert bool(g_st[r] & IRS_ROW_NO_CANDIDATE) == (d["n_surv"] == 0), (r, d)
        if d["n_surv"] == 0:
            assert g_paths[r, step] == 0 and np.array_equal(g_seq[r], seq[r]) and g_hep[r] == d["he"]
            continue
        assert int(g_paths[r, step]) in d["surv"]
        if d["t"] == 0 or k_c == 1:
            assert g_paths[r, step] == d["surv"][0] == greedy[2][r, step]
        if d["t_offered"]:
            dists = (ref.dist_float_many if kind == FLOAT else ref.dist_binary_many)(table, d["t"], d["surv"])
            assert dists[d["surv"].index(int(g_paths[r, step]))] == 0, "the offered target is at distance 0: it, or an earlier twin, wins"
    _same(_run_step(eng, seq, hep, val, ids0, step, paths, status), greedy, ("seq", "hep", "paths", "status"))  # unbound again
    if B == 257:  # every kind of row did occur, and the table did matter
        assert any(d["t"] == 0 and d["n_surv"] for d in info) and any(d["t_offered"] for d in info)
        assert any(d["t_hidden"] and d["n_surv"] for d in info) and any(d["n_surv"] == 0 for d in info)
        assert any(0 < d["n_surv"] < k_c for d in info) or k_c == 1
        if k_c > 1:
            assert (g_paths[:, step] != greedy[2][:, step]).any()
            tied = 0
            for d in info:
                if d["n_surv"] > 1 and 1 <= d["t"]:
                    dd = (ref.dist_float_many if kind == FLOAT else ref.dist_binary_many)(table, d["t"], d["surv"])
                    tied += int((dd == dd.min()).sum() > 1)
            assert tied >= 1, "a tie of the nearest was meant to occur"


# ============================================================================ 2. with exclusions, no_repeat and exact candidates
@pytest.mark.parametrize("kind,F", [(BINARY, 18), (FLOAT, 6)])
@pytest.mark.parametrize("L", [50, 320])
def test_guided_step_with_bound_exclusions_and_no_repeat(L, kind, F):
    eng = _step_engine(L)
    B, k, k_c, step, path_ld, n_excl = 9, 100, 5, 2, 6, 70
    seed = 31 * L + F
    g = np.random.default_rng(seed)
    table = _table(g, kind, F, N_STEP + 1)
    seq, hep, val, ids0, status, info = _step_case(L, B, k, k_c, seed)
    paths = np.zeros((B, path_ld), dtype=np.float32)
    excl = np.full((B, n_excl), -1, dtype=np.int64)
    for r in range(B):
        lead = ids0[r, :12].copy()
        lead = lead[lead >= 0]
        if len(lead) >= 4:
            paths[r, 0], paths[r, 1] = lead[1] + 1, lead[3] + 1  # the row's own earlier choices: gone under no_repeat
            excl[r, :2] = lead[[0, 2]]                             # and two more through the list
        excl[r, 2:40] = g.integers(0, N_STEP, size=38)
    want = ref.path_step(seq, hep, val, ids0, step, paths, status, table, kind, k_c, excl, N_STEP, no_repeat=True)
    only_guide = ref.path_step(seq, hep, val, ids0, step, paths, status, table, kind, k_c)
    scratch = eng.bind_exclusions(_t(excl), B, True)
    try:
        with _Guide(eng, table, k_c):
            got = _run_step(eng, seq, hep, val, ids0, step, paths, status)
    finally:
        torch.cuda.synchronize()
        eng.unbind_exclusions()
    _same(got, want, ("seq", "hep", "paths", "status"))
    assert (want[2][:, step] != only_guide[2][:, step]).any(), "the lists were meant to move a choice"
    for r in range(B):
        assert got[2][r, step] == 0 or not exclusion_ref.is_member(got[2][r, step], seq[r, :hep[r] + 1], excl[r], N_STEP, paths[r], step, True)


class _Model:
    """An engine with its inputs, and the stand-alone calls the host-stepped loops are made of."""

    def __init__(self, cfg, sd, seq, users, rows, evaluator=False):
        self.cfg, self.n_item, self.L = cfg, cfg.n_item, cfg.max_len
        self.eng = make_engine(cfg, sd, evaluator=evaluator, max_rows=rows, max_seqs=rows, max_k=cfg.n_item if cfg.n_item <= 512 else 100)
        self.seq = np.asarray(seq, dtype=np.int64)
        self.users = None if users is None else np.asarray(users, dtype=np.int64)
        self.B = len(self.seq)
        self.hep = np.full(self.B, self.L - 2, dtype=np.int32)

    def usr(self):
        return None if self.users is None else _t(self.users)

    def lists(self, seq, hep, k=None):
        """(val, ids0) of the rows at hep: k = None is the exact ranking of the whole catalog."""
        _, xr, _ = self.eng.decode(_t(seq), self.usr(), want_x=False, pos=_t(hep))
        v, i, _ = self.eng.score_topk(xr, self.n_item if k is None else k, IRS_SWEEP_BF16)
        return _n(v), _n(i)


def _host_guided(m, P, table, kind, k_c, excl=None, no_repeat=False, exact=False, until=False, seq=None, hep=None):
    """(paths, seq, hep, status, repaired rows) of the guided greedy search, stepped on the host.  until: a user is frozen after
    the step that chose its target, its tail zero."""
    seq, hep = (m.seq if seq is None else seq).copy(), (m.hep if hep is None else hep).copy()
    paths, status = np.zeros((m.B, P), dtype=np.float32), np.zeros(m.B, dtype=np.int32)
    fin = np.zeros(m.B, dtype=np.int32)
    repaired = 0
    for step in range(P):
        if until and fin.all():
            break
        if exact:
            fv, fi = m.lists(seq, hep)
            val, ids = fv[:, :100].copy(), fi[:, :100].copy()
            val, ids, st2, starved = exclusion_ref.ensure_survivors(seq, hep, val, ids, status, k_c, lambda r: (fv[r], fi[r]), excl,
                                                                    m.n_item, fin=fin, paths=paths, step=step, no_repeat=no_repeat)
            repaired += len(starved)
        else:
            val, ids = m.lists(seq, hep, 100)
            st2 = status
        s2, h2, p2, st2 = ref.path_step(seq, hep, val, ids, step, paths, st2, table, kind, k_c, excl, m.n_item, no_repeat)
        live = fin == 0
        seq[live], hep[live], paths[live], status[live] = s2[live], h2[live], p2[live], st2[live]
        if until:
            fin |= (live & (paths[:, step] == seq[:, m.L - 1])).astype(np.int32)
    return paths, seq, hep, status, repaired


_MODELS = {}


def _model(name, golden):
    """tiny / default: the golden shapes and users (N = 257, L = 12 / N = 3415, L = 60), P = 20.  L320: the tiny decoder behind a
    long window (n_item = 300, L = 320), P = 4."""
    if name in _MODELS:
        return _MODELS[name]
    if name in ("tiny", "default"):
        g = golden(f"irn_{name}")
        cfg = synth.make_config(name)
        m = _Model(cfg, synth.irn_state_dict(cfg, 1234), g["seqs"], g["users"], 64)
        m.P, m.golden_paths = int(g["meta"][2]), g["paths"]
    else:
        cfg = synth.make_config("tiny", n_item=300, max_len=320)
        rg = np.random.default_rng(320)
        seq = np.zeros((3, 320), dtype=np.int64)
        seq[0, 30:319] = rg.integers(1, 301, size=289)
        seq[1, 300:319] = rg.permutation(300)[:19] + 1
        seq[2, 1:319] = rg.integers(1, 301, size=318)
        seq[:, 319] = [299, 7, 150]
        m = _Model(cfg, synth.irn_state_dict(cfg, 1234), seq, np.array([3, 11, 5]), 16)
        m.P = 4
    m.name = name
    rg = np.random.default_rng(len(name))
    m.tables = {BINARY: _table(rg, BINARY, 18, m.n_item + 1), FLOAT: _table(rg, FLOAT, 12, m.n_item + 1)}
    _MODELS[name] = m
    return m


def _greedy(m, use_graph=False, **kw):
    seq, hep = _t(m.seq), _t(m.hep)
    paths, status = m.eng.generate_paths(seq, m.usr(), hep, m.P, k=100, sweep=IRS_SWEEP_BF16, use_graph=use_graph, **kw)
    return _n(paths), _n(seq), _n(hep), _n(status)


@pytest.mark.parametrize("name", ["tiny", "L320"])
def test_loop_with_exclusions_and_exact_candidates_repairs_to_k_c(name, golden):
    """Every user's list hides its step-0 top-100 but the last two entries: two admissible candidates where k_c = 5 are wanted, so
    the survivor pass (want = k_c) must hand the step the exact best five outside window + list + path."""
    m = _model(name, golden)
    k_c, P = 5, min(m.P, 6)
    top = m.lists(m.seq, m.hep, 100)[1]
    excl = top.copy()
    excl[:, -2:] = -1
    for kind in (BINARY, FLOAT):
        table = m.tables[kind]
        want = _host_guided(m, P, table, kind, k_c, excl, True, True)
        assert want[4] >= m.B, "every user was meant to be starved at step 0 at least"
        seq, hep = _t(m.seq), _t(m.hep)
        paths, status = m.eng.generate_paths(seq, m.usr(), hep, P, k=100, sweep=IRS_SWEEP_BF16, exclude=_t(excl), no_repeat=True,
                                             exact_candidates=True, guide=_t(table), guide_k=k_c)
        got = (_n(paths), _n(seq), _n(hep), _n(status))
        _same(got, want[:4], NAMES4)
        assert (got[3] & IRS_ROW_RESCUED).all() and not (got[3] & IRS_ROW_NO_CANDIDATE).any() and (got[0] != 0).all()
        # without the pass the same call sees only the two entries left: a different (poorer) choice for somebody
        seq, hep = _t(m.seq), _t(m.hep)
        poor, _ = m.eng.generate_paths(seq, m.usr(), hep, P, k=100, sweep=IRS_SWEEP_BF16, exclude=_t(excl), no_repeat=True,
                                       guide=_t(table), guide_k=k_c)
        _same((_n(poor),), (_host_guided(m, P, table, kind, k_c, excl, True, False)[0],), ("paths",))
        assert (_n(poor)[:, 0] != got[0][:, 0]).any()


# ============================================================================ 3. irs_generate_paths
@pytest.mark.parametrize("name", ["tiny", "default"])
def test_generate_paths_equals_the_composition_stream_and_graph(name, golden):
    m = _model(name, golden)
    plain = _greedy(m)
    wants = {}
    for kind in (BINARY, FLOAT):
        table = m.tables[kind]
        want = wants[kind] = _host_guided(m, m.P, table, kind, 5)
        got = _greedy(m, guide=_t(table), guide_k=5)
        _same(got, want[:4], NAMES4)
        _same(_greedy(m, use_graph=True, guide=_t(table), guide_k=5), got, NAMES4)
        assert (got[0] != plain[0]).any(), "the guide was meant to move a choice"
        _same(_greedy(m, guide=_t(table), guide_k=1), plain, NAMES4)  # k_c = 1 is the greedy search
    # bind, captured call, rebind another table, captured call on the SAME buffers: each call its own table's paths
    eng = m.eng
    seq, hep = _t(m.seq), _t(m.hep)
    paths = torch.zeros((m.B, m.P), dtype=torch.float32, device=DEV)
    status = torch.zeros(m.B, dtype=torch.int32, device=DEV)

    def run():
        seq.copy_(_t(m.seq))
        hep.copy_(_t(m.hep))
        paths.fill_(-3.0)
        eng.generate_paths(seq, m.usr(), hep, m.P, k=100, sweep=IRS_SWEEP_BF16, use_graph=True, paths=paths, status=status)
        return _n(paths).copy(), _n(seq).copy(), _n(hep).copy(), _n(status).copy()

    before = run()
    with _Guide(eng, m.tables[BINARY], 5):
        first = run()
    with _Guide(eng, m.tables[FLOAT], 5):
        second = run()
    after = run()
    _same(first, wants[BINARY][:4], NAMES4)
    _same(second, wants[FLOAT][:4], NAMES4)
    assert (first[0] != second[0]).any()
    _same(after, before, NAMES4)
    _same(before, plain, NAMES4)
    # unbound, the committed 20-step golden paths come back (they are cut at the target: the until loop writes them that way)
    gp, gst, _, _ = eng.generate_paths_until(_t(m.seq), m.usr(), _t(m.hep), m.P, check_every=1)
    assert np.array_equal(_n(gp), m.golden_paths) and not _n(gst).any()


# ============================================================================ 4. irs_generate_paths_until
@pytest.mark.parametrize("check_every", [1, 3])
@pytest.mark.parametrize("kind", [BINARY, FLOAT])
def test_generate_paths_until_with_a_guide(kind, check_every, golden):
    """Targets: a third of the users get one of their own step-0 top-5 (unique features: distance 0 only to itself, so the guided
    step offers it at once), a third an item ranked 6 .. 40 at step 0 (it may or may not come within the first five survivors
    later), the rest an item outside their step-0 top-100."""
    m = _model("tiny", golden)
    rg = np.random.default_rng(17)
    if kind == FLOAT:
        table = rg.standard_normal((m.n_item + 1, 8)).astype(np.float32)
    else:
        table = ((np.arange(m.n_item + 1)[:, None] >> np.arange(9)) & 1).astype(np.uint8)  # the item's own number: unique rows
    seq = m.seq.copy()

    def step0(s):
        _, ids = m.lists(s, m.hep, 100)
        return [[x[0] for x in path_ref.survivors(s[b, :m.L - 1], np.zeros(100), ids[b], 100)] for b in range(m.B)]

    surv = step0(seq)
    for b in range(m.B):
        outside = [i for i in range(1, m.n_item + 1) if i not in surv[b] and i not in seq[b]]
        seq[b, -1] = (surv[b][0], surv[b][int(rg.integers(5, 40))], outside[int(rg.integers(0, len(outside)))])[b % 3]
    for attempt in range(8):  # the IRN mask reads the target: settle every third user on a target that its own window ranks in the top 5
        surv = step0(seq)
        loose = [b for b in range(0, m.B, 3) if seq[b, -1] not in surv[b][:5]]
        if not loose:
            break
        for b in loose:
            seq[b, -1] = surv[b][attempt % 5]
    assert not loose
    P = 8
    want = _host_guided(m, P, table, kind, 5, seq=seq)

    def cut(paths):
        out = paths.copy()
        for b in range(m.B):
            pos = np.where(out[b] == seq[b, -1])[0]
            if len(pos):
                out[b, pos[0] + 1:] = 0
        return out

    s, h = _t(seq), _t(m.hep)
    plain, pst = m.eng.generate_paths(s, m.usr(), h, P, k=100, sweep=IRS_SWEEP_BF16, guide=_t(table), guide_k=5)
    _same((_n(plain),), (want[0],), ("paths",))
    gp, gst, steps, row_steps = m.eng.generate_paths_until(_t(seq), m.usr(), _t(m.hep), P, k=100, sweep=IRS_SWEEP_BF16,
                                                           check_every=check_every, guide=_t(table), guide_k=5)
    _same((_n(gp),), (cut(_n(plain)),), ("paths",))
    host = _host_guided(m, P, table, kind, 5, until=True, seq=seq)
    _same((_n(gp), _n(gst)), (host[0], host[3]), ("paths", "status"))
    arrived = [(p == t).any() for p, t in zip(_n(gp), seq[:, -1])]
    assert sum(arrived) >= 1 and sum(arrived) < m.B, arrived
    assert all(arrived[b] and _n(gp)[b, 0] == seq[b, -1] for b in range(0, m.B, 3)), "an offered target at distance 0 is taken"
    assert row_steps < m.B * P, "finished users were retired"


# ============================================================================ 5. with a bound trace
def test_trace_records_the_guided_choice(golden):
    m = _model("tiny", golden)
    cfg = m.cfg
    sd = synth.irn_state_dict(cfg, 1234)
    table, P = m.tables[FLOAT], 8
    seq, hep = _t(m.seq), _t(m.hep)
    paths, status, (lp_item, lp_target, rank) = m.eng.generate_paths(seq, m.usr(), hep, P, k=100, sweep=IRS_SWEEP_BF16, trace=True,
                                                                     guide=_t(table), guide_k=5)
    paths, lp_item = _n(paths), _n(lp_item)
    _same((paths,), (_host_guided(m, P, table, FLOAT, 5)[0],), ("paths",))
    unguided = _greedy(m)[0][:, :P]
    assert (paths != unguided).any()
    win, he = [np.array(r) for r in m.seq], [int(x) for x in m.hep]
    LOGIT = 4e-5 * float(np.abs(sd["project.weight"]).sum(axis=1).max())
    moved = 0
    for i in range(P):
        _, xr, _ = m.eng.decode(_t(np.stack(win)), m.usr(), want_x=False, pos=_t(np.array(he, dtype=np.int32)))
        mx, sm = (_n(v).astype(np.float64) for v in m.eng.score_lse(xr))
        lse = mx + np.log(sm)
        e = _n(m.eng.score_gather(xr, _t((paths[:, i:i + 1] - 1).astype(np.int64))))[:, 0].astype(np.float64)
        e_greedy = _n(m.eng.score_gather(xr, _t((unguided[:, i:i + 1] - 1).astype(np.int64))))[:, 0].astype(np.float64)
        LP = 2 * LOGIT + 4e-6 * max(1.0, float(np.abs(lse).max()))
        err = np.abs(lp_item[:, i].astype(np.float64) - (e - lse))
        print(f"step {i}: max |lp_item - (gather - lse)| {err.max():.3g} bound {LP:.3g}")
        assert (err <= LP).all()
        moved += int((np.abs(e - e_greedy) > 2 * LP).sum())
        for b in range(m.B):
            win[b], he[b] = path_ref.advance(win[b], he[b], int(paths[b, i]))
    assert moved >= 1, "somewhere the guided choice scores clearly apart from the greedy one: lp_item is the guided item's"
    assert (lp_item < 0).all() and (_n(rank) >= 1).all() and (_n(lp_target) < 0).all()


# ============================================================================ 6. Rec2Inf on SampleNet
def _sample_net(cfgname="eval_tiny"):
    cfg = synth.make_config(cfgname)
    net = SampleNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 17, evaluator=True).items()})
    net.to(DEV)
    return cfg, net


def _histories(g, B, L, n_item):
    lens = [L + 7, 1, 2, L - 2, L - 1, L]
    return [g.permutation(n_item)[:lens[b % 6]] + 1 for b in range(B)]


@pytest.mark.parametrize("cfgname,B", [("eval_tiny", 1), ("eval_tiny", 12), ("eval_tiny", 400), ("c2", 400)])
def test_the_consumed_row_never_sees_the_target_slot(cfgname, B):
    """Premise of Rec2Inf's window layout: on a causal context the row at hep <= L - 2 does not attend slot L - 1.  One sequence,
    twelve and four hundred take the latency routes and (c2: d = 128, from 384 sequences) the sequence-resident launch."""
    cfg = synth.make_config(cfgname)
    eng = make_engine(cfg, synth.irn_state_dict(cfg, 17, evaluator=True), evaluator=True, max_rows=max(B, 64), max_seqs=max(B, 8))
    g = np.random.default_rng(B)
    win, hep, _ = rec2inf_windows(_histories(g, B, cfg.max_len, cfg.n_item), g.integers(1, cfg.n_item + 1, size=B), cfg.max_len, DEV)
    assert (win[:, -1] != 0).all() and int(hep.max()) == cfg.max_len - 2
    _, with_t, _ = eng.decode(win, None, want_x=False, pos=hep)
    seq_route = eng.decoder_seq_last
    bare = win.clone()
    bare[:, -1] = 0
    _, without, _ = eng.decode(bare, None, want_x=False, pos=hep)
    err = float((with_t - without).abs().max())
    print(f"{cfgname} B={B}: max |row(target in slot L-1) - row(slot L-1 zero)| = {err:.3g} (sequence-resident: {seq_route})")
    assert err <= 2e-5
    assert seq_route == (cfgname == "c2")


def test_rec2inf_paths_stop_and_success_count():
    cfg, net = _sample_net()
    L, N, B, P, k_c = cfg.max_len, cfg.n_item, 12, 10, 5
    r2i = Rec2Inf(cfg, net, DEV)
    g = np.random.default_rng(5)
    hist = _histories(g, B, L, N)
    table = g.standard_normal((N + 1, 8)).astype(np.float32)
    # a third of the targets from the user's own step-0 top-5 (they arrive at once), the rest anywhere
    win0, hep0, _ = rec2inf_windows(hist, np.zeros(B, dtype=np.int64), L, DEV)
    eng = net._hip.get(B, B)
    _, xr, _ = eng.decode(win0, None, want_x=False, pos=hep0)
    _, ids, _ = eng.score_topk(xr, 100, IRS_SWEEP_BF16)
    ids, targets = _n(ids), g.integers(1, N + 1, size=B)
    for b in range(0, B, 3):
        surv = [s[0] for s in path_ref.survivors(_n(win0)[b, :int(hep0[b]) + 1], np.zeros(100), ids[b], 5)]
        targets[b] = surv[int(g.integers(0, 5))]
    # (b) the statement, driven step by step through the model's own decode_rows and the engine's score_topk
    win, hep, _ = rec2inf_windows(hist, targets, L, DEV)
    seq, he = _n(win).copy(), _n(hep).copy()
    assert (seq[:, -1] == targets).all()
    paths, status = np.zeros((B, P), dtype=np.float32), np.zeros(B, dtype=np.int32)
    rows_b = torch.arange(B, device=DEV)
    for i in range(P):
        x = net.decode_rows(_t(seq), rows_b, _t(he.astype(np.int64)))
        v, idx, _ = eng.score_topk(x, 100, IRS_SWEEP_BF16)
        seq, he, paths, status = ref.path_step(seq, he, _n(v), _n(idx), i, paths, status, table, FLOAT, k_c)
    want = paths.copy()
    arrivals = 0
    for b in range(B):
        pos = np.where(want[b] == targets[b])[0]
        if len(pos):
            arrivals += 1
            want[b, pos[0] + 1:] = 0
    tt = torch.from_numpy(targets)
    full = r2i.get_seq_in_batch(hist, tt, _t(table), guide_k=k_c, max_path_len=P, stop_at_target=False)
    stop = r2i.get_seq_in_batch(hist, tt, _t(table), guide_k=k_c, max_path_len=P, stop_at_target=True)
    assert full[0].dtype == np.float32 and full[0].shape == (B, P)
    assert np.array_equal(full[0], want), np.argwhere(full[0] != want)[:8]                      # (b)
    assert np.array_equal(stop[0], full[0])                                                    # (c)
    assert full[3] == stop[3] == arrivals and 4 <= arrivals < B                                 # (d)
    assert all(full[0][b, 0] == targets[b] for b in range(0, B, 3))
    assert np.array_equal(full[1], targets) and all(np.array_equal(a, b) for a, b in zip(full[2], hist))
    # a binary guide, the users' whole histories excluded (the reference's use_h), no repeats, a trace
    bits = ((np.arange(N + 1)[:, None] >> np.arange(9)) & 1).astype(np.uint8)
    out = r2i.get_seq_in_batch(hist, tt, _t(bits), guide_k=3, max_path_len=P, exclude=hist, no_repeat=True, exact_candidates=True,
                               trace=True)
    for b in range(B):
        nz = out[0][b][out[0][b] != 0].astype(np.int64)
        assert len(set(nz.tolist())) == len(nz) and not set(nz.tolist()) & (set(hist[b].tolist()) - {int(targets[b])})
    assert r2i.last_trace["lp_item"].shape == (B, P) and (r2i.last_trace["n_steps"] >= 1).all()


def test_irn_front_end_takes_the_guide(golden):
    m = _model("tiny", golden)
    g = golden("irn_tiny")
    net = InfluentialNet(m.cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(m.cfg, 1234).items()})
    net.to(DEV)
    irn = IRSNN(m.cfg, net, DEV)
    seqs, users, targets = _t(g["seqs"]), _t(g["users"]), torch.from_numpy(g["targets"])
    table = m.tables[BINARY]
    want = _host_guided(m, m.P, table, BINARY, 5)[0]
    for b in range(m.B):
        pos = np.where(want[b] == g["targets"][b])[0]
        if len(pos):
            want[b, pos[0] + 1:] = 0
    for stop in (False, True):
        paths, t, hist, n = irn.get_seq_in_batch(seqs, users, targets, m.P, 0, stop_at_target=stop, guide=_t(table), guide_k=5)
        assert np.array_equal(paths, want) and n == sum((p == tg).any() for p, tg in zip(want, g["targets"]))
    plain = irn.get_seq_in_batch(seqs, users, targets, m.P, 0)
    assert np.array_equal(plain[0], g["paths"])


# ============================================================================ 7. refusals on a live context
def test_refusals_change_nothing(golden):
    m = _model("tiny", golden)
    eng, table = m.eng, m.tables[FLOAT]
    before = _greedy(m, guide=_t(table), guide_k=5)
    B, W, P, L = m.B, 2, 3, m.L
    with pytest.raises(IrsError, match=r"error -4\b.*irs_bind_guide.*sample"):
        _greedy(m, guide=_t(table), guide_k=5, sample=True, sample_k=3)
    with pytest.raises(IrsError, match=r"error -1\b.*k=4 < k_c=5"):
        eng.generate_paths(_t(m.seq), m.usr(), _t(m.hep), m.P, k=4, guide=_t(table), guide_k=5)
    with pytest.raises(IrsError, match=r"error -4\b.*32"):
        eng.bind_guide(_t(table), 33)
    with pytest.raises(IrsError, match="n_item \\+ 1"):
        eng.bind_guide(_t(table[:-1]), 5)
    eng.bind_guide(_t(table), 5)
    try:
        st = torch.zeros(B, dtype=torch.int32, device=DEV)
        val, ids = torch.zeros((B, 100), device=DEV), torch.zeros((B, 100), dtype=torch.int64, device=DEV)
        with pytest.raises(IrsError, match=r"error -4\b.*sample"):
            eng.path_step(_t(m.seq), _t(m.hep), val, ids, 0, torch.zeros((B, 4), device=DEV), st, sample=True, sample_k=3)
        with pytest.raises(IrsError, match=r"error -1\b.*k_c=5"):
            eng.path_step(_t(m.seq), _t(m.hep), val[:, :4].contiguous(), ids[:, :4].contiguous(), 0, torch.zeros((B, 4), device=DEV), st)
        with pytest.raises(IrsError, match=r"error -4\b.*irs_beam_search\b.*greedy loops only"):
            eng.beam_search(_t(m.seq), m.usr(), _t(m.hep), P, W)
        with pytest.raises(IrsError, match=r"error -4\b.*irs_beam_search_until.*greedy loops only"):
            eng.beam_search_until(_t(m.seq), m.usr(), _t(m.hep), P, W)

        def state(fin):
            s = (torch.zeros((B, W, L), dtype=torch.int64, device=DEV), torch.zeros((B, W), dtype=torch.int32, device=DEV),
                 torch.zeros((B, W), dtype=torch.float64, device=DEV), torch.zeros((B, W, P), dtype=torch.float32, device=DEV))
            return s + (torch.zeros((B, W), dtype=torch.int32, device=DEV),) if fin else s
        v2, i2 = torch.zeros((B * W, 100), device=DEV), torch.zeros((B * W, 100), dtype=torch.int64, device=DEV)
        lse = (torch.zeros(B * W, device=DEV), torch.ones(B * W, device=DEV))
        with pytest.raises(IrsError, match=r"error -4\b.*irs_beam_step\b.*greedy loops only"):
            eng.beam_step(state(False), v2, i2, lse, 0, state(False), st)
        with pytest.raises(IrsError, match=r"error -4\b.*irs_beam_step_until.*greedy loops only"):
            eng.beam_step_until(state(True), v2, i2, lse, 0, 0, state(True), torch.zeros(B, dtype=torch.int32, device=DEV), st)
        assert not _n(st).any()
    finally:
        torch.cuda.synchronize()
        eng.unbind_guide()
    _same(_greedy(m, guide=_t(table), guide_k=5), before, NAMES4)
    eng.beam_search(_t(m.seq), m.usr(), _t(m.hep), P, W)  # unbound: the beam search runs again
    torch.cuda.synchronize()


def test_a_sharded_context_refuses_the_binding():
    cfg = synth.make_config("tiny")
    eng = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=8, max_seqs=8, rank=0, world=2)
    with pytest.raises(IrsError, match=r"error -4\b.*whole catalog"):
        eng.bind_guide(torch.zeros((cfg.n_item + 1, 4), device=DEV), 5)
    with pytest.raises(IrsError, match=r"error -4\b.*whole catalog"):
        eng.bind_guide(torch.zeros((cfg.n_item + 1, 18), dtype=torch.uint8, device=DEV), 5)
