"""-m gpu: bound exclusions (irs_bind_exclusions; exclude= / no_repeat= in the engine and the front end).

Every comparison is exact: ids, float bits, status words.  The steps and the survivor pass are compared with the restatement
of tests/exclusion_ref.py on synthetic lists.  The four loops are compared with a HOST-STEPPED loop: the engine's own decode,
its own score_topk at k = n_item (the exact ranking) and at k = 100 (what a step sees), then the restatement's survivor pass
and step -- so a loop and its reference score the same rows with the same kernels, and only the search logic is the
restatement's.  The first premise of every loop test is that the host-stepped loop WITHOUT lists reproduces the plain loop: a
route difference between a loop's launches and the stand-alone calls would show up there, not as a feature bug.

The survivor pass alone has no path argument (the header), so "hidden by window + list + path together" is a loop case: in the
loop tests no_repeat is on, a survivor scratch is bound, and the lists hide the users' step-0 top-100."""
import ctypes

import numpy as np
import pytest
import torch

import beam_until_ref
import exclusion_ref as ref
import path_ref
from gpu_util import make_engine, path_only_engine
from influentialrs_amd import synth
from influentialrs_amd._lib import (IRS_BEAM_STOP_ALL, IRS_BEAM_STOP_BEST, IRS_ROW_NO_CANDIDATE, IRS_ROW_RESCUED, IRS_SWEEP_BF16,
                                    IRS_SWEEP_F32)
from influentialrs_amd.engine import IrsError
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NINF = -np.inf


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


class _Bound:
    """A binding for the time of a with-block (the engine's own context manager, named for the tests)."""

    def __init__(self, eng, excl, users, no_repeat):
        self.eng, self.excl, self.users, self.no_repeat = eng, excl, users, no_repeat

    def __enter__(self):
        self.scratch = self.eng.bind_exclusions(None if self.excl is None else _t(self.excl), self.users, self.no_repeat)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.eng.unbind_exclusions()


def _fill_list(g, hide_ids, n_excl, n_item, cand_ids, junk=True):
    """One user's row of n_excl slots: the ids to hide (as many as fit), then -1 holes, duplicates, ids >= n_item and valid ids
    that are no candidates; shuffled."""
    row = [int(i) for i in hide_ids][:n_excl]
    free = np.setdiff1d(np.arange(n_item), cand_ids)
    while len(row) < n_excl:
        kind = int(g.integers(0, 4)) if junk else 0
        if kind == 0 or (kind == 1 and not row):
            row.append(-1)
        elif kind == 1:
            row.append(row[int(g.integers(0, len(row)))])
        elif kind == 2:
            row.append(n_item + int(g.integers(0, 1000)))
        else:
            row.append(int(free[int(g.integers(0, len(free)))]))
    return g.permutation(np.array(row, dtype=np.int64))


# ============================================================================ 1. the path step alone
L1, N1, P1, STEP1 = 128, 5000, 8, 5
_ENG = {}


def _step_engine():
    if "step" not in _ENG:
        _ENG["step"] = path_only_engine(L1, n_item=N1, max_k=128)
    return _ENG["step"]


def _path_case(k, n_excl, seed):
    """Ten rows, candidates from ids0 < 4000, window and path fill from items 4001 .. 4900 (never candidates):
      0 a list of -1 only                                   5 the window holds candidates 1 .. k-1, the list candidate 0: the
      1 the list hides candidate 0                             row's only survivor is hidden by the list -> NO_CANDIDATE
      2 ... candidates 0 .. 63   (as many as fit in n_excl)  6 the candidate list ends at entry 70, the list hides 0 .. 69
      3 ... candidates 0 .. 64                               7 path entry 0 is candidate 0 (no_repeat)
      4 ... candidates 0 .. 98: the survivor is entry 99     8 path entry step-1 is candidate 0 (no_repeat)
      9 path entries 0 and step-1 are candidates 0 and 1, the list hides 2, the window holds 3, path entry step+1 (not yet
        part of the path) is candidate 4: candidate 4 it is"""
    g = np.random.default_rng(seed)
    B = 10
    ids0 = np.stack([g.permutation(4000)[:k] for _ in range(B)]).astype(np.int64)
    val = np.stack([np.sort(g.permutation(4 * k)[:k].astype(np.float32) * 0.125 - 7.0)[::-1] for _ in range(B)])
    seq = g.integers(4001, 4900, size=(B, L1)).astype(np.int64)
    hep = g.choice(np.array([0, 40, L1 - 3, L1 - 2], dtype=np.int32), size=B)
    paths = g.integers(4001, 4900, size=(B, P1)).astype(np.float32)
    paths[:, STEP1:] = 0
    paths[3, 1] = 0  # a hole in a path is no item
    hide = [[] for _ in range(B)]
    hide[1] = ids0[1, :1]
    hide[2] = ids0[2, :64]
    hide[3] = ids0[3, :65]
    hide[4] = ids0[4, :99]
    w = ids0[5, 1:] + 1
    seq[5, :len(w)], hep[5] = w, max(len(w) - 1, 0)
    if len(w) == 0:
        seq[5, 0] = 4001
    hide[5] = ids0[5, :1]
    ids0[6, 70:] = -1
    hide[6] = ids0[6, :70]
    paths[7, 0] = ids0[7, 0] + 1
    paths[8, STEP1 - 1] = ids0[8, 0] + 1
    if k > 4:
        paths[9, 0], paths[9, STEP1 - 1], paths[9, STEP1 + 1] = ids0[9, 0] + 1, ids0[9, 1] + 1, ids0[9, 4] + 1
        hide[9] = ids0[9, 2:3]
        seq[9, 0], hep[9] = ids0[9, 3] + 1, max(hep[9], 0)
    excl = np.stack([_fill_list(g, hide[r], n_excl, N1, ids0[r][ids0[r] >= 0], junk=r != 0) for r in range(B)])
    status = np.array([0, 1, 4, 0, 8, 0, 0, 1, 0, 0], dtype=np.int32)
    return dict(seq=seq, hep=hep, val=val, ids0=ids0, paths=paths, status=status, excl=excl)


def _device_step(eng, c, val, ids0, **kw):
    seq, hep, paths, status = _t(c["seq"]), _t(c["hep"]), _t(c["paths"]), _t(c["status"])
    eng.path_step(seq, hep, _t(val), _t(ids0), STEP1, paths, status, **kw)
    return _n(seq), _n(hep), _n(paths), _n(status)


NAMES4 = ("seq", "hep", "paths", "status")


@pytest.mark.parametrize("no_repeat", [True, False])
@pytest.mark.parametrize("k", [100, 1])
@pytest.mark.parametrize("n_excl", [1, 63, 64, 65, 4096])
def test_path_step_greedy_equals_the_restatement(n_excl, k, no_repeat):
    eng = _step_engine()
    c = _path_case(k, n_excl, seed=1000 * n_excl + k)
    want = ref.path_step(c["seq"], c["hep"], c["val"], c["ids0"], STEP1, c["paths"], c["status"], c["excl"], N1, no_repeat)
    with _Bound(eng, c["excl"], 10, no_repeat):
        got = _device_step(eng, c, c["val"], c["ids0"])
    _same(got, want, NAMES4)
    seq, hep, paths, status = got
    chosen = paths[:, STEP1]
    first = c["ids0"][:, 0] + 1
    # what that means row by row (where the list has room for the row's scenario)
    assert chosen[0] == first[0] and status[5] == IRS_ROW_NO_CANDIDATE and chosen[5] == 0
    assert np.array_equal(seq[5], c["seq"][5]) and hep[5] == c["hep"][5] and np.array_equal(paths[5, :STEP1], c["paths"][5, :STEP1])
    assert status[1] & 1 and status[4] & 8 and status[2] & 4, "bits that are there already stay"
    if k == 100:
        assert chosen[1] == c["ids0"][1, 1] + 1
        if n_excl >= 65:
            assert chosen[2] == c["ids0"][2, 64] + 1 and chosen[3] == c["ids0"][3, 65] + 1
        if n_excl == 64:
            assert chosen[2] == c["ids0"][2, 64] + 1 and chosen[3] == c["ids0"][3, 64] + 1
        if n_excl == 4096:
            assert chosen[4] == c["ids0"][4, 99] + 1 and status[6] == IRS_ROW_NO_CANDIDATE and chosen[6] == 0
        assert chosen[7] == c["ids0"][7, 1 if no_repeat else 0] + 1 and chosen[8] == c["ids0"][8, 1 if no_repeat else 0] + 1
        assert chosen[9] == c["ids0"][9, 4 if no_repeat else 0] + 1
    else:
        assert (status[7] & IRS_ROW_NO_CANDIDATE != 0) == no_repeat and (status[8] & IRS_ROW_NO_CANDIDATE != 0) == no_repeat


@pytest.mark.parametrize("n_excl", [1, 65, 4096])
def test_path_step_sampled_draws_among_the_first_admissible(n_excl):
    """sample_k = 3.  The draw itself is the unbound kernel's: the bound step on the row's list equals, bit for bit, the unbound
    step (same seed, row and step) on the list with the hidden entries struck -- the same three survivors with the same scores."""
    eng = _step_engine()
    c = _path_case(100, n_excl, seed=77 + n_excl)
    dists = ref.path_step(c["seq"], c["hep"], c["val"], c["ids0"], STEP1, c["paths"], c["status"], c["excl"], N1, True, sample=True,
                          sample_k=3)
    struck = [ref.strike(c["val"][r], c["ids0"][r], ref.hidden(c["excl"][r], N1, c["paths"][r], STEP1, True)) for r in range(10)]
    kw = dict(sample=True, sample_k=3, seed=20261019)
    plain = _device_step(eng, c, np.stack([s[0] for s in struck]), np.stack([s[1] for s in struck]), **kw)
    with _Bound(eng, c["excl"], 10, True):
        got = _device_step(eng, c, c["val"], c["ids0"], **kw)
    _same(got, plain, NAMES4)
    for r, (items, prob) in enumerate(dists):
        if len(items) == 0:
            assert got[3][r] & IRS_ROW_NO_CANDIDATE and got[2][r, STEP1] == 0
        else:
            assert int(got[2][r, STEP1]) in items.tolist() and not (got[3][r] & IRS_ROW_NO_CANDIDATE)
    assert [len(d[0]) for d in dists][5] == 0 and len(dists[9][0]) == 3 and dists[9][0][0] == c["ids0"][9, 4] + 1


# ============================================================================ 2. the beam steps alone
W2, K2, STEP2, P2, NX2 = 4, 100, 3, 8, 65


def _beam_case(until, seed):
    """Four users, W = 4.  Window items come from 6001 .., so a candidate is hidden only on purpose.
      0 beam 0's path holds its candidates 0 (entry 0) and 1 (entry step-1); the user's ONE list hides beam 0's candidate 2 and
        beam 1's candidates 0 and 1, and beam 2's window its candidate 0
      1 a dead beam, and a list of -1 only
      2 until: beam 1 is finished and its lists are garbage (NaN scores, ids far outside any catalog)
      3 until: done on entry"""
    g = np.random.default_rng(seed)
    B, W, k, P, step = 4, W2, K2, P2, STEP2
    seq = g.integers(6001, 9000, size=(B, W, L1)).astype(np.int64)
    hep = g.choice(np.array([0, 50, L1 - 3, L1 - 2], dtype=np.int32), size=(B, W))
    cum = -(g.integers(0, 80, size=(B, W)).astype(np.float64) * 0.125)
    paths = g.integers(4001, 4900, size=(B, W, P)).astype(np.float32)
    paths[:, :, step:] = 0
    fin = np.zeros((B, W), dtype=np.int32)
    done = np.zeros(B, dtype=np.int32)
    ids0 = np.stack([g.permutation(4000)[:k] for _ in range(B * W)]).astype(np.int64)
    val = np.stack([np.sort(g.permutation(4 * k)[:k].astype(np.float32) * 0.125 - 7.0)[::-1] for _ in range(B * W)])
    lmax = (g.integers(0, 64, size=B * W).astype(np.float64) * 0.125).astype(np.float32)
    lsum = np.ones(B * W, dtype=np.float32)
    paths[0, 0, 0], paths[0, 0, step - 1] = ids0[0, 0] + 1, ids0[0, 1] + 1
    seq[0, 2, 0] = ids0[2, 0] + 1
    cum[0] = [0.0, 0.0, -0.125, -1000.0]  # beams 0, 1 and 2 of user 0 score alike, so all three place children
    val[1], val[2], lmax[:3] = val[0], val[0], 0.0
    hide = [np.concatenate([ids0[0, 2:3], ids0[1, :2]]), [], ids0[2 * W, :3], ids0[3 * W, :1]]
    cum[1, 2] = NINF
    seq[2, :, L1 - 1] = ids0[2 * W, 3] + 1  # beam 0 of user 2 takes its target (its candidates 0 .. 2 are in the list)
    cum[2] = [0.0, 1000.0, -1000.0, -1000.0]  # ... and its children are the user's best, behind beam 1 (finished in the until case)
    if until:
        fin[2, 1] = 1
        row = 2 * W + 1
        val[row], ids0[row], lmax[row], lsum[row] = np.nan, 1 << 40, np.nan, np.nan
        paths[2, 1] = 7000 + np.arange(P)
        done[3] = 1
    excl = np.stack([_fill_list(g, hide[b], NX2, N1, ids0[b * W:(b + 1) * W].reshape(-1), junk=b != 1) for b in range(B)])
    status = np.array([0, 4, 1, 0], dtype=np.int32)
    return dict(state=(seq, hep, cum, paths, fin), done=done, val=val, ids0=ids0, lse=(lmax, lsum), status=status, excl=excl)


KINDS5 = (torch.int64, torch.int32, torch.float64, torch.float32, torch.int32)
NAMES5 = ("seq", "hep", "cum", "paths", "fin")


@pytest.mark.parametrize("no_repeat", [True, False])
def test_beam_step_equals_the_restatement(no_repeat):
    eng = _step_engine()
    c = _beam_case(False, seed=5)
    st4 = c["state"][:4]
    want, w_st = ref.beam_step(st4, c["val"], c["ids0"], *c["lse"], STEP2, P2, c["excl"], N1, no_repeat, c["status"])
    other, _ = ref.beam_step(st4, c["val"], c["ids0"], *c["lse"], STEP2, P2, c["excl"], N1, not no_repeat, c["status"])
    unbound, _ = path_ref.beam_step(st4, c["val"], c["ids0"], *c["lse"], STEP2, P2, c["status"])
    assert not np.array_equal(want[3][0], other[3][0]), "the parent's path decides at user 0"
    assert not np.array_equal(want[3][0], unbound[3][0]) and np.array_equal(want[3][1], unbound[3][1]), "user 1's list is empty"
    outs = tuple(torch.zeros(a.shape, dtype=kd, device=DEV) for a, kd in zip(st4, KINDS5))
    status = _t(c["status"])
    with _Bound(eng, c["excl"], 4, no_repeat):
        eng.beam_step(tuple(_t(a) for a in st4), _t(c["val"]), _t(c["ids0"]), tuple(_t(a) for a in c["lse"]), STEP2, outs, status)
    _same([_n(o) for o in outs], want, NAMES5[:4])
    assert np.array_equal(_n(status), w_st)
    if no_repeat:  # beams of one user share the list: beam 1's candidates 0 and 1 are gone with beam 0's candidate 2
        new = set(_n(outs[3])[0, :, STEP2].astype(np.int64).tolist())
        assert not new & {int(c["ids0"][0, 0]) + 1, int(c["ids0"][0, 1]) + 1, int(c["ids0"][0, 2]) + 1}
        assert not new & {int(c["ids0"][1, 0]) + 1, int(c["ids0"][1, 1]) + 1, int(c["ids0"][2, 0]) + 1}


@pytest.mark.parametrize("rule", [IRS_BEAM_STOP_ALL, IRS_BEAM_STOP_BEST])
@pytest.mark.parametrize("no_repeat", [True, False])
def test_beam_step_until_equals_the_restatement(no_repeat, rule):
    eng = _step_engine()
    c = _beam_case(True, seed=6)
    want, w_done, w_st = ref.beam_step_until(c["state"], c["done"], c["val"], c["ids0"], *c["lse"], STEP2, P2, rule, c["excl"], N1,
                                             no_repeat, c["status"])
    assert want[4][2].tolist() == [1, 1, 0, 0], "user 2: the finished beam stays, whole, and beam 0's first child takes the target"
    assert np.array_equal(want[3][2, 0], c["state"][3][2, 1]) and want[3][2, 1, STEP2] == c["ids0"][2 * W2, 3] + 1
    outs = tuple(torch.zeros(a.shape, dtype=kd, device=DEV) for a, kd in zip(c["state"], KINDS5))
    status, done = _t(c["status"]), _t(c["done"])
    with _Bound(eng, c["excl"], 4, no_repeat):
        eng.beam_step_until(tuple(_t(a) for a in c["state"]), _t(c["val"]), _t(c["ids0"]), tuple(_t(a) for a in c["lse"]), STEP2, rule,
                            outs, done, status)
    _same([_n(o) for o in outs], want, NAMES5)
    assert np.array_equal(_n(done), w_done) and np.array_equal(_n(status), w_st)
    assert np.array_equal(_n(outs[3])[3], c["state"][3][3]), "a done user is copied through"


# ============================================================================ 3. the survivor pass with a binding
K3 = 100


@pytest.fixture(scope="module", params=[32, 30])
def bound_rows(request, oracle):
    """n_item = 300, k = 100, L = 128, eight rows of four users (rows_per_status = 2: rows 2u and 2u + 1 read user u's list):
      0 (user 0) the list holds the row's top 120 items, the window none of them      starved by the list alone
      1 (user 0) another row under the same list                                        whatever the restatement says
      2 (user 1) the window holds ranks 0 .. 59, the list ranks 60 .. 124              starved by window + list together
      3 (user 1) a random window
      4, 5 (user 2) the list holds ranks 200 .. 259 of row 4                            row 4 is not starved
      6 (user 3) the window holds the top 120, the list is -1 only                      starved by the window alone
      7 (user 3) finished (fin = 1): skipped"""
    d = request.param
    n_item, M = 300, 8
    g = np.random.default_rng(70 + d)
    Wt = ((g.random((n_item, d), dtype=np.float32) * 2 - 1) / np.sqrt(d)).astype(np.float32)
    b = (g.standard_normal(n_item) * 0.1).astype(np.float32)
    x = g.standard_normal((M, d)).astype(np.float32)
    rank = [oracle.topk(oracle.score_chain(x[m], Wt, b), n_item) for m in range(M)]
    seq = np.zeros((M, L1), dtype=np.int64)
    hep = np.zeros(M, dtype=np.int32)

    def window(m, items):
        seq[m, :len(items)], hep[m] = items, len(items) - 1

    window(0, rank[0][1][150:190] + 1)
    window(1, rank[1][1][10:40] + 1)
    window(2, rank[2][1][:60] + 1)
    window(3, g.permutation(n_item)[:50] + 1)
    window(4, rank[4][1][5:30] + 1)
    window(5, rank[5][1][:3] + 1)
    window(6, rank[6][1][:120] + 1)
    window(7, rank[7][1][:120] + 1)
    seq[:, L1 - 1] = 1 + np.array([r[1][140] for r in rank])
    nx = 130
    none = np.zeros(0, dtype=np.int64)
    excl = np.stack([_fill_list(g, rank[0][1][:120], nx, n_item, none), _fill_list(g, rank[2][1][60:125], nx, n_item, none),
                     _fill_list(g, rank[4][1][200:260], nx, n_item, none), _fill_list(g, [], nx, n_item, none, junk=False)])
    nh = d // 32 if d % 32 == 0 else 1
    cfg = synth.make_config("tiny", n_item=n_item, emb_dim=d, n_heads=nh, n_layers=1, max_len=L1, ffn_dim=8, n_user=2)
    sd = synth.irn_state_dict(cfg, seed=1)
    sd["project.weight"], sd["project.bias"] = Wt, b
    eng = make_engine(cfg, sd, max_rows=M, max_seqs=1, max_k=K3)
    val, ids, _ = eng.score_topk(_t(x), K3, IRS_SWEEP_F32)
    val, ids = _n(val), _n(ids)
    for m in range(M):
        assert np.array_equal(ids[m], rank[m][1][:K3]) and val[m].tobytes() == rank[m][0][:K3].tobytes()
    fin = np.array([0] * 7 + [1], dtype=np.int32)
    return dict(eng=eng, x=x, seq=seq, hep=hep, val=val, ids=ids, rank=rank, excl=excl, fin=fin, n_item=n_item)


@pytest.mark.parametrize("want", [1, 4])
def test_survivor_pass_with_a_binding_equals_the_restatement(bound_rows, want):
    c = bound_rows
    rank = c["rank"]
    status = np.array([0, 4, 0, 1], dtype=np.int32)
    e_val, e_ids, e_st, starved = ref.ensure_survivors(c["seq"], c["hep"], c["val"], c["ids"], status, want, lambda m: rank[m], c["excl"],
                                                       c["n_item"], rows_per_status=2, fin=c["fin"])
    assert {0, 2, 6} <= set(starved) and 4 not in starved and 7 not in starved
    plain = ref.ensure_survivors(c["seq"], c["hep"], c["val"], c["ids"], status, want, lambda m: rank[m], None, c["n_item"],
                                 rows_per_status=2, fin=c["fin"])
    assert plain[3] == [6], "without the lists only the window of row 6 starves anybody"
    eng = c["eng"]
    v, i, s = _t(c["val"]), _t(c["ids"]), _t(status)
    with _Bound(eng, c["excl"], 4, False):
        eng.ensure_survivors(_t(c["x"]), _t(c["seq"]), _t(c["hep"]), v, i, s, want=want, rows_per_status=2, fin=_t(c["fin"]))
        got = (_n(v), _n(i), _n(s))
    _same(got, (e_val, e_ids, e_st), ("val", "ids0", "status"))
    assert got[1][0, 0] == rank[0][1][120] and got[0][0, 0].tobytes() == rank[0][0][120].tobytes()
    assert got[1][2, 0] == rank[2][1][125], "the first rank outside window (0 .. 59) and list (60 .. 124)"
    assert got[1][6, 0] == rank[6][1][120]
    # unbound again: the pass is the parent's
    v, i, s = _t(c["val"]), _t(c["ids"]), _t(status)
    eng.ensure_survivors(_t(c["x"]), _t(c["seq"]), _t(c["hep"]), v, i, s, want=want, rows_per_status=2, fin=_t(c["fin"]))
    _same((_n(v), _n(i), _n(s)), plain[:3], ("val", "ids0", "status"))


# ============================================================================ 4 - 6. the loops against the host-stepped loop
class _Model:
    """An engine with its inputs, and the stand-alone calls the host-stepped loops are made of."""

    def __init__(self, cfg, sd, seq, users, rows):
        self.cfg, self.n_item, self.L = cfg, cfg.n_item, cfg.max_len
        self.eng = make_engine(cfg, sd, max_rows=rows, max_seqs=rows, max_k=cfg.n_item)
        self.seq, self.users = np.asarray(seq, dtype=np.int64), np.asarray(users, dtype=np.int64)
        self.B = len(self.seq)
        self.hep = np.full(self.B, self.L - 2, dtype=np.int32)

    def lists(self, seq, users, hep, lse=False):
        """(full val, full ids0[, norm float64]) of the rows: the exact ranking; its first 100 entries are the step's list."""
        _, xr, _ = self.eng.decode(_t(seq), _t(users), want_x=False, pos=_t(hep))
        fv, fi, _ = self.eng.score_topk(xr, self.n_item, IRS_SWEEP_BF16)
        if not lse:
            return _n(fv), _n(fi)
        v, i, _, mx, sm = self.eng.score_topk_lse(xr, 100, IRS_SWEEP_BF16)
        assert np.array_equal(_n(i), _n(fi)[:, :100]) and np.array_equal(_bits(_n(v)), _bits(_n(fv)[:, :100]))
        norm = mx.double() + torch.log(sm.double())  # (the device's own log: the beam step's arithmetic)
        return _n(fv), _n(fi), _n(norm)

    def step0_top100(self):
        return self.lists(self.seq, self.users, self.hep)[1][:, :100].copy()


def _host_greedy(m, P, excl, no_repeat, exact, until=False):
    """(paths, seq, hep, status) of the greedy search, stepped on the host.  until: a user is frozen after the step that chose its
    target, its tail zero (the tail of the plain search goes on)."""
    seq, hep = m.seq.copy(), m.hep.copy()
    paths, status = np.zeros((m.B, P), dtype=np.float32), np.zeros(m.B, dtype=np.int32)
    fin = np.zeros(m.B, dtype=np.int32)
    bound = excl is not None or no_repeat
    for step in range(P):
        if until and fin.all():
            break
        fv, fi = m.lists(seq, m.users, hep)
        val, ids = fv[:, :100].copy(), fi[:, :100].copy()
        if exact:
            val, ids, st2, _ = ref.ensure_survivors(seq, hep, val, ids, status, 1, lambda r: (fv[r], fi[r]), excl, m.n_item, fin=fin,
                                                    paths=paths, step=step, no_repeat=no_repeat)
        else:
            st2 = status
        if bound:
            s2, h2, p2, st2 = ref.path_step(seq, hep, val, ids, step, paths, st2, excl, m.n_item, no_repeat)
        else:
            s2, h2, p2, st2 = path_ref.path_step(seq, hep, val, ids, step, paths, st2)
        live = fin == 0
        seq[live], hep[live], paths[live], status[live] = s2[live], h2[live], p2[live], st2[live]
        if until:
            fin |= (live & (paths[:, step] == seq[:, m.L - 1])).astype(np.int32)
    return paths, seq, hep, status


def _host_beam(m, P, W, excl, no_repeat, exact, rule=None):
    """(paths [B, W, P], scores [B, W], status [B], final windows, fin [B, W]) of the beam search, stepped on the host.
    rule None: irs_beam_search; else the until form (a done user is copied through by the step itself)."""
    B, L = m.B, m.L
    seq = np.repeat(m.seq[:, None], W, axis=1)
    hep = np.repeat(m.hep[:, None], W, axis=1)
    cum = np.full((B, W), NINF)
    cum[:, 0] = 0.0
    paths = np.zeros((B, W, P), dtype=np.float32)
    fin, done, status = np.zeros((B, W), dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    users = np.repeat(m.users, W)
    ones = np.ones(B * W)
    bound = excl is not None or no_repeat
    for step in range(P):
        if rule is not None and done.all():
            break
        fv, fi, norm = m.lists(seq.reshape(B * W, L), users, hep.reshape(-1), lse=True)
        val, ids = fv[:, :100].copy(), fi[:, :100].copy()
        if exact:
            val, ids, status, _ = ref.ensure_survivors(seq.reshape(B * W, L), hep.reshape(-1), val, ids, status, W,
                                                       lambda r: (fv[r], fi[r]), excl, m.n_item, rows_per_status=W, cum=cum.reshape(-1),
                                                       fin=fin.reshape(-1) if rule is not None else None,
                                                       done=done if rule is not None else None, paths=paths.reshape(B * W, P), step=step,
                                                       no_repeat=no_repeat)
        # norm + log(1) is norm: the restatements take (max, sumexp)
        if rule is None:
            if bound:
                (seq, hep, cum, paths), status = ref.beam_step((seq, hep, cum, paths), val, ids, norm, ones, step, P, excl, m.n_item,
                                                               no_repeat, status)
            else:
                (seq, hep, cum, paths), status = path_ref.beam_step((seq, hep, cum, paths), val, ids, norm, ones, step, P, status)
        elif bound:
            (seq, hep, cum, paths, fin), done, status = ref.beam_step_until((seq, hep, cum, paths, fin), done, val, ids, norm, ones, step,
                                                                            P, rule, excl, m.n_item, no_repeat, status)
        else:
            (seq, hep, cum, paths, fin), done, status = beam_until_ref.beam_step_until((seq, hep, cum, paths, fin), done, val, ids, norm,
                                                                                       ones, step, P, rule, status)
    return paths, cum, status, seq, fin


USERS_TINY = [0, 4, 7, 8, 2, 10]  # of the tiny goldens: the unbound search of 4, 7 and 8 repeats an item; 2 and 10 arrive early


_MODELS = {}


def _model(name, golden):
    """tiny: the golden shape (N = 257, d = 16, L = 12, two layers), P = 20: path items slide out of the window.
    L104: n_item = 300, L = 104 (a window of more than one 64-lane round), P = 6."""
    if name in _MODELS:
        return _MODELS[name]
    if name == "tiny":
        g = golden("irn_tiny")
        cfg = synth.make_config("tiny")
        m = _Model(cfg, synth.irn_state_dict(cfg, 1234), g["seqs"][USERS_TINY], g["users"][USERS_TINY], 32)
        m.P = 20
    else:
        cfg = synth.make_config("tiny", n_item=300, max_len=104)
        rg = np.random.default_rng(104)
        seq = np.zeros((3, 104), dtype=np.int64)
        seq[0, 3:103] = rg.permutation(300)[:100] + 1
        seq[1, 80:103] = rg.permutation(300)[:23] + 1
        seq[2, 1:103] = rg.permutation(300)[:102] + 1
        seq[:, 103] = [299, 7, 150]
        m = _Model(cfg, synth.irn_state_dict(cfg, 1234), seq, np.array([3, 11, 5]), 16)
        m.P = 6
    m.name = name
    m.excl = m.step0_top100()  # every user's own step-0 top-100: unbound k = 100 plus this list starves the user for certain
    _MODELS[name] = m
    return m


@pytest.fixture(scope="module", params=["tiny", "L104"])
def model(request, golden):
    return _model(request.param, golden)


def _greedy(m, use_graph=False, **kw):
    seq, hep = _t(m.seq), _t(m.hep)
    paths, status = m.eng.generate_paths(seq, _t(m.users), hep, m.P, k=100, sweep=IRS_SWEEP_BF16, use_graph=use_graph, **kw)
    return _n(paths), _n(seq), _n(hep), _n(status)


def _assert_no_repeat(paths, excl):
    for b in range(len(paths)):
        nz = paths[b][paths[b] != 0].astype(np.int64)
        assert len(set(nz.tolist())) == len(nz), (b, paths[b])
        assert not set((nz - 1).tolist()) & set(excl[b].tolist()), (b, paths[b])


@pytest.mark.parametrize("use_graph", [False, True])
def test_generate_paths_equals_the_host_stepped_loop(model, use_graph):
    m = model
    plain = _greedy(m, use_graph)
    _same(plain, _host_greedy(m, m.P, None, False, False), NAMES4)  # premise 1: the reference walks the plain loop
    if m.name == "tiny":  # premise 2: the unbound search offers an item twice
        assert any(len(set(p[p != 0].tolist())) < (p != 0).sum() for p in plain[0])
    ex = _t(m.excl)
    starved = _greedy(m, use_graph, exclude=ex)  # premise 3: the list alone starves every user at step 0
    assert (starved[3] & IRS_ROW_NO_CANDIDATE).all() and (starved[0][:, 0] == 0).all()
    _same(starved, _host_greedy(m, m.P, m.excl, False, False), NAMES4)
    got = _greedy(m, use_graph, exclude=ex, no_repeat=True, exact_candidates=True)
    want = _host_greedy(m, m.P, m.excl, True, True)
    _same(got, want, NAMES4)
    assert (got[3] & IRS_ROW_RESCUED).all()
    _assert_no_repeat(got[0], m.excl)
    if m.name == "tiny":
        assert (got[0] != 0).all() and not (got[3] & IRS_ROW_NO_CANDIDATE).any()
    again = _greedy(m, use_graph)  # unbound again
    _same(again, plain, NAMES4)


@pytest.mark.parametrize("check_every", [1, 3])
def test_generate_paths_until_keeps_every_users_list_through_the_compactions(model, check_every):
    """A different list per user: the step-0 top-100 without the user's target, so the starved users still see their target among
    the exact candidates and finish at different steps; the rows behind a finished user move up, and read their own lists and
    their own rows of the caller's paths through the map."""
    m = model
    excl = m.excl.copy()
    excl[excl == (m.seq[:, -1] - 1)[:, None]] = -1

    def run(**kw):
        paths, status, steps, row_steps = m.eng.generate_paths_until(_t(m.seq), _t(m.users), _t(m.hep), m.P, k=100, sweep=IRS_SWEEP_BF16,
                                                                    check_every=check_every, **kw)
        return _n(paths), _n(status), steps, row_steps

    plain = run()
    h = _host_greedy(m, m.P, None, False, False, until=True)
    _same(plain[:2], (h[0], h[3]), ("paths", "status"))
    got = run(exclude=_t(excl), no_repeat=True, exact_candidates=True)
    w = _host_greedy(m, m.P, excl, True, True, until=True)
    _same(got[:2], (w[0], w[3]), ("paths", "status"))
    _assert_no_repeat(got[0], excl)
    arrived = [int(np.where(p == t)[0][0]) if (p == t).any() else None for p, t in zip(w[0], m.seq[:, -1])]
    if m.name == "tiny":
        assert len({a for a in arrived if a is not None}) >= 2 and None in arrived, arrived
        assert got[3] < m.B * m.P, "finished users were retired"
    _same(run()[:2], plain[:2], ("paths", "status"))


def _beams(m, W, use_graph=False, **kw):
    out = m.eng.beam_search(_t(m.seq), _t(m.users), _t(m.hep), m.P, W, k=100, sweep=IRS_SWEEP_BF16, use_graph=use_graph,
                            want_windows=True, **kw)
    return [_n(t) for t in out]


NAMESB = ("paths", "scores", "status", "windows")


def test_beam_search_equals_the_host_stepped_loop(model):
    m, W = model, 4
    plain = _beams(m, W)
    _same(plain, _host_beam(m, m.P, W, None, False, False)[:4], NAMESB)
    got = _beams(m, W, exclude=_t(m.excl), no_repeat=True, exact_candidates=True)
    want = _host_beam(m, m.P, W, m.excl, True, True)
    _same(got, want[:4], NAMESB)
    assert (got[2] & IRS_ROW_RESCUED).all()
    for j in range(W):
        _assert_no_repeat(got[0][:, j], m.excl)
    _same(_beams(m, W), plain, NAMESB)


@pytest.mark.parametrize("rule", [IRS_BEAM_STOP_ALL, IRS_BEAM_STOP_BEST])
def test_beam_search_until_equals_the_host_stepped_loop(model, rule):
    m, W = model, 4
    excl = m.excl.copy()
    excl[excl == (m.seq[:, -1] - 1)[:, None]] = -1

    def run(**kw):
        out = m.eng.beam_search_until(_t(m.seq), _t(m.users), _t(m.hep), m.P, W, k=100, sweep=IRS_SWEEP_BF16, stop_rule=rule,
                                      check_every=1, **kw)
        return [_n(t) for t in out[:4]]

    names = ("paths", "scores", "status", "fin")
    plain = run()
    h = _host_beam(m, m.P, W, None, False, False, rule)
    _same(plain, (h[0], h[1], h[2], h[4]), names)
    got = run(exclude=_t(excl), no_repeat=True, exact_candidates=True)
    w = _host_beam(m, m.P, W, excl, True, True, rule)
    _same(got, (w[0], w[1], w[2], w[4]), names)
    for j in range(W):
        _assert_no_repeat(got[0][:, j], excl)
    _same(run(), plain, names)


# ============================================================================ 6. unbound is the parent; captured steps
def test_unbound_outputs_are_byte_identical_and_a_captured_step_is_not_replayed(model):
    m = model
    eng = m.eng
    seq, hep, users = _t(m.seq), _t(m.hep), _t(m.users)
    paths = torch.zeros((m.B, m.P), dtype=torch.float32, device=DEV)
    status = torch.zeros(m.B, dtype=torch.int32, device=DEV)

    def run():  # the same buffers every time: a captured step's key stays the same
        seq.copy_(_t(m.seq))
        hep.copy_(_t(m.hep))
        paths.fill_(-3.0)
        eng.generate_paths(seq, users, hep, m.P, k=100, sweep=IRS_SWEEP_BF16, use_graph=True, paths=paths, status=status)
        return _n(paths).copy(), _n(seq).copy(), _n(hep).copy(), _n(status).copy()

    before = run()
    with _Bound(eng, m.excl, m.B, False):
        during = run()
    after = run()
    _same(after, before, NAMES4)
    assert (during[3] & IRS_ROW_NO_CANDIDATE).all() and (during[0][:, 0] == 0).all(), "the step captured before the bind was not replayed"
    assert (before[0][:, 0] != 0).all()


# ============================================================================ 7. refusals before any launch
def test_refusals_before_any_launch(model):
    m = model
    eng = m.eng
    ex = _t(m.excl)
    with pytest.raises(IrsError, match=r"error -4\b.*4096"):
        eng.bind_exclusions(torch.full((m.B, 4097), -1, dtype=torch.int64, device=DEV), scratch=torch.zeros(1 << 20, dtype=torch.uint8,
                                                                                                         device=DEV))
    with pytest.raises(IrsError, match=r"error -1\b.*too small"):
        eng.bind_exclusions(ex, scratch=torch.zeros(64, dtype=torch.uint8, device=DEV))
    big = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(IrsError, match=r"error -1\b.*aligned"):
        eng.bind_exclusions(ex, scratch=big[8:])
    plain = _greedy(m)
    eng.bind_exclusions(ex[:2].contiguous())  # two users bound
    try:
        with pytest.raises(IrsError, match=r"error -1\b.*bound for 2"):
            _greedy(m)
        st = torch.zeros(m.B, dtype=torch.int32, device=DEV)
        val, ids = torch.zeros((m.B, 100), device=DEV), torch.zeros((m.B, 100), dtype=torch.int64, device=DEV)
        with pytest.raises(IrsError, match=r"error -1\b.*bound for 2"):
            eng.path_step(_t(m.seq), _t(m.hep), val, ids, 0, torch.zeros((m.B, 4), device=DEV), st)
        with pytest.raises(IrsError, match=r"error -1\b.*bound for 2"):
            eng.beam_search(_t(m.seq), _t(m.users), _t(m.hep), 3, 4)
    finally:
        eng.unbind_exclusions()
    _same(_greedy(m), plain, NAMES4)


def test_a_sharded_context_refuses_the_binding():
    cfg = synth.make_config("tiny")
    eng = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=8, max_seqs=8, rank=0, world=2)
    with pytest.raises(IrsError, match=r"error -4\b.*whole catalog"):
        eng.bind_exclusions(torch.full((2, 4), -1, dtype=torch.int64, device=DEV))
    with pytest.raises(IrsError, match=r"error -4\b.*whole catalog"):
        eng.bind_exclusions(None, 2, no_repeat=True)


# ============================================================================ 8. front end and harness
def _handler(m):
    net = InfluentialNet(m.cfg)
    sd = synth.irn_state_dict(m.cfg, 1234)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.to(DEV)
    irn = IRSNN(m.cfg, net, DEV)
    irn.eval()
    return irn


def test_front_end_tuple_and_the_sharded_refusal(golden):
    m = _model("tiny", golden)
    g = golden("irn_tiny")
    raw = [g["raw"][u][g["raw"][u] != 0] for u in USERS_TINY]
    irn = _handler(m)
    seq, usr, tgt = _t(m.seq), _t(m.users), _t(m.seq[:, -1].copy())
    with torch.no_grad():
        paths, tt, hh, early = irn.get_seq_in_batch(seq, usr, tgt, m.P, 0, False, 3, exclude=raw, no_repeat=True, exact_candidates=True)
        padded = np.zeros((m.B, max(len(r) for r in raw)), dtype=np.int64)
        for b, r in enumerate(raw):
            padded[b, :len(r)] = r
        again = irn.get_seq_in_batch(seq, usr, tgt, m.P, 0, False, 3, exclude=_t(padded), no_repeat=True, exact_candidates=True)
    # the engine call it stands for: the raw history and the initial window as the list
    excl = np.full((m.B, padded.shape[1] + m.L - 1), -1, dtype=np.int64)
    excl[:, :padded.shape[1]] = padded - 1
    excl[:, padded.shape[1]:] = m.seq[:, :m.L - 1] - 1
    want = _host_greedy(m, m.P, excl, True, True)[0]
    for b in range(m.B):
        hit = np.where(want[b] == m.seq[b, -1])[0]
        if len(hit):
            want[b, hit[0] + 1:] = 0
    assert paths.dtype == np.float32 and np.array_equal(paths, want) and np.array_equal(again[0], paths)
    assert np.array_equal(tt, m.seq[:, -1]) and len(hh) == m.B and early == int(sum((want[b] == m.seq[b, -1]).any() for b in range(m.B)))
    for b in range(m.B):
        nz = paths[b][paths[b] != 0].astype(np.int64)
        assert len(set(nz.tolist())) == len(nz) and not set(nz.tolist()) & set(raw[b].tolist())
        assert not set(nz.tolist()) & set(m.seq[b, :m.L - 1].tolist())
    assert irn._exclude is None and irn._no_repeat is False
    net = InfluentialNet(m.cfg)
    net.shard_items(0, 2, drop_full=False)
    with pytest.raises(ValueError, match="exclude / no_repeat is not built for an item-sharded catalog"):
        IRSNN(m.cfg, net, "cpu").get_seq_in_batch(seq.cpu(), usr.cpu(), tgt.cpu(), 5, 0, exclude=raw)


def test_harness_passes_the_history_through(golden):
    m = _model("tiny", golden)
    from influentialrs_amd import harness
    cfg = synth.make_config("tiny")
    for k, v in dict(gap_len=0, batch_size=4, top_k=5, use_h=True, max_path_len=6, sample=False, sample_k=3).items():
        setattr(cfg, k, v)
    hists = synth.user_histories(8, cfg.n_item, seed=7)
    rows = synth.eval_rows(hists, cfg.n_item, seed=11)[:4]
    irn = _handler(m)
    cfg.exclude_history, cfg.no_repeat, cfg.exact_candidates = True, True, True
    out = harness.test_model(cfg, rows, irn, DEV, verbose=False)
    raws = synth.collate_eval_irs(rows, cfg.max_len, gap_len=0)[0]
    for b, p in enumerate(out["paths"]):
        nz = p[p != 0].astype(np.int64)
        raw = np.asarray(raws[b])
        assert len(nz) and len(set(nz.tolist())) == len(nz) and not set(nz.tolist()) & set(raw[raw != 0].tolist()), (b, p, raw)
    cfg.exclude_history, cfg.no_repeat = False, False
    base = harness.test_model(cfg, rows, irn, DEV, verbose=False)
    assert base["paths"].shape == out["paths"].shape
