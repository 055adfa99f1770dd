"""-m gpu: every mode of the float32 catalog sweep (k_sweep_f32, k_lse_f32, k_lse_ring: dense logits, gather, count-before,
log-sum-exp, cross entropy forward and gradient, the path trace's sweep) at every row-block geometry of its launchers, against
references that share no code with the kernels.  tests/sweep_mode_cases.py is the table ((n_item, d, M) and the restated launch
geometry); tests/test_sweep_mode_cases.py proves on the CPU that the table reaches every cell.

References, per case, computed once and shared by the modes (the `case` fixture is module-scoped: pytest runs all modes of one case,
then frees it):
  S[m]   = oracle.score_chain(x[m], W, b): the float32 fixed-order chain that include/irs_hip.h promises bit for bit;
  S64    = the same product in float64 numpy.
Bars.  Bitwise wherever the header promises the chain (dense, gather, label scores) and on every integer (counts, ranks).
Log-sum-exp: the project's bar, 4e-6 * max(1, |lse|), per row against logsumexp(S64[m]).  CE gradient: 4 x the error of the same
formula in float32 numpy (from S and the float32 lse the kernel is given) against the float64 one, floor 2e-6 * scale -- the
calibration of tests/test_gpu_train_trunk.py (the kernel's exp and rounding order differ from numpy's); both errors per case go to
sweep_mode_errors.json beside the parity record.
Every entry point is called twice with identical inputs and must return identical bits: scratch, counters or partial slots left
dirty by the first call would show in the second."""
import json
import os

import numpy as np
import pytest
import torch

import sweep_mode_cases as C
import test_gpu_path_trace as PT
from gpu_util import scoring_only_engine
from parity_record import OUT as PARITY_OUT

pytestmark = pytest.mark.gpu

OUT = os.path.join(os.path.dirname(PARITY_OUT), "sweep_mode_errors.json")
SENT = np.float32(-12345.5)  # what the padding of a wider output buffer is filled with
N_IDS = 9                    # gathered ids per row
N_EXCL = 8                   # exclusion slots per row
LSE_BAR = 4e-6               # x max(1, |lse|): tests/test_gpu_scoring.py


def _weights(n_item, d, seed):
    g = np.random.default_rng(seed)
    W = ((g.random((n_item, d), dtype=np.float32) * 2 - 1) / np.sqrt(d)).astype(np.float32)
    b = (g.standard_normal(n_item) * 0.1).astype(np.float32)
    return W, b


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _n(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _twice(fn):
    """fn() -> tuple of arrays, called twice on identical inputs: identical bits; returns the first result."""
    first = fn()
    again = fn()
    for i, (p, q) in enumerate(zip(first, again)):
        assert _same(p, q), f"output {i} differs between two identical calls"
    return first


def _lse64(S64):
    m = S64.max(axis=1)
    return m + np.log(np.exp(S64 - m[:, None]).sum(axis=1))


def _record(key, data):
    try:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        cur = {}
        if os.path.exists(OUT):
            with open(OUT) as fh:
                cur = json.load(fh)
        cur[key] = data
        with open(OUT, "w") as fh:
            json.dump(cur, fh, indent=1, sort_keys=True)
    except OSError:
        pass  # a read-only tree must not fail the test


class _Case:
    """One case's inputs, engine and references."""

    def __init__(self, c, oracle):
        self.c, self.oracle = c, oracle
        self.n, self.d, self.M = c.n_item, c.d, c.M
        self.geo = c.geometry()
        self.W, self.b = _weights(self.n, self.d, 1000 + self.n + self.d)
        g = np.random.default_rng(self.M * 7 + self.d)
        self.x = g.standard_normal((self.M, self.d)).astype(np.float32)
        self.S = np.stack([oracle.score_chain(self.x[m], self.W, self.b) for m in range(self.M)])
        self.S64 = self.x.astype(np.float64) @ self.W.astype(np.float64).T + self.b.astype(np.float64)
        self.lse64 = _lse64(self.S64)
        self.eng = scoring_only_engine(self.n, self.d, self.W, self.b, max_rows=self.M)
        self.xt = _t(self.x)

    def gather_ids(self):
        """[M, 9]: id 0, id n - 1, a -1, random ids, one of them twice."""
        g = np.random.default_rng(self.n + self.M)
        ids = g.integers(0, self.n, size=(self.M, N_IDS)).astype(np.int64)
        ids[:, 0], ids[:, 1], ids[:, 2] = 0, self.n - 1, -1
        ids[:, 8] = ids[:, 5]
        return ids

    def count_inputs(self, S):
        """Reference ids (0 and n - 1 among them) and exclusion lists with a duplicate, a -1 slot, the reference id itself and
        the row's arg-max, on every row."""
        g = np.random.default_rng(self.n + 3 * self.M)
        ref = g.integers(0, self.n, size=self.M).astype(np.int64)
        ref[0], ref[1 % self.M] = 0, self.n - 1
        ref[-1], ref[-2] = self.n - 1, 0  # in the last row block too
        ex = g.integers(0, self.n, size=(self.M, N_EXCL)).astype(np.int64)
        ex[:, 1] = ex[:, 0]
        ex[:, 2] = -1
        ex[:, 3] = ref
        ex[:, 4] = S.argmax(axis=1)
        ex[:, 6] = ex[:, 4]  # the arg-max twice
        return ref, ex

    def want_ranks(self, S, ref, ex):
        return np.array([self.oracle.rank_of(S[m], int(ref[m]), ex[m][ex[m] >= 0]) for m in range(self.M)], dtype=np.int64)

    def labels(self):
        g = np.random.default_rng(self.n + 5 * self.M)
        lab = g.integers(0, self.n, size=self.M).astype(np.int64)
        lab[0], lab[1], lab[2], lab[3] = -1, 0, self.n - 1, self.n + 5
        lab[-1], lab[-2] = -1, self.n - 1  # an ignored row and the last item in the last row block
        return lab


@pytest.fixture(scope="module", params=C.CASES, ids=lambda c: c.id)
def case(request, oracle):
    k = _Case(request.param, oracle)
    yield k
    del k.eng
    torch.cuda.empty_cache()


# ============================================================================ dense
def test_dense(case):
    k = case
    (dense,) = _twice(lambda: (_n(k.eng.score_dense(k.xt)),))
    bad = np.argwhere(_bits(dense) != _bits(k.S))
    assert dense.shape == (k.M, k.n) and not len(bad), f"{k.c.id} {k.geo}: dense differs first at (row, item) {bad[:4].tolist()}"

    def wide():
        out = torch.full((k.M + 1, k.n + 3), float(SENT), dtype=torch.float32, device="cuda")
        k.eng.score_dense(k.xt, out=out)  # ld = out.stride(0) = n_local + 3
        return (_n(out),)
    (w,) = _twice(wide)
    bad = np.argwhere(_bits(w[:k.M, :k.n]) != _bits(k.S))
    assert not len(bad), f"{k.c.id} {k.geo}: dense (ld = n + 3) differs first at (row, item) {bad[:4].tolist()}"
    assert (w[:, k.n:] == SENT).all(), "padding columns written"
    assert (w[k.M] == SENT).all(), "a row past M written"


# ============================================================================ gather
def test_gather(case):
    k = case
    ids = k.gather_ids()
    (got,) = _twice(lambda: (_n(k.eng.score_gather(k.xt, _t(ids))),))
    want = np.where(ids >= 0, np.take_along_axis(k.S, np.maximum(ids, 0), axis=1), np.float32(-np.inf)).astype(np.float32)
    assert (ids[:, 2] == -1).all() and np.isneginf(got[:, 2]).all()
    assert _same(got, want), np.argwhere(_bits(got) != _bits(want))[:4].tolist()


# ============================================================================ count-before
def test_count_before(case):
    k = case
    ref, ex = k.count_inputs(k.S)
    ref_score = k.S[np.arange(k.M), ref]
    (cnt,) = _twice(lambda: (_n(k.eng.score_count_before(k.xt, _t(ref_score), _t(ref), _t(ex))),))
    want = k.want_ranks(k.S, ref, ex)
    assert np.array_equal(cnt + 1, want), f"{k.c.id} {k.geo}: rows {np.where(cnt + 1 != want)[0][:8].tolist()}"
    (plain,) = _twice(lambda: (_n(k.eng.score_count_before(k.xt, _t(ref_score), _t(ref), None)),))
    want0 = np.array([k.oracle.rank_of(k.S[m], int(ref[m]), np.zeros(0, dtype=np.int64)) for m in range(k.M)])
    assert np.array_equal(plain + 1, want0)
    assert (want0 > want).any(), "the exclusions took nothing away"


def test_count_before_ties(case):
    """7 distinct item rows and a constant bias (the construction of test_topk_ties_and_fallback at this case's catalog): every
    reference is tied exactly with about n / 7 items, and only those with a smaller id count."""
    k = case
    W, b = _weights(k.n, k.d, 3)
    W[:] = W[:7][np.arange(k.n) % 7]
    b[:] = 0.25
    s7 = np.stack([k.oracle.score_chain(k.x[m], W[:7], b[:7]) for m in range(k.M)])
    S = np.ascontiguousarray(s7[:, np.arange(k.n) % 7])  # an item's chain depends on its own row only
    if k.M > 3:
        assert _same(S[3], k.oracle.score_chain(k.x[3], W, b))
    eng = scoring_only_engine(k.n, k.d, W, b, max_rows=k.M)
    ref, ex = k.count_inputs(S)
    ex[:, 5] = np.maximum(ref - 7, 0)   # a tied item in front of the reference (or the reference itself)
    ex[:, 7] = np.minimum(ref + 7, k.n - 1)  # and one behind it
    ref_score = S[np.arange(k.M), ref]
    (cnt,) = _twice(lambda: (_n(eng.score_count_before(k.xt, _t(ref_score), _t(ref), _t(ex))),))
    want = k.want_ranks(S, ref, ex)
    assert np.array_equal(cnt + 1, want), f"{k.c.id} {k.geo}: rows {np.where(cnt + 1 != want)[0][:8].tolist()}"
    (plain,) = _twice(lambda: (_n(eng.score_count_before(k.xt, _t(ref_score), _t(ref), None)),))
    ties_in_front = np.array([(S[m, :ref[m]] == ref_score[m]).sum() for m in range(k.M)])
    above = (S > ref_score[:, None]).sum(axis=1)
    assert np.array_equal(plain, above + ties_in_front)
    if k.n >= 70:
        assert ties_in_front.max() >= 2 and ((S == ref_score[:, None]).sum(axis=1) > ties_in_front + 1).any()


# ============================================================================ log-sum-exp
def _check_lse(k, mx, sm, what):
    """max + log(sum) against logsumexp(S64[m]) on every row, the project's bar."""
    got = mx.astype(np.float64) + np.log(sm.astype(np.float64))
    err = np.abs(got - k.lse64)
    bar = LSE_BAR * np.maximum(1.0, np.abs(k.lse64))
    print(f"{k.c.id} {what}: lse err max {err.max():.3e} (bar {bar.min():.3e})")
    assert (err <= bar).all(), f"{k.c.id} {what} {k.geo}: rows {np.where(err > bar)[0][:8].tolist()}, err {err.max():.3e}"


def _check_max_bits(k, mx, what):
    """max == S[m].max() in every bit."""
    smax = k.S.max(axis=1)
    off = np.where(_bits(mx) != _bits(smax))[0]
    ulps = np.abs(_bits(mx).astype(np.int64) - _bits(smax).astype(np.int64))  # (both maxima are positive here)
    print(f"{k.c.id} {what}: max differs from S.max() on {len(off)} of {k.M} rows, at most {int(ulps.max())} ulp")
    assert not len(off), (f"{k.c.id} {what} {k.geo}: max != S.max() on {len(off)} of {k.M} rows (first {off[:6].tolist()}), "
                          f"at most {int(ulps.max())} ulp")


def test_lse(case):
    k = case
    mx, sm = _twice(lambda: tuple(_n(v) for v in k.eng.score_lse(k.xt)))
    _check_lse(k, mx, sm, f"lse[{k.geo['lse_form']}]")


def test_lse_max_bits(case):
    """The row maximum irs_score_lse returns against the chain's, S[m].max(), bit for bit, in every log-sum-exp form.  The forms that
    load 16-byte fragments (k_lse_f32, k_lse_ring, the vector form of the generic sweep) get the four consecutive k of a lane half per
    load and exchange halves in registers (chain_pairs in score.hip), so that the MFMAs sum k in the chain's order.  Before that
    exchange they summed 0, 4, 1, 5, ...: this test then failed at every width with d == d_pad (up to 237 of 520 rows, 1 to 6 ulp) and
    passed at the scalar-staging widths."""
    k = case
    mx, _ = _twice(lambda: tuple(_n(v) for v in k.eng.score_lse(k.xt)))
    _check_max_bits(k, mx, f"lse[{k.geo['lse_form']}]")


@pytest.fixture(scope="module", params=C.misaligned_lse_cases(), ids=lambda c: c.id)
def misaligned(request, oracle):
    """xrows as a contiguous view 4 bytes into its buffer: lse_fast_ok fails and the generic MODE_LSE sweep runs at KS >= 2.  Its
    x staging (k_sweep_f32's prologue) reads x32 one float at a time; the 16-byte loads are on the weights (guarded by `vec`)."""
    c = request.param
    assert c.geometry()["lse_form"] == "fast" and c.geometry(aligned=False)["lse_form"] == "generic"
    k = _Case(c, oracle)
    buf = torch.zeros(k.M * k.d + 1, dtype=torch.float32, device="cuda")
    xm = buf[1:].view(k.M, k.d)
    xm.copy_(k.xt)
    assert xm.is_contiguous() and xm.data_ptr() % 16 == 4
    yield k, xm
    del k.eng


def test_lse_misaligned_rows(misaligned):
    k, xm = misaligned
    mx, sm = _twice(lambda: tuple(_n(v) for v in k.eng.score_lse(xm)))
    _check_lse(k, mx, sm, "lse[generic, misaligned]")
    fm, fs = (_n(v) for v in k.eng.score_lse(k.xt))  # the aligned call's 16-byte-fragment form sums a score in the same order
    assert _same(mx, fm)


def test_lse_misaligned_rows_max_bits(misaligned):
    """As test_lse_max_bits, on the generic sweep with vector-staged weights that misaligned rows fall back to."""
    k, xm = misaligned
    mx, _ = _twice(lambda: tuple(_n(v) for v in k.eng.score_lse(xm)))
    _check_max_bits(k, mx, "lse[generic, misaligned]")


# ============================================================================ cross entropy
def test_ce(case):
    k = case
    lab = k.labels()
    labt = _t(lab)
    valid = (lab >= 0) & (lab < k.n)
    lse, ls, loss = _twice(lambda: tuple(_n(v) for v in k.eng.ce_forward(k.xt, labt)))
    err = np.abs(lse.astype(np.float64) - k.lse64)
    bar = LSE_BAR * np.maximum(1.0, np.abs(k.lse64))
    assert (err <= bar).all(), f"{k.c.id} {k.geo}: lse rows {np.where(err > bar)[0][:8].tolist()}, err {err.max():.3e}"
    rows = np.where(valid)[0]
    assert _same(ls[rows], k.S[rows, lab[rows]]), "label scores"
    assert np.isneginf(ls[~valid]).all()
    assert loss[1] == valid.sum() and loss[2] == (lab >= k.n).sum() == 1
    own = (lse[rows].astype(np.float64) - ls[rows].astype(np.float64)).sum()  # the sum of the call's own float32 outputs, in float64
    assert abs(loss[0] - own) <= 1e-12 * k.M * max(1.0, abs(own))
    want = (k.lse64[rows] - k.S64[rows, lab[rows]]).sum()
    slack = (bar[rows] + np.abs(k.S[rows, lab[rows]].astype(np.float64) - k.S64[rows, lab[rows]])).sum()
    assert abs(loss[0] - want) <= slack, (loss[0], want, slack)

    # the gradient, into a wider buffer
    scale = 1.0 / float(valid.sum())
    lset = _t(lse)

    def grad():
        out = torch.full((k.M + 1, k.n + 3), float(SENT), dtype=torch.float32, device="cuda")
        k.eng.ce_grad_logits(k.xt, labt, lset, scale, out)
        return (_n(out),)
    (G,) = _twice(grad)
    assert (G[:, k.n:] == SENT).all() and (G[k.M] == SENT).all(), "padding written"
    G = G[:k.M, :k.n]
    ign = lab < 0
    assert ign.sum() >= 2 and (_bits(G[ign]) == 0).all(), "ignored rows are exactly +0"
    onehot = np.zeros((k.M, k.n))
    onehot[rows, lab[rows]] = 1.0
    G64 = scale * (np.exp(k.S64 - k.lse64[:, None]) - onehot)
    G64[ign] = 0.0
    s32 = np.float32(scale)
    G32 = s32 * (np.exp(k.S - lse[:, None]) - onehot.astype(np.float32))
    assert G32.dtype == np.float32
    G32[ign] = 0.0
    e32 = float(np.abs(G32.astype(np.float64) - G64).max())
    e = float(np.abs(G.astype(np.float64) - G64).max())
    gbar = max(4.0 * e32, 2e-6 * scale)
    over = lab >= k.n  # subtracts nowhere: the whole row is a plain softmax
    assert (G[over] > 0).all() and abs(float(G[over].astype(np.float64).sum()) - scale) <= 1e-4 * scale
    assert (G[rows, lab[rows]] < 0).all()
    soft = onehot == 0  # for the record: the same two errors off the labels, where a value is scale * p and p is small
    m = dict(float32_formula_err=e32, kernel_err=e, bar=gbar, scale=scale, KS=k.geo["KS"], vec=k.geo["vec"], n_ublocks=k.geo["n_ublocks"],
             float32_formula_err_off_label=float(np.abs(G32.astype(np.float64) - G64)[soft].max()),
             kernel_err_off_label=float(np.abs(G.astype(np.float64) - G64)[soft].max()), largest_off_label=float(G64[soft].max()))
    print(k.c.id, json.dumps(m, sort_keys=True))
    _record(k.c.id, m)
    assert e <= gbar, (k.c.id, m)


# ============================================================================ the path trace's sweep
@pytest.mark.parametrize("c", [c for c in C.CASES if c.trace], ids=lambda c: c.id)
def test_trace_sweep(c):
    """irs_score_target_trace alone above one row block: the assertions of tests/test_gpu_path_trace.py::test_sweep_alone (its
    shapes end at 70 rows at d = 128 and 37 at d = 256: one row block each), at n_ublocks = 2 and 3 for KS 2, 8 and 16."""
    assert c.geometry()["n_ublocks"] in (2, 3)
    PT.test_sweep_alone(c.n_item, c.d, c.M)


# ============================================================================ item shards
@pytest.mark.parametrize("c", [c for c in C.CASES if c.shards], ids=lambda c: c.id)
def test_shards(c, oracle):
    """world = 3 item shards (item_lo > 0, n_local < n_item) of the KS 2 scalar-staging, KS 8 and KS 16 cases with two row blocks."""
    k = _Case(c, oracle)
    engs = [scoring_only_engine(k.n, k.d, k.W, k.b, max_rows=k.M, rank=r, world=C.WORLD) for r in range(C.WORLD)]
    bounds = [(e.item_lo, e.item_hi) for e in engs]
    assert bounds == [C.shard_bounds(k.n, C.WORLD, r) for r in range(C.WORLD)]
    # dense: the shards' columns side by side
    parts = [_twice(lambda e=e: (_n(e.score_dense(k.xt)),))[0] for e in engs]
    assert [p.shape[1] for p in parts] == [hi - lo for lo, hi in bounds]
    assert _same(np.concatenate(parts, axis=1), k.S)
    # gather: -inf on exactly the two shards that do not own the id
    ids = k.gather_ids()
    got = np.stack([_twice(lambda e=e: (_n(e.score_gather(k.xt, _t(ids))),))[0] for e in engs])
    want = np.where(ids >= 0, np.take_along_axis(k.S, np.maximum(ids, 0), axis=1), np.float32(-np.inf)).astype(np.float32)
    assert _same(got.max(axis=0), want)
    owner = np.stack([(ids >= lo) & (ids < hi) for lo, hi in bounds])
    assert (owner.sum(axis=0) == (ids >= 0)).all() and np.array_equal(np.isneginf(got), ~owner)
    assert all(owner[r].any() for r in range(C.WORLD))
    # count-before: the shards' counts add up, the reference being local to one of them
    ref, ex = k.count_inputs(k.S)
    ref_score = k.S[np.arange(k.M), ref]
    cnts = [_twice(lambda e=e: (_n(e.score_count_before(k.xt, _t(ref_score), _t(ref), _t(ex))),))[0] for e in engs]
    want_rank = k.want_ranks(k.S, ref, ex)
    assert np.array_equal(sum(cnts) + 1, want_rank), np.where(sum(cnts) + 1 != want_rank)[0][:8].tolist()
    assert all(((ref >= lo) & (ref < hi)).any() for lo, hi in bounds)
    # log-sum-exp: the host combination of the three (max, sum) pairs
    pairs = [_twice(lambda e=e: tuple(_n(v) for v in e.score_lse(k.xt))) for e in engs]
    mx = np.stack([p[0] for p in pairs]).astype(np.float64)
    sm = np.stack([p[1] for p in pairs]).astype(np.float64)
    top = mx.max(axis=0)
    got_lse = top + np.log((sm * np.exp(mx - top)).sum(axis=0))
    err = np.abs(got_lse - k.lse64)
    assert (err <= LSE_BAR * np.maximum(1.0, np.abs(k.lse64))).all(), err.max()
    for r, (lo, hi) in enumerate(bounds):  # and each shard's pair on its own columns
        part = _lse64(k.S64[:, lo:hi])
        e1 = np.abs(mx[r] + np.log(sm[r]) - part)
        assert (e1 <= LSE_BAR * np.maximum(1.0, np.abs(part))).all(), (r, e1.max())
