"""-m gpu: the kernels that turn scores into paths, alone, against the plain references of tests/path_ref.py
(themselves tied to the reference's golden paths, oracle_np.beam_search and the contract golden by
test_path_ref_host.py): k_path_step / irs_path_step_row, k_beam_step, k_merge / k_pack_topk, k_build_eval_batch.

Inputs are synthetic and built to sit on the edges (window lengths around the 64-lane registers, partial workgroups,
exact ties, dead beams, the second round of 64 candidates, -1 holes, users without events).  The engine is a dummy:
nothing depends on a model, except the last test, which runs a whole search against its own parts.

Tolerances: 1e-12 on float64 beam scores where log(sum exp) is not exact (device log against numpy's), and the
binomial 6-sigma bound  |count - n p| <= 6 sqrt(n p (1 - p)) + 1  on every frequency (n independent draws of
probability p have standard deviation sqrt(n p (1 - p)); 6 sigma is a chance of about 2e-9 per count, the + 1 covers
the 24-bit uniform and the float32 exp of the device).  The inputs are fixed, so every run sees the same counts.
Everything else is equality."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import path_ref
from gpu_util import make_engine, path_only_engine
from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_SWEEP_BF16

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E_INVALID, E_UNSUPPORTED = -1, -4
NO_CAND = path_ref.NO_CANDIDATE


@functools.lru_cache(maxsize=None)
def _engine(L, n_item=64):
    return path_only_engine(L, n_item=n_item)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.cpu().numpy()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sigma6(n, p):
    """The binomial 6-sigma bound of the module docstring."""
    return 6.0 * math.sqrt(n * p * (1.0 - p)) + 1.0


def _desc_vals(g, k):
    """k strictly descending float32 scores."""
    return np.sort(g.permutation(4 * k)[:k].astype(np.float32) * 0.125 - 7.0)[::-1].copy()


def _fill_window(g, L, hep, ids_row, c, *, survivor_is_target, pads=True):
    """A window of length L whose live part [0, hep] holds the leading c candidates of ids_row (c <= hep + 1), pad
    zeros and a duplicate; the first survivor also sits at a stale position past hep and, on request, at the target."""
    win = g.integers(6001, 9000, size=L).astype(np.int64)
    wl = hep + 1
    if pads and wl >= 3:
        win[g.integers(0, wl)] = 0
    if wl >= 2:
        win[1] = win[0]  # a duplicate item
    slots = g.permutation(wl)[:c]
    win[slots] = ids_row[:c] + 1
    first = int(ids_row[c]) + 1 if c < len(ids_row) and ids_row[c] >= 0 else 0
    if first and hep + 1 <= L - 2:
        win[g.integers(hep + 1, L - 1)] = first  # stale: only past hep
    if first and survivor_is_target:
        win[L - 1] = first
    return win


# --------------------------------------------------------------------------------------------- path step, greedy
def _greedy_case(L, B, k, seed):
    """Rows cycle through hep in {0, mid, L-3 (last grow), L-2 (shift)} and through the number of leading candidates
    placed in the window, c in {0, 1, k-1, k} (clipped to the window), plus a row whose list has -1 before its
    first survivor."""
    g = np.random.default_rng(seed)
    heps = [0, max(0, (L - 2) // 2), max(0, L - 3), L - 2]
    modes = [0, 1, k - 1, k, "hole"]
    off = int(g.integers(0, 20))
    seq = np.zeros((B, L), dtype=np.int64)
    hep = np.zeros(B, dtype=np.int32)
    val = np.zeros((B, k), dtype=np.float32)
    ids0 = np.zeros((B, k), dtype=np.int64)
    info = []
    for r in range(B):
        he = heps[(r + off) % 4]
        mode = modes[(r + off) % 5]
        ids0[r] = g.permutation(5000)[:k]
        val[r] = _desc_vals(g, k)
        c = min(k - 1 if mode == "hole" else mode, he + 1)
        if mode == "hole":
            ids0[r, c] = -1  # valid entries follow unless c == k - 1
        seq[r] = _fill_window(g, L, he, ids0[r], c, survivor_is_target=(r % 3 == 0))
        hep[r] = he
        info.append((he, mode, c))
    status = np.array([0, 1, 4, 5], dtype=np.int32)[(np.arange(B) // 2) % 4]
    return seq, hep, val, ids0, status, info


def _run_path_step(eng, seq, hep, val, ids0, step, paths, status, guard=2, **kw):
    """Runs irs_path_step on the leading B rows of buffers that carry `guard` more rows; returns the outputs, after
    checking that the guard rows, val and ids0 are untouched."""
    B = seq.shape[0]

    def padded(a, fill):
        return _t(np.concatenate([a, np.full((guard,) + a.shape[1:], fill, dtype=a.dtype)]))
    d_seq, d_hep, d_paths, d_st = padded(seq, 4242), padded(hep, 1), padded(paths, 555.0), padded(status, 8)
    d_val, d_ids = _t(val), _t(ids0)
    eng.path_step(d_seq[:B], d_hep[:B], d_val, d_ids, step, d_paths[:B], d_st[:B], **kw)
    torch.cuda.synchronize()
    assert (_n(d_seq[B:]) == 4242).all() and (_n(d_hep[B:]) == 1).all()
    assert (_n(d_paths[B:]) == 555.0).all() and (_n(d_st[B:]) == 8).all()
    assert np.array_equal(_n(d_val).view(np.uint32), val.view(np.uint32)) and np.array_equal(_n(d_ids), ids0)
    return _n(d_seq[:B]), _n(d_hep[:B]), _n(d_paths[:B]), _n(d_st[:B])


@pytest.mark.parametrize("k", [1, 3, 64, 65, 100])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 67])
@pytest.mark.parametrize("L", [3, 10, 64, 65, 200, 256])
def test_path_step_greedy_exact(L, B, k):
    eng = _engine(L)
    seq, hep, val, ids0, status, info = _greedy_case(L, B, k, seed=L * 10007 + B * 101 + k)
    step, path_ld = 2, 5
    paths = np.full((B, path_ld), 777.0, dtype=np.float32)
    want = path_ref.path_step(seq, hep, val, ids0, step, paths, status)
    got = _run_path_step(eng, seq, hep, val, ids0, step, paths, status)
    for name, w, g_ in zip(("seq", "hep", "paths", "status"), want, got):
        assert np.array_equal(w, g_), (name, np.argwhere(w != g_)[:8])
    g_seq, g_hep, g_paths, g_st = got
    assert (g_paths[:, [0, 1, 3, 4]] == 777.0).all()           # other path columns
    assert ((g_st & 5) == status).all()                         # bits already set survive the OR
    for r, (he, mode, c) in enumerate(info):
        exhausted = mode == "hole" or c == k
        assert bool(g_st[r] & NO_CAND) == exhausted, (r, he, mode, c)
        if exhausted:  # no candidate: a zero path entry, window and hep as they were
            assert g_paths[r, step] == 0 and np.array_equal(g_seq[r], seq[r]) and g_hep[r] == he
            continue
        chosen = ids0[r, c] + 1
        assert g_paths[r, step] == chosen
        if r % 3 == 0:
            assert chosen == seq[r, L - 1]                      # the target is not filtered, and is chosen
        if he < L - 2:                                          # grow: only [hep + 1] changes
            assert g_hep[r] == he + 1 and g_seq[r, he + 1] == chosen
            assert np.array_equal(np.delete(g_seq[r], he + 1), np.delete(seq[r], he + 1))
        else:                                                   # shift: the whole row
            assert g_hep[r] == he and g_seq[r, L - 2] == chosen and g_seq[r, L - 1] == seq[r, L - 1]
            assert np.array_equal(g_seq[r, :L - 2], seq[r, 1:L - 1])
    if B == 67:  # every combination is present in the large launch: both branches run side by side
        seen = {(he, mode) for he, mode, c in info}
        assert len({he for he, _ in seen}) == len({0, max(0, (L - 2) // 2), max(0, L - 3), L - 2})
        assert {m for _, m in seen} == {0, 1, k - 1, k, "hole"}
        assert any(c == k for _, m, c in info if m != "hole") or L - 1 < k


def test_path_step_argument_contract():
    L, B, k = 10, 3, 5
    eng = _engine(L)
    seq, hep, val, ids0, status, _ = _greedy_case(L, B, k, seed=1)
    paths = np.full((B, 4), 777.0, dtype=np.float32)
    d = [_t(a) for a in (seq, hep, val, ids0, paths, status)]
    d_seq, d_hep, d_val, d_ids, d_paths, d_st = d

    def call(seq_=d_seq, hep_=d_hep, val_=d_val, ids_=d_ids, k_=k, step=0, paths_=d_paths, ld=4, sample=0, sk=3, st=d_st):
        rc = eng.lib.irs_path_step(eng.h, _ptr(seq_), _ptr(hep_), B, _ptr(val_), _ptr(ids_), k_, step, _ptr(paths_), ld,
                                   sample, sk, 0, _ptr(st), _stream())
        torch.cuda.synchronize()
        return rc
    assert call(step=4) == E_INVALID and call(step=7) == E_INVALID and call(step=-1) == E_INVALID
    assert call(k_=0) == E_INVALID and call(k_=-3) == E_INVALID
    assert call(sample=1, sk=0) == E_UNSUPPORTED and call(sample=1, sk=9) == E_UNSUPPORTED
    for name in ("seq_", "hep_", "val_", "ids_", "paths_", "st"):
        assert call(**{name: None}) == E_INVALID, name
    for t, a in zip(d, (seq, hep, val, ids0, paths, status)):  # rejected before any write
        assert np.array_equal(_n(t), a)
    assert call(step=3) == 0 and call(sample=1, sk=8) == 0 and call(sk=0) == 0  # sample_k is ignored when greedy


# --------------------------------------------------------------------------------------------- path step, sampled
SAMPLE_B = 65536


def _sampled_inputs(scenario, sample_k):
    """Identical rows: L = 8, hep = 2, the two leading candidates in the window.  Returns (seq, hep, val, ids0)."""
    L, k = 8, 14
    ids_row = np.arange(100, 100 + k, dtype=np.int64) * 3
    val_row = np.array([3.0, 2.5, 2.0, 1.75, 1.0, 0.875, 0.5, 0.25, 0.0, -0.5, -1.0, -1.5, -2.0, -2.5], dtype=np.float32)
    if scenario == "equal":
        val_row[:] = 1.25
    elif scenario == "minus30":  # the last of the first sample_k survivors (the 2nd when sample_k == 1) is e^-30 times as likely
        low = 2 + max(sample_k, 2) - 1
        val_row[3:low] = val_row[2]
        val_row[low:] = val_row[2] - 30.0 - np.arange(k - low, dtype=np.float32)  # the list stays descending
    elif scenario == "fewer":  # sample_k - 1 survivors, then the end of the list
        ids_row[2 + sample_k - 1] = -1
    win = np.array([ids_row[1] + 1, 0, ids_row[0] + 1, 0, 0, 0, 0, 4000], dtype=np.int64)
    seq = np.repeat(win[None], SAMPLE_B, axis=0)
    hep = np.full(SAMPLE_B, 2, dtype=np.int32)
    return seq, hep, np.repeat(val_row[None], SAMPLE_B, axis=0), np.repeat(ids_row[None], SAMPLE_B, axis=0)


def _sample_once(eng, inputs, step, sample_k, seed, path_ld=8):
    seq, hep, val, ids0 = inputs
    paths = np.zeros((SAMPLE_B, path_ld), dtype=np.float32)
    status = np.zeros(SAMPLE_B, dtype=np.int32)
    return _run_path_step(eng, seq, hep, val, ids0, step, paths, status, sample=True, sample_k=sample_k, seed=seed)


@pytest.mark.parametrize("scenario", ["plain", "fewer", "equal", "minus30"])
@pytest.mark.parametrize("sample_k", [1, 2, 3, 8])
def test_path_step_sampled_frequencies(sample_k, scenario):
    eng = _engine(8)
    inputs = _sampled_inputs(scenario, sample_k)
    seq, hep, val, ids0 = inputs
    n, step = SAMPLE_B, 3
    dist = path_ref.path_step(seq[:1], hep[:1], val[:1], ids0[:1], step, np.zeros((1, 8), np.float32), np.zeros(1, np.int32),
                              sample=True, sample_k=sample_k)[0]
    items, p = dist
    g_seq, g_hep, g_paths, g_st = _sample_once(eng, inputs, step, sample_k, seed=11)
    again = _sample_once(eng, inputs, step, sample_k, seed=11)
    for a, b in zip((g_seq, g_hep, g_paths, g_st), again):
        assert np.array_equal(a, b)                                       # same seed, same choices
    choice = g_paths[:, step]
    assert not g_paths[:, [0, 1, 2, 4, 5, 6, 7]].any()
    if len(items) == 0:  # sample_k == 1 with "fewer": nothing survives
        assert scenario == "fewer" and sample_k == 1
        assert (g_st == NO_CAND).all() and not choice.any() and np.array_equal(g_seq, seq) and np.array_equal(g_hep, hep)
        return
    assert len(items) == (sample_k - 1 if scenario == "fewer" else sample_k)
    assert not g_st.any()
    assert np.isin(choice, items).all()                                   # one of the first sample_k survivors
    want_seq = seq.copy()
    want_seq[:, 3] = choice.astype(np.int64)
    assert np.array_equal(g_seq, want_seq) and (g_hep == 3).all()        # the window grows by the chosen item
    for it, pi in zip(items, p):
        cnt = int((choice == it).sum())
        print(f"sample_k={sample_k} {scenario}: item {it} p={pi:.6g} count={cnt} expected={n * pi:.1f} bound={_sigma6(n, pi):.1f}")
        assert abs(cnt - n * pi) <= _sigma6(n, pi), (it, cnt, n * pi)     # 6 sqrt(n p (1 - p)) + 1
    if scenario == "minus30" and sample_k > 1:
        assert p[-1] < 1e-12 and int((choice == items[-1]).sum()) == 0    # e^-30: never drawn
    if (p > 1e-3).sum() > 1:  # a real choice exists
        other = _sample_once(eng, inputs, step, sample_k, seed=12)[2][:, step]
        assert not np.array_equal(other, choice)                          # a different seed, different choices
    if sample_k == 1:  # equals greedy
        gr = _run_path_step(eng, seq, hep, val, ids0, step, np.zeros((n, 8), np.float32), np.zeros(n, np.int32))
        for a, b in zip((g_seq, g_hep, g_paths, g_st), gr):
            assert np.array_equal(a, b)


def test_path_step_sampled_independence():
    """The counter RNG (row * 1315423911 + step + 1): choices at consecutive steps of a row, and of neighbouring rows
    at one step, are independent.  Steps 0..7 each run from the same fresh state.  Joint counts against the product of
    the marginals' expectation, n p_i p_j, with the bound of the module docstring for q = p_i p_j.  The row pairs are
    the disjoint ones (2r, 2r + 1), so that the n = 8 B / 2 pairs are independent draws and the binomial bound applies
    as it stands."""
    eng = _engine(8)
    inputs = _sampled_inputs("plain", 3)
    seq, hep, val, ids0 = inputs
    items, p = path_ref.path_step(seq[:1], hep[:1], val[:1], ids0[:1], 0, np.zeros((1, 8), np.float32),
                                  np.zeros(1, np.int32), sample=True, sample_k=3)[0]
    assert len(items) == 3 and (np.diff(items) > 0).all()
    idx = []
    for step in range(8):
        choice = _sample_once(eng, inputs, step, 3, seed=2024)[2][:, step]
        assert np.isin(choice, items).all()
        idx.append(np.searchsorted(items, choice.astype(np.int64)))
    idx = np.stack(idx)  # [8, B] index of the chosen survivor (items ascend in these inputs)
    m = len(items)
    for s in range(7):
        joint = np.bincount(idx[s] * m + idx[s + 1], minlength=m * m).reshape(m, m)
        for i in range(m):
            for j in range(m):
                q = p[i] * p[j]
                assert abs(joint[i, j] - SAMPLE_B * q) <= _sigma6(SAMPLE_B, q), ("steps", s, i, j, joint[i, j], SAMPLE_B * q)
    n = 8 * SAMPLE_B // 2
    joint = np.bincount((idx[:, 0::2] * m + idx[:, 1::2]).reshape(-1), minlength=m * m).reshape(m, m)
    for i in range(m):
        for j in range(m):
            q = p[i] * p[j]
            assert abs(joint[i, j] - n * q) <= _sigma6(n, q), ("rows", i, j, joint[i, j], n * q)


# --------------------------------------------------------------------------------------------- beam step
def _beam_case(B, W, k, L, P, step, seed, *, ties=False, dead_frac=0.3, force_c=None, holes=True, lse=True):
    """Random beam state and candidate lists.  Every beam draws its own hep from {0, mid, L-3, L-2} (grow and shift
    parents under one user), its number of leading candidates inside the window, and possibly a -1 in mid-list; dead
    input beams are interleaved with live ones and carry ordinary-looking lists; paths_in holds garbage from `step` on.
    ties: lse_max = 0, lse_sum = 1, val and cum multiples of 1/4 from small sets, so that float64 sums are exact and
    equal scores meet across parents and inside a parent."""
    g = np.random.default_rng(seed)
    heps = [0, max(0, (L - 2) // 2), max(0, L - 3), L - 2]
    seq = np.zeros((B, W, L), dtype=np.int64)
    hep = np.zeros((B, W), dtype=np.int32)
    cum = np.zeros((B, W), dtype=np.float64)
    paths = g.integers(1, 5000, size=(B, W, P)).astype(np.float32)
    paths[:, :, step:] = 12345.0
    val = np.zeros((B * W, k), dtype=np.float32)
    ids0 = np.zeros((B * W, k), dtype=np.int64)
    for row in range(B * W):
        b, j = divmod(row, W)
        he = heps[int(g.integers(0, 4))] if force_c is None else L - 2
        ids0[row] = g.permutation(5000)[:k]
        if ties:
            val[row] = np.sort(g.integers(-3, 1, size=k).astype(np.float32) * 0.25)[::-1]
            cum[b, j] = float(g.integers(-2, 1)) * 0.25
        else:
            val[row] = _desc_vals(g, k)
            cum[b, j] = -float(g.random()) * 20.0
        c = force_c if force_c is not None else [0, 1, k - 1, k][int(g.integers(0, 4))]
        c = min(c, he + 1, k)
        if holes and k > 2 and g.random() < 0.3:
            ids0[row, int(g.integers(1, k))] = -1  # ends this beam's list
        seq[b, j] = _fill_window(g, L, he, np.where(ids0[row] >= 0, ids0[row], 0), c, survivor_is_target=bool(g.integers(0, 2)))
        hep[b, j] = he
        if g.random() < dead_frac:
            cum[b, j] = -np.inf
    if ties or not lse:
        lmax, lsum = np.zeros(B * W, dtype=np.float32), np.ones(B * W, dtype=np.float32)
    else:
        lmax = (g.random(B * W) * 8.0).astype(np.float32)
        lsum = (1.0 + g.random(B * W) * 500.0).astype(np.float32)
    status = g.choice(np.array([0, 1, 4, 5], dtype=np.int32), size=B)
    return dict(state=(seq, hep, cum, paths), val=val, ids0=ids0, lse=(lmax, lsum), status=status, step=step, P=P)


def _beam_gpu(eng, case, guard=1):
    seq, hep, cum, paths = case["state"]
    B, W, L = seq.shape
    P = case["P"]
    d_in = tuple(_t(a) for a in case["state"])
    outs = (torch.full((B + guard, W, L), 4242, dtype=torch.int64, device=DEV),
            torch.full((B + guard, W), 7, dtype=torch.int32, device=DEV),
            torch.full((B + guard, W), 3.5, dtype=torch.float64, device=DEV),
            torch.full((B + guard, W, P), 555.0, dtype=torch.float32, device=DEV))
    d_st = _t(np.concatenate([case["status"], np.full(guard, 8, dtype=np.int32)]))
    d_val, d_ids = _t(case["val"]), _t(case["ids0"])
    lse = tuple(_t(a) for a in case["lse"]) if W > 1 or case.get("pass_lse") else None
    eng.beam_step(d_in, d_val, d_ids, lse, case["step"], tuple(o[:B] for o in outs), d_st[:B])
    torch.cuda.synchronize()
    for t, a in zip(d_in, case["state"]):
        assert np.array_equal(_n(t), a, equal_nan=True)        # the input state is read-only
    assert np.array_equal(_n(d_val), case["val"]) and np.array_equal(_n(d_ids), case["ids0"])
    assert (_n(outs[0][B:]) == 4242).all() and (_n(outs[1][B:]) == 7).all() and (_n(outs[2][B:]) == 3.5).all()
    assert (_n(outs[3][B:]) == 555.0).all() and (_n(d_st[B:]) == 8).all()
    return tuple(_n(o[:B]) for o in outs), _n(d_st[:B])


def _beam_check(eng, case, exact_cum):
    seq, hep, cum, paths = case["state"]
    W = seq.shape[1]
    lmax, lsum = case["lse"] if W > 1 else (None, None)
    (w_seq, w_hep, w_cum, w_paths), w_st = path_ref.beam_step(case["state"], case["val"], case["ids0"], lmax, lsum,
                                                                case["step"], case["P"], case["status"])
    (g_seq, g_hep, g_cum, g_paths), g_st = _beam_gpu(eng, case)
    assert np.array_equal(np.isfinite(w_cum), np.isfinite(g_cum)) and (np.isneginf(g_cum) | np.isfinite(g_cum)).all()
    fin = np.isfinite(w_cum)
    if exact_cum:
        assert np.array_equal(w_cum, g_cum)
    else:
        live = w_cum[fin]
        if len(live) > 1:  # well separated: no two scores of the case within 1e-9 (an assertion on the inputs)
            for b in range(w_cum.shape[0]):
                assert (np.abs(np.diff(w_cum[b][fin[b]])) > 1e-9).all()
        assert (np.abs(w_cum[fin] - g_cum[fin]) <= 1e-12).all(), np.abs(w_cum[fin] - g_cum[fin]).max()
    assert np.array_equal(w_paths, g_paths), np.argwhere(w_paths != g_paths)[:8]
    assert np.array_equal(w_seq, g_seq), np.argwhere(w_seq != g_seq)[:8]
    assert np.array_equal(w_hep, g_hep) and np.array_equal(w_st, g_st)
    assert ((g_st & 5) == case["status"]).all()                 # pre-set bits survive
    assert not g_paths[:, :, case["step"] + 1:].any()            # garbage of paths_in does not leak
    return (g_seq, g_hep, g_cum, g_paths), g_st


BEAM_W = [1, 2, 3, 4, 5, 16, 17, 32]


def _beam_grid():
    """Every W with every k of {1, W-1, 64, 65, 100} (k >= 1); L, P, step position and B cycle through their values so
    that each appears with small and with large W."""
    out, n = [], 0
    for W in BEAM_W:
        for k in sorted({1, max(1, W - 1), 64, 65, 100}):
            for rep in range(2):
                L = [10, 65, 256][(n + rep) % 3]
                P = [1, 5, 64][(n // 3 + rep) % 3]
                step = [0, P // 2, P - 1][(n // 2 + rep) % 3]
                B = [1, 3][(n + rep) % 2]
                out.append((W, k, L, P, step, B))
            n += 1
    return out


@pytest.mark.parametrize("W,k,L,P,step,B", _beam_grid())
def test_beam_step_random_separated(W, k, L, P, step, B):
    """Random well-separated scores, with dead input beams, holes, mixed hep, garbage paths and pre-set status bits:
    cum within 1e-12, everything else exact."""
    case = _beam_case(B, W, k, L, P, step, seed=W * 7919 + k * 31 + L + P + step + B)
    _beam_check(_engine(L), case, exact_cum=(W == 1))


@pytest.mark.parametrize("W,k,L,P,step,B", _beam_grid())
def test_beam_step_exact_ties(W, k, L, P, step, B):
    """Equal scores across parents, inside a parent and both: the order is (score desc, parent asc, rank asc), and
    everything, cum included, is compared exactly."""
    case = _beam_case(B, W, k, L, P, step, seed=W * 104729 + k * 37 + L + P + step + B, ties=True, dead_frac=0.15)
    (g_seq, g_hep, g_cum, g_paths), _ = _beam_check(_engine(L), case, exact_cum=True)
    if W >= 16 and k >= W - 1:
        fin = np.isfinite(g_cum)
        assert any((np.diff(g_cum[b][fin[b]]) == 0).any() for b in range(B)), "the case was built to contain ties"


def test_beam_step_tie_order_spelled_out():
    """The documented order (score desc, parent asc, rank asc) on three hand-built users, W = k = 4: equal scores across
    parents; equal scores inside one parent; both at once (five candidates tie, the first four by (parent, rank) win)."""
    B, W, k, L, P, step = 3, 4, 4, 10, 5, 2
    case = _beam_case(B, W, k, L, P, step, seed=21, ties=True, dead_frac=0.0, holes=False, force_c=0)
    seq, hep, cum, paths = case["state"]
    val, ids0 = case["val"], case["ids0"]
    cum[0] = [0.0, 0.0, -0.25, 0.0]
    val[0:4] = [-0.5, -1.0, -1.5, -2.0]
    cum[1] = [0.0, -5.0, -5.0, -5.0]
    val[4:8] = -0.5
    cum[2] = [-0.25, 0.0, 0.0, -np.inf]
    val[8] = [0.0, 0.0, -1.0, -1.0]
    val[9] = [-0.25, -0.25, -0.5, -0.5]
    val[10] = [-0.25, -0.5, -0.5, -0.75]
    (g_seq, g_hep, g_cum, g_paths), g_st = _beam_check(_engine(L), case, exact_cum=True)
    item = lambda row, rank: float(ids0[row, rank] + 1)
    assert list(g_paths[0, :, step]) == [item(0, 0), item(1, 0), item(3, 0), item(2, 0)]
    assert list(g_cum[0]) == [-0.5, -0.5, -0.5, -0.75]
    assert list(g_paths[1, :, step]) == [item(4, 0), item(4, 1), item(4, 2), item(4, 3)] and (g_cum[1] == -0.5).all()
    assert list(g_paths[2, :, step]) == [item(8, 0), item(8, 1), item(9, 0), item(9, 1)] and (g_cum[2] == -0.25).all()
    for t in range(W):  # the rest of the state follows the parent
        assert np.array_equal(g_paths[0, t, :step], paths[0, [0, 1, 3, 2][t], :step])
        assert np.array_equal(g_paths[2, t, :step], paths[2, [0, 0, 1, 1][t], :step])


@pytest.mark.parametrize("W,k,L", [(4, 65, 65), (4, 100, 256), (17, 65, 256), (17, 100, 65), (32, 100, 200), (1, 65, 65)])
def test_beam_step_second_round_of_candidates(W, k, L):
    """Every beam's first 64 candidates are in its window (L > 64): survivors come from the second round of 64."""
    case = _beam_case(3, W, k, L, 5, 2, seed=W + k + L, force_c=64, holes=False, dead_frac=(0.2 if W > 1 else 0.0))
    (g_seq, g_hep, g_cum, g_paths), g_st = _beam_check(_engine(L), case, exact_cum=(W == 1))
    assert np.isfinite(g_cum).any() and not (g_st & NO_CAND).any()
    seq, hep, _, _ = case["state"]
    for row in range(3 * W):  # the inputs are what the test is named after
        b, j = divmod(row, W)
        assert hep[b, j] + 1 >= 64 and np.isin(case["ids0"][row, :64] + 1, seq[b, j, :hep[b, j] + 1]).all()


def test_beam_step_fewer_than_w_candidates_and_dead_beams():
    """W = 5, k = 3: two live beams between dead ones, one of them cut short by a -1: four candidates in all.  The
    trailing output beams are dead: cum -inf, a zero path, window and hep of input beam 0 (itself dead here)."""
    B, W, k, L, P, step = 2, 5, 3, 10, 5, 2
    case = _beam_case(B, W, k, L, P, step, seed=5, dead_frac=0.0, holes=False, force_c=0)
    seq, hep, cum, paths = case["state"]
    cum[:, [0, 2, 4]] = -np.inf
    case["ids0"][np.arange(B) * W + 3, 1] = -1
    case["ids0"] = case["ids0"].copy()
    (g_seq, g_hep, g_cum, g_paths), g_st = _beam_check(_engine(L), case, exact_cum=False)
    assert np.isfinite(g_cum[:, :4]).all() and np.isneginf(g_cum[:, 4:]).all()
    assert not g_paths[:, 4:].any()
    assert np.array_equal(g_seq[:, 4], seq[:, 0]) and np.array_equal(g_hep[:, 4], hep[:, 0])
    assert not (g_st & NO_CAND).any()
    assert set(g_paths[0, :4, step].astype(np.int64)) == set(case["ids0"][[1, 1, 1, 3], [0, 1, 2, 0]] + 1)


def test_beam_step_status_bit():
    """B = 3.  User 0: every live beam has survivors, the bit stays clear.  User 1: no live beam has a survivor: the bit
    is set and every output beam is dead.  User 2: one live beam of three has no survivor: the bit is set although the
    user keeps W live beams (the bit means `some live beam of this user ran out`).  A dead beam without survivors sets
    nothing (user 0's beam 1)."""
    B, W, k, L, P, step = 3, 4, 3, 10, 5, 1
    case = _beam_case(B, W, k, L, P, step, seed=9, dead_frac=0.0, holes=False, force_c=0)
    seq, hep, cum, paths = case["state"]
    hep[:] = 4

    def swallow(b, j):
        seq[b, j, :3] = case["ids0"][b * W + j] + 1
    cum[0, 1] = -np.inf
    swallow(0, 1)
    for j in range(W):
        swallow(1, j)
    swallow(2, 2)
    case["status"] = np.array([4, 1, 0], dtype=np.int32)
    (g_seq, g_hep, g_cum, g_paths), g_st = _beam_check(_engine(L), case, exact_cum=False)
    assert list(g_st) == [4, 1 | NO_CAND, NO_CAND]
    assert np.isfinite(g_cum[0]).all() and np.isneginf(g_cum[1]).all() and np.isfinite(g_cum[2]).all()
    assert not g_paths[1].any() and np.array_equal(g_seq[1], np.repeat(seq[1, :1], W, axis=0))


@pytest.mark.parametrize("L,B,k", [(3, 5, 3), (10, 67, 100), (65, 4, 65), (256, 3, 64)])
def test_beam_w1_equals_path_step(L, B, k):
    """W == 1 without the log-sum-exp is the greedy step on the same inputs: path entry, window and hep, for rows that
    have a candidate.  The exhausted rows differ as documented: greedy keeps the path prefix and writes 0 at the step,
    the beam step leaves a dead beam (an all-zero path, cum -inf); the window, hep and the status bit agree."""
    eng = _engine(L)
    seq, hep, val, ids0, status, info = _greedy_case(L, B, k, seed=L + B + k)
    step, P = 2, 5
    paths = np.full((B, P), 12345.0, dtype=np.float32)
    paths[:, :step] = np.arange(1, 1 + B * step, dtype=np.float32).reshape(B, step)
    p_seq, p_hep, p_paths, p_st = _run_path_step(eng, seq, hep, val, ids0, step, paths, status)
    cum = -np.arange(B, dtype=np.float64)[:, None]
    case = dict(state=(seq[:, None].copy(), hep[:, None].copy(), cum, paths[:, None].copy()), val=val, ids0=ids0,
                lse=(None, None), status=status, step=step, P=P)
    (g_seq, g_hep, g_cum, g_paths), g_st = _beam_check(eng, case, exact_cum=True)
    ok = (p_st & NO_CAND) == 0
    assert np.array_equal(g_st, p_st)
    assert np.array_equal(g_seq[:, 0], p_seq) and np.array_equal(g_hep[:, 0], p_hep)
    assert np.array_equal(g_paths[ok, 0, :step + 1], p_paths[ok, :step + 1])
    first = val[np.arange(B), [min(c, k - 1) for _, _, c in info]].astype(np.float64)  # the first survivor's score
    assert np.array_equal(g_cum[ok, 0], cum[ok, 0] + first[ok])
    if (~ok).any():  # the exhausted rows
        assert np.array_equal(p_paths[~ok, :step], paths[~ok, :step]) and not p_paths[~ok, step].any()
        assert not g_paths[~ok, 0].any() and np.isneginf(g_cum[~ok, 0]).all()
    assert B < 20 or ((~ok).any() and ok.any())


def test_beam_step_argument_contract():
    L, B, W, k, P = 10, 2, 3, 5, 4
    eng = _engine(L)
    case = _beam_case(B, W, k, L, P, 1, seed=3)
    d_in = [_t(a) for a in case["state"]]
    d_out = [torch.full_like(t, 9) for t in d_in]
    d_val, d_ids, d_st = _t(case["val"]), _t(case["ids0"]), _t(case["status"])
    lmax, lsum = (_t(a) for a in case["lse"])

    def call(W_=W, step=1, P_=P, lm=lmax, ls=lsum, k_=k):
        rc = eng.lib.irs_beam_step(eng.h, *(_ptr(t) for t in d_in), _ptr(d_val), _ptr(d_ids), _ptr(lm), _ptr(ls), B, W_, k_,
                                   step, P_, *(_ptr(t) for t in d_out), _ptr(d_st), _stream())
        torch.cuda.synchronize()
        return rc
    assert call(W_=0) == E_INVALID
    assert call(W_=33) == E_UNSUPPORTED
    assert call(step=P) == E_INVALID and call(step=P + 3) == E_INVALID and call(step=-1) == E_INVALID
    assert call(lm=None) == E_INVALID and call(ls=None) == E_INVALID and call(lm=None, ls=None) == E_INVALID
    assert call(k_=0) == E_INVALID
    for t in d_out:
        assert (_n(t) == 9).all()
    assert np.array_equal(_n(d_st), case["status"])
    assert call() == 0


# --------------------------------------------------------------------------------------------- pack and merge
def _lists(g, W, M, k):
    """Scores from a small set (equal scores meet across shards with different ids) with +-0, +-inf, subnormals and
    negative values; ids up to 2^31 - 1; -1 holes anywhere; all-empty rows."""
    pool = np.array([0.0, -0.0, 1.5, -1.5, 1e-42, -1e-42, np.inf, -np.inf, 3.25, 2.0 ** -126, -7.0, 1.5000001],
                    dtype=np.float32)
    val = pool[g.integers(0, len(pool), size=(W, M, k))]
    ids = g.integers(0, 2 ** 31, size=(W, M, k)).astype(np.int64)
    ids[:, :, 0] = np.arange(W)[:, None]
    ids[0, :, k - 1] = 2 ** 31 - 1
    ids[g.random((W, M, k)) < 0.2] = -1
    if M > 1:
        ids[:, M // 2] = -1  # an all-empty row
    if M > 2:
        ids[1:, 1] = -1  # a row fed by one shard only
    return val, ids


@pytest.mark.parametrize("M", [1, 5, 300])
@pytest.mark.parametrize("W,k", [(1, 1), (2, 100), (3, 100), (7, 37), (8, 100), (20, 100), (16, 128)])
def test_pack_and_merge_bit_exact(W, k, M):
    eng = _engine(10)
    val, ids = _lists(np.random.default_rng(W * 1000 + k * 7 + M), W, M, k)
    keys = eng.pack_topk(_t(val), _t(ids))
    assert np.array_equal(_n(keys).view(np.uint64), path_ref.pack_keys(val, ids))
    w_val, w_ids = path_ref.merge(val, ids, k)
    a_val, a_ids = eng.merge_topk(_t(val), _t(ids))
    b_val, b_ids = eng.merge_topk_keys(keys)
    torch.cuda.synchronize()
    for g_val, g_ids in ((a_val, a_ids), (b_val, b_ids)):
        assert np.array_equal(_n(g_ids), w_ids), np.argwhere(_n(g_ids) != w_ids)[:8]
        assert np.array_equal(_n(g_val).view(np.uint32), w_val.view(np.uint32))
    assert torch.equal(a_ids, b_ids) and torch.equal(a_val.view(torch.int32), b_val.view(torch.int32))
    assert M == 1 or (w_ids[M // 2] == -1).all()


def test_merge_rejects_more_than_2048_entries():
    eng = _engine(10)
    W, M, k = 17, 2, 128
    val, ids = _lists(np.random.default_rng(0), W, M, k)
    d_val, d_ids = _t(val), _t(ids)
    keys = eng.pack_topk(d_val, d_ids)
    o_val = torch.full((M, k), 9.0, dtype=torch.float32, device=DEV)
    o_ids = torch.full((M, k), 9, dtype=torch.int64, device=DEV)
    for W_, k_ in ((17, 128), (21, 100), (2049, 1)):
        assert eng.lib.irs_merge_topk(eng.h, _ptr(d_val), _ptr(d_ids), W_, M, k_, _ptr(o_val), _ptr(o_ids), _stream()) == E_UNSUPPORTED
        assert eng.lib.irs_merge_topk_keys(eng.h, _ptr(keys), W_, M, k_, _ptr(o_val), _ptr(o_ids), _stream()) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (_n(o_val) == 9.0).all() and (_n(o_ids) == 9).all()


# --------------------------------------------------------------------------------------------- evaluation batch
def _eval_call(eng, items, offsets, raw_len, gap_len, *, targets=None, pool=None, seed=0, status=None):
    """irs_build_eval_batch with a caller-owned status (Engine.build_eval_batch always starts from zeros)."""
    B = len(offsets) - 1
    d_items = _t(items if len(items) else np.zeros(1, dtype=np.int64))
    d_off, d_tg, d_pool = _t(offsets), (None if targets is None else _t(targets)), (None if pool is None else _t(pool))
    seq = torch.full((B, eng.L), -5, dtype=torch.int64, device=DEV)
    tgt = torch.full((B,), -5, dtype=torch.int64, device=DEV)
    lab = torch.full((B,), -5, dtype=torch.int64, device=DEV)
    raw = torch.full((B, raw_len), -5, dtype=torch.int64, device=DEV)
    raw_n = torch.full((B,), -5, dtype=torch.int32, device=DEV)
    st = _t(np.zeros(B, dtype=np.int32) if status is None else status)
    rc = eng.lib.irs_build_eval_batch(eng.h, _ptr(d_items), _ptr(d_off), B, raw_len, gap_len, _ptr(d_tg), _ptr(d_pool),
                                      0 if pool is None else len(pool), seed, _ptr(seq), _ptr(tgt), _ptr(lab), _ptr(raw),
                                      _ptr(raw_n), _ptr(st), _stream())
    torch.cuda.synchronize()
    return rc, tuple(_n(t) for t in (seq, tgt, lab, raw, raw_n, st))


def _eval_users(g, counts, n_item):
    hists = [g.permutation(n_item)[:c].astype(np.int64) + 1 for c in counts]
    items = np.concatenate(hists) if sum(counts) else np.zeros(0, dtype=np.int64)
    return hists, items, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


@pytest.mark.parametrize("gap_name", ["0", "3", "L-2"])
@pytest.mark.parametrize("raw_rel", ["smaller", "equal", "larger"])
@pytest.mark.parametrize("L", [12, 70])
def test_eval_batch_exact_and_drawn_targets(L, raw_rel, gap_name):
    """Users with 0, 1, 2, raw_len - 1, raw_len and raw_len + 50 events (a user with no event comes first and last, so
    that an empty range sits at both ends of `items`).  raw_len smaller than, equal to and larger than the
    L - gap_len - 1 history slots; where only one slot is left (gap_len = L - 2) `smaller` cannot be, and raw_len = 1
    stands in."""
    n_item = 500
    eng = _engine(L, n_item)
    gap = {"0": 0, "3": 3, "L-2": L - 2}[gap_name]
    slots = L - gap - 1
    raw_len = {"smaller": max(1, slots - 2), "equal": slots, "larger": slots + 7}[raw_rel]
    g = np.random.default_rng(L * 100 + raw_len * 10 + gap)
    counts = [0, 1, 2, max(0, raw_len - 1), raw_len, raw_len + 50, 3, 0]
    hists, items, offsets = _eval_users(g, counts, n_item)
    B = len(counts)
    given = g.integers(1, n_item + 1, size=B).astype(np.int64)
    w_seq, w_lab, w_raw, w_n = path_ref.build_eval_batch(items, offsets, L, raw_len, gap, given)
    rc, (seq, tgt, lab, raw, raw_n, st) = _eval_call(eng, items, offsets, raw_len, gap, targets=given)
    assert rc == 0
    assert np.array_equal(seq, w_seq) and np.array_equal(tgt, given) and np.array_equal(lab, w_lab)
    assert np.array_equal(raw, w_raw) and np.array_equal(raw_n, w_n) and not st.any()
    # drawn targets: over the catalog, then over a pool
    pool = np.arange(40, 80, dtype=np.int64)
    for pl in (None, pool):
        rc, (seq, tgt, lab, raw, raw_n, st) = _eval_call(eng, items, offsets, raw_len, gap, pool=pl, seed=5)
        assert rc == 0 and not st.any()
        assert np.array_equal(seq[:, :-1], w_seq[:, :-1]) and np.array_equal(seq[:, -1], tgt)
        assert np.array_equal(lab, w_lab) and np.array_equal(raw, w_raw) and np.array_equal(raw_n, w_n)
        assert (np.isin(tgt, pool) if pl is not None else (tgt >= 1) & (tgt <= n_item)).all()
        for b in range(B):
            assert tgt[b] not in set(w_raw[b, raw_len - w_n[b]:].tolist())
        again = _eval_call(eng, items, offsets, raw_len, gap, pool=pl, seed=5)[1]
        assert np.array_equal(again[1], tgt) and np.array_equal(again[0], seq)
    assert _eval_call(eng, items, offsets, raw_len, L - 1, targets=given)[0] == E_UNSUPPORTED


def test_eval_batch_pool_inside_the_window():
    """The pool (and, for the last user, the whole catalog) is contained in the raw window: no target exists.
    NO_CANDIDATE is OR-ed into the caller's status, the target is 0; the other users draw as usual."""
    L, n_item = 12, 64
    eng = _engine(L, n_item)
    g = np.random.default_rng(1)
    pool = np.array([3, 9, 27, 50], dtype=np.int64)
    h0 = np.concatenate([g.permutation(np.setdiff1d(np.arange(1, 65), pool))[:20], pool, [1]])   # window holds the pool
    h1 = np.concatenate([np.setdiff1d(np.arange(1, 65), pool)[:30], [2]])                          # window misses the pool
    h2 = np.concatenate([pool[:3], [60, 61, 5]])                                                   # one pool item is left
    hists = [h0, h1, h2]
    items = np.concatenate(hists).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int64)
    pre = np.array([5, 1, 4], dtype=np.int32)
    rc, (seq, tgt, lab, raw, raw_n, st) = _eval_call(eng, items, offsets, 100, 0, pool=pool, seed=3, status=pre)
    assert rc == 0 and list(st) == [5 | NO_CAND, 1, 4]
    assert tgt[0] == 0 and seq[0, -1] == 0 and tgt[1] in pool and tgt[2] == 50
    full = np.concatenate([g.permutation(64) + 1, [7]]).astype(np.int64)                            # the whole catalog
    rc, (seq, tgt, lab, raw, raw_n, st) = _eval_call(eng, full, np.array([0, 65], dtype=np.int64), 100, 0, seed=3,
                                                     status=np.array([1], dtype=np.int32))
    assert rc == 0 and list(st) == [1 | NO_CAND] and tgt[0] == 0 and lab[0] == 7 and raw_n[0] == 64


def test_eval_batch_draw_is_uniform():
    """One user's history copied B = 65536 times; half of the 64-item catalog is in its window.  Every allowed item is
    drawn B / 32 times within the binomial bound of the module docstring (p = 1 / 32); a forbidden item never."""
    L, n_item, B = 12, 64, 65536
    eng = _engine(L, n_item)
    g = np.random.default_rng(2)
    perm = g.permutation(64) + 1
    window, allowed = perm[:32], np.sort(perm[32:])
    hist = np.concatenate([window, [allowed[0]]]).astype(np.int64)  # the label is not part of the window
    items = np.tile(hist, B)
    offsets = np.arange(B + 1, dtype=np.int64) * len(hist)
    rc, (seq, tgt, lab, raw, raw_n, st) = _eval_call(eng, items, offsets, 100, 0, seed=77)
    assert rc == 0 and not st.any() and (raw_n == 32).all()
    assert np.isin(tgt, allowed).all() and not np.isin(tgt, window).any()
    counts = np.bincount(tgt, minlength=65)
    p = 1.0 / 32
    bound = _sigma6(B, p)  # 6 sqrt(n p (1 - p)) + 1
    print("eval draw counts", counts[allowed].min(), counts[allowed].max(), "expected", B * p, "bound", bound)
    assert (np.abs(counts[allowed] - B * p) <= bound).all()


# --------------------------------------------------------------------------------------------- the loop against its parts
@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("gap_len", [0, 3])
@pytest.mark.parametrize("B", [3, 67])
def test_generate_paths_equals_its_parts(B, gap_len, sample):
    """irs_generate_paths (stream launches and the captured graph; at B = 3 the merged one-launch route) against the
    same search done by hand through the ABI: decode(pos = hep), score_topk, path_step."""
    cfg = synth.make_config("tiny")
    sd = synth.irn_state_dict(cfg, 1234)
    eng = make_engine(cfg, sd, max_rows=B, max_seqs=B)
    hists = synth.user_histories(max(B, 8), cfg.n_item, seed=7)
    rows = synth.eval_rows(hists, cfg.n_item, seed=11)[:B]
    _, seqs, users, _, _ = synth.collate_eval_irs(rows, cfg.max_len, gap_len=gap_len)
    L, P, k = cfg.max_len, 6, 100
    kw = dict(sample=sample, sample_k=3, seed=99)
    d_users = _t(users)
    seq, hep = _t(seqs), torch.full((B,), L - gap_len - 2, dtype=torch.int32, device=DEV)
    paths = torch.zeros((B, P), dtype=torch.float32, device=DEV)
    status = torch.zeros(B, dtype=torch.int32, device=DEV)
    for step in range(P):
        _, xr, _ = eng.decode(seq, d_users, want_x=False, pos=hep)
        val, ids0, _ = eng.score_topk(xr, k, IRS_SWEEP_BF16)
        eng.path_step(seq, hep, val, ids0, step, paths, status, **kw)
    torch.cuda.synchronize()
    assert (_n(paths) > 0).all() and not _n(status).any()
    for use_graph in (False, True):
        seq2, hep2 = _t(seqs), torch.full((B,), L - gap_len - 2, dtype=torch.int32, device=DEV)
        paths2, status2 = eng.generate_paths(seq2, d_users, hep2, P, k=k, sweep=IRS_SWEEP_BF16, use_graph=use_graph, **kw)
        torch.cuda.synchronize()
        assert torch.equal(paths2, paths), (use_graph, np.argwhere(_n(paths2) != _n(paths))[:8])
        assert torch.equal(seq2, seq) and torch.equal(hep2, hep) and torch.equal(status2, status)
