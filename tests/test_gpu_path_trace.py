"""-m gpu: the path trace (include/irs_hip.h, "path trace"): irs_score_target_trace alone, the greedy / sampled loops with a
bound trace against the step-by-step composition of the public calls, the until loop against the plain loop, the refusals, and
IRSNN.get_seq_in_batch(trace=True).

Bounds.  Bit for bit wherever both sides run the same launches on the same bytes.  Where they do not (the until loop decodes a
compacted batch; forward() decodes whole windows), both decoder rows are within the project's decoder tolerance of 2e-5 per
element of the truth, so a logit moves by at most LOGIT = 4e-5 * max_j ||W_j||_1, a log-probability by at most twice that plus
the log-sum-exp bound of test_gpu_scoring.py, 4e-6 * max(1, max |lse|), and a rank may differ only where the target stands
closer than LOGIT to a neighbour in the dense logits."""
import ctypes

import numpy as np
import pytest
import torch

import path_ref
import path_trace_ref as ref
from gpu_util import make_engine, scoring_only_engine
from influentialrs_amd import _lib, synth
from influentialrs_amd._lib import IRS_SWEEP_BF16
from influentialrs_amd.engine import IrsError
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
from long_window_cases import BY_ID

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# of the tiny golden: users 2, 6, 10, 11 arrive at steps 3, 3, 2, 7.  Chosen on the CPU oracle's logits so that the gap rule of
# the until test excuses nobody: over their 8 steps the target's nearest neighbour is 1.5e-4 away or more (the logit bound is
# 1.1e-4); users 1, 5 and 9 each have a step with a neighbour within 2e-5 and are left out.
USERS6 = [0, 2, 3, 6, 10, 11]
P8 = 8


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


# ============================================================================ 1. the sweep alone
# (n_item, d, M).  n_item not a multiple of 32, d = 30 not a multiple of 8, M = 33 and 70 cross a 32-row tile.  The sweep is cut
# by launch_sweep_f32's decomposition: tiles = ceil(n_item / 32), tiles per wave = ceil(tiles / 1024), strips =
# ceil(tiles / (4 tiles per wave)), one workgroup per (strip, row block).  (4099, 128, 70): 129 tiles, 1 per wave, 33 strips, so 33
# workgroups and 129 waves contribute to every row; (40003, 32, 9): 1251 tiles, 2 per wave, 157 strips.
SWEEP_SHAPES = [(257, 16, 5), (3415, 30, 33), (4099, 128, 70), (1031, 256, 37), (40003, 32, 9)]
L4 = 4  # scoring_only_engine's max_len: a window of at most three entries and the target


def _strips(n_item):
    tiles = (n_item + 31) // 32
    tpw = (tiles + 1023) // 1024
    return (tiles + 4 * tpw - 1) // (4 * tpw)


@pytest.mark.parametrize("n_item,d,M", SWEEP_SHAPES)
def test_sweep_alone(n_item, d, M):
    assert _strips(n_item) >= 2
    rng = np.random.default_rng(n_item + d)
    W = (rng.standard_normal((n_item, d)) * 0.3).astype(np.float32)
    b = (rng.standard_normal(n_item) * 0.1).astype(np.float32)
    T0 = n_item // 2  # 0-based id of the tied target; its twins sit below and above it
    lo, hi = T0 - 5, T0 + 7
    W[lo], W[hi], b[lo], b[hi] = W[T0], W[T0], b[T0], b[T0]
    eng = scoring_only_engine(n_item, d, W, b, max_rows=max(M, 64))
    x = _t(rng.standard_normal((M, d)).astype(np.float32))
    logits = _n(eng.score_dense(x))
    seq = np.zeros((M, L4), dtype=np.int64)
    hep = np.full(M, L4 - 2, dtype=np.int32)
    for m in range(M):
        order = np.argsort(-logits[m].astype(np.float64), kind="stable")
        t0 = T0 if m % 3 == 0 else int(rng.integers(0, n_item))  # kinds 0 and 3 below: the tied target
        pos = int(np.where(order == t0)[0][0])
        above = [int(v) + 1 for v in order[:pos] if v not in (lo, hi, T0)]  # items ranked before the target
        below = [int(v) + 1 for v in order[pos + 1:] if v not in (lo, hi, T0)]
        a = above[len(above) // 2] if above else below[0]
        c = above[0] if above else below[1]
        bl = below[len(below) // 2] if below else above[-1]
        kind = m % 6
        if kind == 0:
            seq[m, :3] = (0, a, a)  # a leading pad, a duplicate ranked before the target
        elif kind == 1:
            seq[m, :3] = (a, bl, c)  # before, after, before
        elif kind == 2:
            seq[m, :3] = (0, 0, t0 + 1)  # the target in its own window
        elif kind == 3:
            seq[m, :3] = (lo + 1, bl, bl)  # one of the tied twins hidden (it ranks before the tied target), a duplicate behind
        elif kind == 4:
            seq[m, :3] = (bl, a, c)
            hep[m] = 0  # only slot 0 is window: the two items ranked before the target behind it still count
        else:
            seq[m, :3] = (a, c, t0 + 1)
            hep[m] = L4 - 1  # the window reaches over the target's own slot
        seq[m, L4 - 1] = t0 + 1
    if M > 4:
        seq[4, L4 - 1] = 0  # a row without a target
    out = [_n(v) for v in eng.score_target_trace(x, _t(seq), _t(hep))]
    again = [_n(v) for v in eng.score_target_trace(x, _t(seq), _t(hep))]
    assert _same_bits(out, again)
    mx, sm, ts, rank = out
    assert rank.dtype == np.int32 and ts.dtype == np.float32
    gat = _n(eng.score_gather(x, _t(seq[:, L4 - 1:] - 1)))[:, 0]
    assert np.array_equal(ts.view(np.uint32), gat.view(np.uint32))
    want = np.array([ref.target_rank(logits[m], seq[m, :hep[m] + 1], seq[m, L4 - 1]) for m in range(M)], dtype=np.int32)
    assert np.array_equal(rank, want), np.where(rank != want)
    want_lse = torch.logsumexp(torch.from_numpy(logits).double(), dim=1).numpy()
    got_lse = mx.astype(np.float64) + np.log(sm.astype(np.float64))
    assert np.abs(got_lse - want_lse).max() <= 4e-6 * max(1.0, np.abs(want_lse).max())
    # the engineered cases did happen: ties counted on the low side only, hidden items ranked before the target
    assert all(rank[m] >= 2 for m in range(0, M, 6)) and (M <= 4 or (rank[4] == 0 and ts[4] == -np.inf))
    for m in range(3, M, 6):  # the low twin hidden, the high twin behind the target by id: nobody ties in front
        assert rank[m] == 1 + int((logits[m].astype(np.float64) > float(logits[m, T0])).sum()) - int(logits[m, seq[m, 1] - 1] > logits[m, T0])
    plain = np.array([ref.target_rank(logits[m], [], seq[m, L4 - 1]) for m in range(M)])
    assert (plain > want).any()


# ============================================================================ 2. a long window
def test_sweep_long_window():
    case = BY_ID["tiny_L1024_b3"]  # the tiny model, the longest window
    cfg = case.config()
    L, N = cfg.max_len, cfg.n_item
    assert L > 256
    eng = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=8, max_seqs=8)
    rng = np.random.default_rng(5)
    M = 5
    seq = rng.integers(1, N + 1, (M, L)).astype(np.int64)  # up to 1023 entries out of 257 items: duplicates are certain
    seq[:, :7] = 0
    seq[1, :200] = 0
    hep = np.array([L - 2, L - 2, 100, 600, 300], dtype=np.int32)
    usr = _t(np.arange(M, dtype=np.int64))
    _, x, _ = eng.decode(_t(seq), usr, want_x=False, pos=_t(hep))
    logits = _n(eng.score_dense(x))
    mx, sm, ts, rank = (_n(v) for v in eng.score_target_trace(x, _t(seq), _t(hep)))
    assert (hep + 1 > 256).sum() >= 3
    want = np.array([ref.target_rank(logits[m], seq[m, :hep[m] + 1], seq[m, L - 1]) for m in range(M)], dtype=np.int32)
    assert np.array_equal(rank, want)
    assert len(set(want.tolist())) > 1 and (want < np.array([ref.target_rank(logits[m], [], seq[m, L - 1]) for m in range(M)])).any()
    assert np.array_equal(ts.view(np.uint32), _n(eng.score_gather(x, _t(seq[:, L - 1:] - 1)))[:, 0].view(np.uint32))
    want_lse = torch.logsumexp(torch.from_numpy(logits).double(), dim=1).numpy()
    assert np.abs(mx.astype(np.float64) + np.log(sm.astype(np.float64)) - want_lse).max() <= 4e-6 * max(1.0, np.abs(want_lse).max())


# ============================================================================ 3. the loop against the composition
_ENG = {}


def _engine(cfgname, rows):
    key = (cfgname, rows)
    if key not in _ENG:
        _ENG.clear()  # one catalog resident at a time
        cfg = synth.make_config(cfgname)
        _ENG[key] = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=rows, max_seqs=rows)
    return _ENG[key]


def _inputs(g, src):
    src = np.asarray(src)
    seq = g["seqs"][src]
    return seq, g["users"][src], np.full(len(src), seq.shape[1] - 2, dtype=np.int32)  # the goldens' gap_len is 0


def _loop(eng, seq, usr, hep, P, **kw):
    paths, status, tr = eng.generate_paths(_t(seq), _t(usr), _t(hep), P, k=100, sweep=IRS_SWEEP_BF16, trace=True, **kw)
    return _n(paths), _n(status), tuple(_n(a) for a in tr)


def _composition(eng, seq, usr, hep, P, sample=False, sample_k=3, seed=0):
    """decode at hep, the sweep, top-100, the path step, through the public calls; lp_item from the lists in numpy."""
    B = len(seq)
    seq, usr, hep = _t(seq), _t(usr), _t(hep)
    paths = torch.zeros((B, P), dtype=torch.float32, device=DEV)
    status = torch.zeros(B, dtype=torch.int32, device=DEV)
    lp_item, lp_target = np.zeros((B, P), dtype=np.float32), np.zeros((B, P), dtype=np.float32)
    rank = np.zeros((B, P), dtype=np.int32)
    for i in range(P):
        _, xr, _ = eng.decode(seq, usr, want_x=False, pos=hep)
        mx, sm, ts, rk = (_n(v) for v in eng.score_target_trace(xr, seq, hep))
        val, ids, _ = eng.score_topk(xr, 100, IRS_SWEEP_BF16, carry=i > 0)
        eng.path_step(seq, hep, val, ids, i, paths, status, sample, sample_k, seed)
        val, ids, chosen = _n(val), _n(ids), _n(paths)[:, i]
        lse = mx.astype(np.float64) + np.log(sm.astype(np.float64))
        for b in range(B):
            lp_target[b, i] = np.float32(np.float64(ts[b]) - lse[b])
            at = np.where(ids[b] == int(chosen[b]) - 1)[0]
            assert chosen[b] != 0 and len(at) == 1
            lp_item[b, i] = np.float32(np.float64(val[b, at[0]]) - lse[b])
        rank[:, i] = rk
    return _n(paths), _n(status), (lp_item, lp_target, rank)


@pytest.mark.parametrize("sample", [False, True])
def test_loop_equals_composition_and_graph_equals_stream(golden, sample):
    g = golden("irn_tiny")
    eng = _engine("tiny", 128)
    seq, usr, hep = _inputs(g, USERS6)
    kw = dict(sample=sample, sample_k=3, seed=4711)
    got = _loop(eng, seq, usr, hep, P8, **kw)
    want = _composition(eng, seq, usr, hep, P8, **kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert _same_bits(got[2], want[2])
    assert got[2][0].dtype == np.float32 and got[2][2].dtype == np.int32
    assert (got[2][0] < 0).all() and (got[2][1] < 0).all() and (got[2][2] >= 1).all()
    graph = _loop(eng, seq, usr, hep, P8, use_graph=True, **kw)
    assert np.array_equal(graph[0], got[0]) and _same_bits(graph[2], got[2])
    if not sample:  # the trace changes nothing the search returns
        plain = eng.generate_paths(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16)
        assert np.array_equal(_n(plain[0]), got[0]) and np.array_equal(_n(plain[1]), got[1])


def test_loop_above_the_small_plan_switch(golden):
    g = golden("irn_tiny")
    eng = _engine("tiny", 128)
    src = np.arange(70) % 12  # 70 rows: beyond the 64 of the single-workgroup plan
    seq, usr, hep = _inputs(g, src)
    got = _loop(eng, seq, usr, hep, 4)
    want = _composition(eng, seq, usr, hep, 4)
    assert np.array_equal(got[0], want[0]) and _same_bits(got[2], want[2])
    assert _same_bits([a[12:24] for a in got[2]], [a[:12] for a in got[2]])  # equal users, equal traces


def test_loop_behind_the_sequence_resident_decode(golden):
    g = golden("irn_c2")
    B = 384
    eng = _engine("c2", B)
    seq, usr, hep = _inputs(g, np.arange(B) % g["seqs"].shape[0])
    got = _loop(eng, seq, usr, hep, 3)
    assert eng.decoder_seq_last
    want = _composition(eng, seq, usr, hep, 3)
    assert eng.decoder_seq_last
    assert np.array_equal(got[0], want[0]) and _same_bits(got[2], want[2])
    assert (got[2][2] >= 1).all() and (got[2][1] < 0).all()


# ============================================================================ 4. the until loop
def _bounds(sd, lse_abs):
    logit = 4e-5 * float(np.abs(sd["project.weight"]).sum(axis=1).max())
    return logit, 2 * logit + 4e-6 * max(1.0, lse_abs)


def _walk_logits(eng, seq, usr, hep, paths, n_steps):
    """The dense logits and the window of every live (user, step): windows rebuilt from the paths with path_ref.advance."""
    B, P = paths.shape
    win, he = [np.array(r) for r in seq], [int(h) for h in hep]
    logits, windows = {}, {}
    for i in range(P):
        _, xr, _ = eng.decode(_t(np.stack(win)), _t(usr), want_x=False, pos=_t(np.array(he, dtype=np.int32)))
        lg = _n(eng.score_dense(xr))
        for b in range(B):
            if i < n_steps[b]:
                logits[b, i], windows[b, i] = lg[b], win[b][:he[b] + 1].copy()
                win[b], he[b] = path_ref.advance(win[b], he[b], int(paths[b, i]))
    return logits, windows


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


def _check_against_plain(eng, sd, seq, usr, hep, targets, plain, got_paths, got_tr):
    """The until loop's (or the front end's) arrays against the plain loop's after the host cut: the module docstring's rule."""
    n, want = _cut(plain[0], targets, plain[2])
    assert np.array_equal(got_paths, _cut(plain[0], targets, [plain[0]])[1][0])
    logits, windows = _walk_logits(eng, seq, usr, hep, plain[0], n)
    lse_abs = max(abs(ref.lse64(v)) for v in logits.values())
    LOGIT, LP = _bounds(sd, lse_abs)
    live = excused = cpu_excused = 0
    for b in range(len(seq)):
        for a in got_tr:
            assert not a[b, n[b]:].any(), "exactly zero behind the arrival"
        for i in range(n[b]):
            live += 1
            print(f"user {b} step {i}: dlp_item {abs(float(got_tr[0][b, i]) - float(want[0][b, i])):.3g} "
                  f"dlp_target {abs(float(got_tr[1][b, i]) - float(want[1][b, i])):.3g} bound {LP:.3g} "
                  f"rank {got_tr[2][b, i]} / {want[2][b, i]}")
            assert abs(float(got_tr[0][b, i]) - float(want[0][b, i])) <= LP
            assert abs(float(got_tr[1][b, i]) - float(want[1][b, i])) <= LP
            lg, t0 = logits[b, i].astype(np.float64), int(targets[b]) - 1
            others = np.delete(lg, t0)
            close = np.abs(others - lg[t0]).min() <= LOGIT
            cpu_excused += close
            assert want[2][b, i] == ref.target_rank(logits[b, i], windows[b, i], targets[b])
            if got_tr[2][b, i] != want[2][b, i]:
                assert close
                excused += 1
    assert excused <= 0.05 * live and cpu_excused == 0
    return n


@pytest.mark.parametrize("check_every", [1, 3])
def test_until_loop(golden, check_every):
    g = golden("irn_tiny")
    cfg = synth.make_config("tiny")
    sd = synth.irn_state_dict(cfg, 1234)
    eng = _engine("tiny", 128)
    seq, usr, hep = _inputs(g, USERS6)
    targets = seq[:, -1].copy()
    plain = _loop(eng, seq, usr, hep, P8)

    def until(s):
        paths, status, steps, row_steps, tr = eng.generate_paths_until(_t(s), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16,
                                                                       check_every=check_every, trace=True)
        return _n(paths), _n(status), steps, row_steps, tuple(_n(a) for a in tr)

    # targets that never arrive: item 1 is in nobody's path.  Nothing is compacted: the same launches on the same bytes
    far = seq.copy()
    far[:, -1] = 1
    want = _loop(eng, far, usr, hep, P8)
    assert not (want[0] == 1).any()
    got = until(far)
    assert np.array_equal(got[0], want[0]) and _same_bits(got[4], want[2]) and got[2:4] == (P8, 6 * P8)
    # arrivals
    got = until(seq)
    assert got[3] < 6 * P8
    n = _check_against_plain(eng, sd, seq, usr, hep, targets, plain, got[0], got[4])
    assert sorted(n.tolist()) == [3, 4, 4, 8, 8, 8]


# ============================================================================ 5. refusals
def test_refusals_and_unbinding(golden):
    g = golden("irn_tiny")
    eng = _engine("tiny", 128)
    lib = eng.lib
    seq, usr, hep = _inputs(g, USERS6)
    never_bound = eng.generate_paths(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16)
    never_bound = (_n(never_bound[0]), _n(never_bound[1]))

    hip = ctypes.CDLL("libamdhip64.so")  # the copy torch has already loaded
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    calls = []

    def copy(user, send, recv, nbytes, stream):  # one rank: what everybody sent is what this rank sent
        calls.append(nbytes)
        return 0 if hip.hipMemcpyAsync(recv, send, nbytes, 3, stream) == 0 else 1

    def reduce(user, buf, count, op, stream):
        calls.append(count)
        return 0

    cbs = (_lib.ALLGATHER_FN(copy), _lib.ALLTOALL_FN(copy), _lib.ALLREDUCE_F32_FN(reduce))
    comm = ctypes.c_void_p()
    assert lib.irs_comm_init_callbacks(ctypes.byref(comm), 0, 1, None, *(ctypes.cast(f, ctypes.c_void_p) for f in cbs)) == 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    s, u, h = _t(seq), _t(usr), _t(hep)
    paths, status = torch.zeros((6, P8), device=DEV), torch.zeros(6, dtype=torch.int32, device=DEV)
    sharded = lambda: lib.irs_generate_paths_sharded(eng.h, comm, p(s), p(u), p(h), 6, P8, 100, 0, 0, 0, 0, 0, p(paths), p(status),  # noqa: E731
                                                     eng._stream())
    keep = eng.bind_path_trace(6, 4)
    try:
        for call in (lambda: eng.beam_search(_t(seq), _t(usr), _t(hep), 3, 2),
                     lambda: eng.beam_search_until(_t(seq), _t(usr), _t(hep), 3, 2)):
            with pytest.raises(IrsError, match=r"error -4\b.*irs_bind_path_trace"):
                call()
        st_in = (torch.zeros((6, 2, 12), dtype=torch.int64, device=DEV), torch.zeros((6, 2), dtype=torch.int32, device=DEV),
                 torch.zeros((6, 2), dtype=torch.float64, device=DEV), torch.zeros((6, 2, 4), device=DEV))
        st_out = tuple(torch.zeros_like(t) for t in st_in)
        val, ids = torch.zeros((12, 100), device=DEV), torch.zeros((12, 100), dtype=torch.int64, device=DEV)
        lse = (torch.zeros(12, device=DEV), torch.ones(12, device=DEV))
        with pytest.raises(IrsError, match=r"error -4\b.*irs_bind_path_trace"):
            eng.beam_step(st_in, val, ids, lse, 0, st_out, status)
        assert sharded() == -4 and b"irs_bind_path_trace" in lib.irs_last_error(eng.h) and not calls
        with pytest.raises(IrsError, match=r"error -1\b.*bound for \[6, 4\]"):  # P = 8 > ld = 4
            eng.generate_paths(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16)
        with pytest.raises(IrsError, match=r"error -1\b.*bound for \[6, 4\]"):
            eng.generate_paths_until(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16)
        seq7, usr7, hep7 = _inputs(g, np.arange(7))
        with pytest.raises(IrsError, match=r"error -1\b.*bound for \[6, 4\]"):  # 7 users > 6
            eng.generate_paths(_t(seq7), _t(usr7), _t(hep7), 4, k=100, sweep=IRS_SWEEP_BF16)
    finally:
        eng.unbind_path_trace()
    del keep
    # an undersized scratch, at the binding and at the stand-alone sweep
    arr = [torch.zeros((6, 4), device=DEV), torch.zeros((6, 4), device=DEV), torch.zeros((6, 4), dtype=torch.int32, device=DEV)]
    small = torch.zeros(eng.path_trace_scratch_bytes(6) - 1, dtype=torch.uint8, device=DEV)
    assert lib.irs_bind_path_trace(eng.h, *(p(a) for a in arr), 6, 4, p(small), small.numel()) == -1
    with pytest.raises(IrsError, match=r"error -1\b.*too small"):
        eng.score_target_trace(torch.zeros((6, 16), device=DEV), _t(seq), _t(hep), scratch=small)
    # unbound: everything runs again, and the greedy loop is the never-bound one bit for bit
    try:
        eng.beam_search(_t(seq), _t(usr), _t(hep), 3, 2)
        eng.beam_search_until(_t(seq), _t(usr), _t(hep), 3, 2)
        assert sharded() == 0 and calls
        torch.cuda.synchronize()
        assert np.array_equal(_n(paths), never_bound[0])
    finally:
        lib.irs_comm_destroy(comm)
    after = eng.generate_paths(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16)
    assert np.array_equal(_n(after[0]).view(np.uint32), never_bound[0].view(np.uint32)) and np.array_equal(_n(after[1]), never_bound[1])


# ============================================================================ 6. the front end
def test_front_end(golden):
    g = golden("irn_tiny")
    cfg = synth.make_config("tiny")
    sd = synth.irn_state_dict(cfg, 1234)
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.to(DEV)
    irn = IRSNN(cfg, net, DEV)
    irn.eval()
    seq, usr, hep = _inputs(g, USERS6)
    targets = seq[:, -1].copy()
    s, u, t = _t(seq), _t(usr), _t(targets)
    with torch.no_grad():
        plain = irn.get_seq_in_batch(s, u, t, P8, 0, False, 3)
        assert not hasattr(irn, "last_trace")
        traced = irn.get_seq_in_batch(s, u, t, P8, 0, False, 3, trace=True)
        tr = irn.last_trace
        stopped = irn.get_seq_in_batch(s, u, t, P8, 0, False, 3, stop_at_target=True, trace=True)
        tr_stop = irn.last_trace
        with pytest.raises(ValueError, match="trace is not built for beam search"):
            irn.get_seq_in_batch(s, u, t, P8, 0, False, 3, beam_width=2, trace=True)
    for a, b in ((traced, plain), (stopped, plain)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3] == 4
        assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    paths, n = traced[0], tr["n_steps"]
    assert n.tolist() == [8, 4, 8, 4, 3, 8]
    # against float64 log_softmax of the package's own forward() logits, windows rebuilt from the returned paths
    win, he = [np.array(r) for r in seq], [int(h) for h in hep]
    LP = None
    for i in range(P8):
        with torch.no_grad():
            lg = net(_t(np.stack(win)), u)
        he_t = _t(np.array(he, dtype=np.int64))
        lg = lg[torch.arange(6, device=DEV), he_t].double()
        lsm = torch.log_softmax(lg, dim=1).cpu().numpy()
        if LP is None:
            LP = _bounds(sd, float(torch.logsumexp(lg, dim=1).abs().max()))[1]
        for b in range(6):
            if i >= n[b]:
                assert tr["lp_item"][b, i] == 0 and tr["lp_target"][b, i] == 0 and tr["rank_target"][b, i] == 0
                continue
            print(f"user {b} step {i}: dlp_target {abs(tr['lp_target'][b, i] - lsm[b, targets[b] - 1]):.3g} "
                  f"dlp_item {abs(tr['lp_item'][b, i] - lsm[b, int(paths[b, i]) - 1]):.3g} bound {LP:.3g}")
            assert abs(tr["lp_target"][b, i] - lsm[b, targets[b] - 1]) <= LP
            assert abs(tr["lp_item"][b, i] - lsm[b, int(paths[b, i]) - 1]) <= LP
            win[b], he[b] = path_ref.advance(win[b], he[b], int(paths[b, i]))
    rows, last = np.arange(6), n - 1
    assert np.array_equal(tr["ioi"], tr["lp_target"][rows, last].astype(np.float64) - tr["lp_target"][:, 0].astype(np.float64))
    assert np.array_equal(tr["ior"], tr["rank_target"][:, 0].astype(np.int64) - tr["rank_target"][rows, last])
    assert np.allclose(tr["avg_lp_item"], [tr["lp_item"][b, :n[b]].astype(np.float64).mean() for b in range(6)], rtol=0, atol=1e-12)
    # an arrival: the target was the chosen item, so the two log-probabilities of that step are one number
    for b in np.where(n < P8)[0]:
        assert tr["lp_item"][b, last[b]] == tr["lp_target"][b, last[b]]
    # stop_at_target: the same dict under the until loop's rule
    eng = net._hip.get(6, 6)
    plain_loop = (traced[0], None, (tr["lp_item"], tr["lp_target"], tr["rank_target"]))
    _check_against_plain(eng, sd, seq, usr, hep, targets, plain_loop, stopped[0],
                         (tr_stop["lp_item"], tr_stop["lp_target"], tr_stop["rank_target"]))
    assert np.array_equal(tr_stop["n_steps"], n)
    for k in ("ioi", "avg_lp_item"):
        assert np.abs(tr_stop[k] - tr[k]).max() <= 2 * LP


# ============================================================================ 7. with exclusions and exact candidates bound as well
def test_trace_with_exclusions_and_exact_candidates(golden):
    """The rank ignores a bound exclusion list and no_repeat, and the chosen item is found in the lists the step chose from
    with the survivor pass in the step: every value against the CPU statement on the dense logits of the windows rebuilt from the returned paths
    (the same rows the loop scored, decoded by another call: the module docstring's bounds)."""
    g = golden("irn_tiny")
    cfg = synth.make_config("tiny")
    sd = synth.irn_state_dict(cfg, 1234)
    eng = _engine("tiny", 128)
    seq, usr, hep = _inputs(g, USERS6)
    targets = seq[:, -1]
    plain = eng.generate_paths(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16)
    excl = _t(_n(plain[0])[:, :3].astype(np.int64) - 1)  # strike what the plain search shows first: the paths must change
    paths, status, tr = eng.generate_paths(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16, trace=True, exclude=excl,
                                           no_repeat=True, exact_candidates=True)
    paths, status, tr = _n(paths), _n(status), [_n(a) for a in tr]
    assert not status.any() and not np.array_equal(paths, _n(plain[0]))
    logits, windows = _walk_logits(eng, seq, usr, hep, paths, np.full(6, P8))
    LOGIT, LP = _bounds(sd, max(abs(ref.lse64(v)) for v in logits.values()))
    excused = 0
    for (b, i), lg in logits.items():
        lp_c, lp_t, rank = ref.step_values(lg, windows[b, i], targets[b], paths[b, i])
        assert abs(float(tr[0][b, i]) - float(lp_c)) <= LP and abs(float(tr[1][b, i]) - float(lp_t)) <= LP
        if tr[2][b, i] != rank:
            assert np.abs(np.delete(lg.astype(np.float64), targets[b] - 1) - float(lg[targets[b] - 1])).min() <= LOGIT
            excused += 1
    assert excused <= 0.05 * len(logits)
