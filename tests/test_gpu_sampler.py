"""-m gpu: the bound sampler (include/irs_hip.h, "sampler": irs_bind_sampler, irs_sampler_choose; sampler= in the engine,
temperature / top_p / draw_k in the front end), against the numpy statement of tests/sampler_ref.py.

Which rows are written, the end mark, status words, the draw u and the support (where the float64 support is unambiguous) are
compared exactly.  The chosen id is the float64 statement's unless the draw lies within TOL of a float64 cumulative bound or
(top_p < 1) top_p lies within TOL of a float64 prefix share S_m / S_n; then either neighbour is accepted, and such cells are
capped at 1 % of the cells of a case.  (At top_p = 1 the float32 support may stop at an earlier prefix that already equals S_n in
float32; the draw is then compared with the same bounds within TOL, so no allowance is needed and none is made.)
TOL = 5e-5 is derived in sampler_ref and confirmed on a float32 emulation in tests/test_sampler_host.py.

lq.  The ratio w_i / S_m* carries a relative error of at most TOL, so log of it moves by at most TOL (1 + TOL), and logf rounds
within 2 ulp of |lq|: |lq - lq64| <= 2 TOL max(1, |lq64|), which is "2 TOL relative" wherever |lq64| >= 1 and the same absolute
bound below (a probability within 1e-4 of 1 has a log that float32 cannot give to 2 TOL RELATIVE: 1 - 2^-24 is the nearest ratio
to 1).

Kernel cases (test_kernel_equals_the_statement): a case is one (L, k, top_k, exclusions) with all nine (T, top_p) and steps 0, 3
and 7: 13 x 27 = 351 cells.  The data seed of a case is 1000 L + 10 k + top_k (+ 5 with exclusions), + 100000 SALT for the three
cases whose first seed put 4, 5 and 6 cells near a bound (1.1 % to 1.7 %).  Checked on the CPU with the float64 statement alone:
the largest share of excused cells over all 78 cases is 0.85 % (3 of 351), 62 cases have none.

The loops are compared with a HOST-STEPPED loop made of the engine's own public calls (decode at hep, score_topk, ..., sampler_choose,
path_step): both sides score the same rows with the same kernels, so everything is equal bit for bit.

Float bounds where the launches differ (the until loop after a compaction, the front end's engine, the float64 oracle): the bound
tests/test_gpu_path_trace.py derives: a logit moves by at most LOGIT = 4e-5 max_j ||W_j||_1, a log-probability by at most
LP = 2 LOGIT + 4e-6 max(1, |lse|).  A weight exp((v_i - v_0) / T) then moves by a relative 2 LOGIT / T, a cumulative share by
twice that: a choice can move only where a draw lies within TOL + 2 LP / T of a bound.  Users and seeds of those tests are chosen
on the CPU oracle so that no draw does, the tests assert it, and nobody is excused (the until test's docstring has its figures).

Meaning (test_paths_are_the_float64_oracles): users [0, 1, 3, 6, 8, 11] of the tiny golden (user 2 of the other tests has two
candidates 9e-5 apart at its first step: the order of its list is undecided between float32 and float64), P = 8, top_k = 5, T = 1,
top_p = 0.9.  Seeds 8, 18 and 23 were chosen on the CPU (oracle_np.decode in float64, stepped by sampler_ref; 12 of the seeds 1 .. 40
qualify) so that every draw of the oracle run is further than TOL + 2 LP = 5.4e-4 from every bound it could cross (LOGIT 1.1e-4,
|lse| <= 5.9):
  seed 8:  smallest distance of a draw to a cumulative bound 1.9e-3, of top_p to a prefix share 3.9e-2, smallest gap between
           neighbouring logits among the kept candidates and the next one 1.5e-3
  seed 18: 2.3e-3, 4.2e-2, 9.3e-4
  seed 23: 4.2e-3, 3.8e-2, 8.1e-4
(the gap between neighbouring logits must exceed 2 LOGIT = 2.2e-4, or the list order itself is undecided)."""
import functools

import numpy as np
import pytest
import torch

import path_ref
import sampler_ref as ref
from gpu_util import make_engine, path_only_engine
from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_ROW_NO_CANDIDATE, IRS_ROW_OFFERED, IRS_ROW_RESCUED, IRS_SWEEP_BF16
from influentialrs_amd.engine import IrsError, Sampler
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_STEP = 600  # catalog of the step-only engines
NINF = np.float32(-np.inf)
TOL = ref.TOL
USERS6 = [0, 2, 3, 6, 8, 11]
P8 = 8
TS = (0.05, 1.0, 4.0)
PS = (0.1, 0.9, 1.0)
STEPS = (0, 3, 7)
K_PAIRS = [(1, 1), (64, 1), (64, 3), (64, 64), (65, 1), (65, 3), (65, 64), (65, 65), (256, 1), (256, 3), (256, 64), (256, 65), (256, 256)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _b32(x):
    return np.float32(x).tobytes()


def _same(got, want, names):
    for name, a, b in zip(names, got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(_bits(a), _bits(b)), (name, np.argwhere(a != b)[:8])


# ============================================================================ 1. the kernel alone
M13 = 13  # three full workgroups of four waves and a quarter-full one
BOUND = 20  # users of the bound records and exclusion lists: a row reads user row_ids[r]
LD = 8


@functools.lru_cache(maxsize=None)
def _step_engine(L):
    return path_only_engine(L, n_item=N_STEP, max_k=256)  # (L > 256: the engine opens a long-window context)


SALT = {(16, 256, 256, True): 2, (256, 256, 256, True): 4, (1024, 65, 64, False): 1}  # cases whose first data seed put more than 1 % of the cells near a bound: another seed (checked on the CPU)


def kernel_case(L, k, top_k, with_excl):
    """13 rows that cycle through hep (first slot, last grow slot, shift slot), through the number of leading candidates the
    window hides (0, 1, top_k, all of them), lists that end early at a negative id, -inf values in the tail, ties in val (the
    values lie on a grid of 1/8 and are drawn with replacement, and the first two admissible values are made equal), a finished
    row, an offered row (the status bit and the offer's list) and a row with the status bit of an earlier step (walked).  With
    exclusions the user's list hides two of the leading admissible candidates and the path (no_repeat) one."""
    g = np.random.default_rng(1000 * L + 10 * k + top_k + (5 if with_excl else 0) + 100000 * SALT.get((L, k, top_k, with_excl), 0))
    heps = [0, L - 3, L - 2]
    seq = g.integers(6001, 9000, size=(M13, L)).astype(np.int64)  # filler: no item of the catalog
    hep = np.zeros(M13, dtype=np.int32)
    val = np.zeros((M13, k), dtype=np.float32)
    ids0 = np.zeros((M13, k), dtype=np.int64)
    fin = np.zeros(M13, dtype=np.int32)
    status = np.zeros(M13, dtype=np.int32)
    row_ids = g.permutation(BOUND)[:M13].astype(np.int32)
    excl = np.full((BOUND, 6), -1, dtype=np.int64)
    paths = np.zeros((BOUND, LD), dtype=np.float32)
    kinds = []
    for r in range(M13):
        he = heps[r % 3]
        wl = he + 1
        ids0[r] = g.permutation(N_STEP)[:k]
        val[r] = np.sort(g.integers(0, 48, size=k).astype(np.float32) * 0.125 - 3.0)[::-1]
        seq[r, L - 1] = int(g.integers(1, N_STEP + 1))
        mode = (r // 3) % 4
        end = k
        if mode == 3:  # the window hides every candidate of a list that ends inside it
            end = min(k, wl)
            c = end
        else:
            c = min([0, 1, top_k][mode], wl, k)
        if r % 5 == 2:
            end = min(end, c + int(g.integers(0, top_k + 2)))
        if end < k:
            ids0[r, end] = -1  # (valid ids follow the end mark: they must not be read)
        free = [int(p) for p in g.permutation(wl)]
        seq[r, free[:c]] = ids0[r, :c] + 1
        if len(free) > c:
            seq[r, free[c]] = 0  # a pad inside the window
        if c + 1 < end:
            val[r, c + 1] = val[r, c]  # a tie at the head of what is left
        if r % 4 == 1 and c + 2 < k:
            val[r, c + 2:] = NINF
        if he + 1 <= L - 2 and c < end:
            seq[r, int(g.integers(he + 1, L - 1))] = ids0[r, c] + 1  # a slot behind hep holds the first admissible: not window
        if with_excl and end - c >= 4:
            u = int(row_ids[r])
            excl[u, :2] = [ids0[r, c], ids0[r, c + 2]]
            paths[u, 0] = ids0[r, c + 1] + 1  # the row's own earlier choice: gone under no_repeat from step 1 on
        hep[r] = he
        kinds.append(dict(he=he, c=c, end=end))
    fin[5] = 1
    status[9] = IRS_ROW_OFFERED | 4
    ids0[9, 0] = seq[9, L - 1] - 1
    if k > 1:
        ids0[9, 1] = -1
    status[11] = IRS_ROW_OFFERED  # the bit of an earlier step: the list is not the offer's
    if ids0[11, 0] == seq[11, L - 1] - 1:
        seq[11, L - 1] = seq[11, L - 1] % N_STEP + 1
    paths[:, 3:] = 5.0  # (entries from `step` on are not path yet: item 5 is admissible at step 3 and gone at step 7)
    return dict(seq=seq, hep=hep, val=val, ids0=ids0, fin=fin, status=status, row_ids=row_ids, excl=excl, paths=paths, kinds=kinds)


def kernel_cells(case, top_k, with_excl, seed=77):
    """The float64 statement of every cell of a case: [(T, top_p, step, val, ids0, rec)]."""
    out = []
    for T in TS:
        for p in PS:
            for step in STEPS:
                v, i, rec = ref.choose(case["seq"], case["hep"], case["val"], case["ids0"], top_k, T, p, step, seed, row_ids=case["row_ids"],
                                       status=case["status"], fin=case["fin"], excl=case["excl"] if with_excl else None, n_item=N_STEP,
                                       paths=case["paths"] if with_excl else None, no_repeat=with_excl)
                out.append((T, p, step, v, i, rec))
    return out


def excused(rec, top_p, extra=0.0):
    """Rows whose chosen id may be a neighbour's: the draw within TOL of a cumulative bound, or (top_p < 1) top_p within TOL of a
    prefix share."""
    e = rec["near_u"] <= TOL + extra
    if top_p < 1.0:
        e = e | (rec["near_p"] <= TOL + extra)
    return e & rec["written"]


@pytest.mark.parametrize("with_excl", [False, True])
@pytest.mark.parametrize("k,top_k", K_PAIRS)
@pytest.mark.parametrize("L", [16, 256, 1024])
def test_kernel_equals_the_statement(L, k, top_k, with_excl):
    eng = _step_engine(L)
    case = kernel_case(L, k, top_k, with_excl)
    cells = kernel_cells(case, top_k, with_excl)
    seq, hep, status, fin, row_ids = (_t(case[n]) for n in ("seq", "hep", "status", "fin", "row_ids"))
    d_paths = _t(case["paths"])
    n_cells = n_excused = n_support = 0
    seen = dict(written=0, none=0, later=0, short=0)
    held = eng.bind_exclusions(_t(case["excl"]), BOUND, True) if with_excl else None  # (the caller keeps the scratch alive while bound)
    try:
        for T, p, step, w_val, w_ids, rec in cells:
            got = []
            for _ in range(2):  # two calls give equal bits
                rec_t = eng.bind_sampler(top_k, T, p, BOUND, LD, record=True)
                for a in rec_t:
                    a.fill_(7)  # (cells the kernel must not write keep the 7)
                d_val, d_ids = _t(case["val"]), _t(case["ids0"])
                eng.sampler_choose(seq, hep, d_val, d_ids, step, 77, status, row_ids=row_ids, fin=fin, paths=d_paths if with_excl else None)
                got.append((_n(d_val), _n(d_ids)) + tuple(_n(a) for a in rec_t))
                eng.unbind_sampler()
            _same(got[1], got[0], ("val", "ids0", "u", "lq", "support"))
            o_val, o_ids, r_u, r_lq, r_sup = got[0]
            assert np.array_equal(_n(status), case["status"]), "the status words are read only"
            exc = excused(rec, p)
            for r in range(M13):
                n_cells += 1
                u_row = int(case["row_ids"][r])
                cell = (L, k, top_k, with_excl, T, p, step, r)
                if not rec["written"][r]:  # finished, offered, or without an admissible candidate: the list is left alone
                    assert np.array_equal(o_ids[r], case["ids0"][r]) and np.array_equal(_bits(o_val[r]), _bits(case["val"][r])), cell
                    if not rec["recorded"][r]:
                        assert r_u[u_row, step] == 7 and r_lq[u_row, step] == 7 and r_sup[u_row, step] == 7, cell
                    else:
                        assert (r_u[u_row, step], r_lq[u_row, step], r_sup[u_row, step]) == (0, 0, int(rec["support"][r])), cell
                        seen["none"] += rec["support"][r] == 0
                    continue
                seen["written"] += 1
                seen["later"] += rec["index"][r] > 0
                seen["short"] += rec["support"][r] < rec["n"][r]
                # entries 0 and 1 are rewritten, nothing else
                if k > 1:
                    assert o_ids[r, 1] == -1 and o_val[r, 1] == NINF, cell
                    assert np.array_equal(o_ids[r, 2:], case["ids0"][r, 2:]) and np.array_equal(_bits(o_val[r, 2:]), _bits(case["val"][r, 2:])), cell
                assert _b32(r_u[u_row, step]) == _b32(rec["u"][r]), cell
                kept = rec["kept"][r]
                want = rec["index"][r]
                at = [j for j, (v, c) in enumerate(kept) if case["ids0"][r, c] == o_ids[r, 0]]
                assert len(at) == 1 and _b32(o_val[r, 0]) == _b32(kept[at[0]][0]), cell
                if exc[r]:
                    n_excused += 1
                    assert abs(at[0] - want) <= 1, cell
                    continue
                assert at[0] == want, cell + (at[0], want, rec["near_u"][r], rec["near_p"][r])
                if rec["near_p"][r] > TOL:
                    n_support += 1
                    assert r_sup[u_row, step] == rec["support"][r], cell
                assert 1 <= r_sup[u_row, step] <= rec["n"][r] and at[0] < r_sup[u_row, step], cell
                lq64 = rec["lq"][r]
                assert abs(float(r_lq[u_row, step]) - lq64) <= 2 * TOL * max(1.0, abs(lq64)), cell + (r_lq[u_row, step], lq64)
    finally:
        torch.cuda.synchronize()
        if with_excl:
            eng.unbind_exclusions()
        del held
    assert n_cells == M13 * 27 and n_excused <= 0.01 * n_cells, (n_excused, n_cells)
    assert seen["written"] and seen["none"] and n_support
    if top_k > 1 and k > 1:
        assert seen["later"] and seen["short"]


# ============================================================================ 2. the loops against a host-stepped loop
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


NAMES = ("paths", "seq", "hep", "status", "u", "lq", "support")


def _host_stepped(eng, seq, usr, hep, P, sm, seed, k=100, arrive_rank=None, exact=False, excl=None, no_repeat=False, offer=None):
    """The bound loop made of public calls, one step at a time.  Returns dict(paths, seq, hep, status, u, lq, support, trace,
    near): near [B, P] is the float64 statement's distance of each draw to a bound it could cross, index [B, P] its choice."""
    B = len(seq)
    n_item = eng.n_item
    seq, usr, hep = _t(seq), _t(usr), _t(hep)
    paths = torch.zeros((B, P), dtype=torch.float32, device=DEV)
    status = torch.zeros(B, dtype=torch.int32, device=DEV)
    lp_item, lp_target = np.zeros((B, P), dtype=np.float32), np.zeros((B, P), dtype=np.float32)
    rank = np.zeros((B, P), dtype=np.int32)
    near, index, item = np.ones((B, P)), np.full((B, P), -1), np.zeros((B, P), dtype=np.int64)
    bound = excl is not None or no_repeat
    held = []  # (the caller keeps a binding's scratch alive while bound)
    if bound:
        held.append(eng.bind_exclusions(None if excl is None else _t(excl), B, no_repeat))
    if offer is not None:
        held.append(eng.bind_offer_set(_t(offer), B))
    rec = eng.bind_sampler(sm.top_k, sm.temperature, sm.top_p, B, P, record=True)
    try:
        for i in range(P):
            _, xr, _ = eng.decode(seq, usr, want_x=False, pos=hep)
            if offer is not None:
                val, ids, _ = eng.score_topk_offer(xr, k)
            else:
                val, ids, _ = eng.score_topk(xr, k, IRS_SWEEP_BF16, carry=i > 0)
            if exact:
                eng.ensure_survivors(xr, seq, hep, val, ids, status, want=sm.top_k)
            if arrive_rank is not None:
                mx, smx, ts, rk = eng.score_target_trace(xr, seq, hep)
                eng.arrival_offer(seq, hep, mx, smx, ts, rk, val, ids, status, rank_max=arrive_rank, paths=paths, step=i)
            step_status = _n(status)
            _, w_ids, w = ref.choose(_n(seq), _n(hep), _n(val), _n(ids), sm.top_k, sm.temperature, sm.top_p, i, seed, status=step_status,
                                     excl=excl, n_item=n_item, paths=_n(paths), no_repeat=no_repeat)
            near[:, i] = np.minimum(w["near_u"], w["near_p"] if sm.top_p < 1 else 1.0)
            index[:, i], item[:, i] = w["index"], w_ids[:, 0] + 1
            eng.sampler_choose(seq, hep, val, ids, i, seed, status, paths=paths if no_repeat else None)
            eng.path_step(seq, hep, val, ids, i, paths, status)
            if arrive_rank is not None:
                n_val, n_ids, chosen = _n(val), _n(ids), _n(paths)[:, i]
                lse = _n(mx).astype(np.float64) + np.log(_n(smx).astype(np.float64))
                for b in range(B):
                    lp_target[b, i] = np.float32(np.float64(_n(ts)[b]) - lse[b])
                    assert chosen[b] != 0 and n_ids[b, 0] == int(chosen[b]) - 1, "the chosen item stands in entry 0"
                    lp_item[b, i] = np.float32(np.float64(n_val[b, 0]) - lse[b])
                rank[:, i] = _n(rk)
        out = dict(paths=_n(paths), seq=_n(seq), hep=_n(hep), status=_n(status), u=_n(rec[0]).copy(), lq=_n(rec[1]).copy(),
                   support=_n(rec[2]).copy(), trace=(lp_item, lp_target, rank) if arrive_rank is not None else None, near=near, index=index,
                   item=item)
    finally:
        torch.cuda.synchronize()
        eng.unbind_sampler()
        if offer is not None:
            eng.unbind_offer_set()
        if bound:
            eng.unbind_exclusions()
        held.clear()
    return out


def _loop(eng, seq, usr, hep, P, sm, seed, k=100, until=False, **kw):
    """generate_paths / generate_paths_until with sampler= and a record: the same dict as _host_stepped (without near)."""
    d_seq, d_hep = _t(seq), _t(hep)
    trace = kw.get("trace", False)
    sm = Sampler(sm.top_k, sm.temperature, sm.top_p, True)
    if until:
        out = eng.generate_paths_until(d_seq, _t(usr), d_hep, P, k=k, sweep=IRS_SWEEP_BF16, seed=seed, sampler=sm, **kw)
        paths, status, rest = out[0], out[1], out[4:]
    else:
        out = eng.generate_paths(d_seq, _t(usr), d_hep, P, k=k, sweep=IRS_SWEEP_BF16, seed=seed, sampler=sm, **kw)
        paths, status, rest = out[0], out[1], out[2:]
    tr = tuple(_n(a) for a in rest[0]) if trace else None
    u, lq, support = rest[-1]
    return dict(paths=_n(paths), seq=_n(d_seq), hep=_n(d_hep), status=_n(status), u=_n(u), lq=_n(lq), support=_n(support), trace=tr)


def _equal_runs(got, want, what):
    _same([got[k] for k in NAMES], [want[k] for k in NAMES], [f"{what}: {k}" for k in NAMES])
    if want["trace"] is not None:
        _same(got["trace"], want["trace"], [f"{what}: lp_item", f"{what}: lp_target", f"{what}: rank_target"])


SM = Sampler(5, 1.5, 0.9)


def _check_against_statement(run):
    """Where the float64 statement is unambiguous, a written draw of the host-stepped loop chose what it names; lq <= 0."""
    far = run["near"] > TOL
    assert far.mean() >= 0.9
    assert (run["lq"] <= 0).all() and (run["support"] >= 0).all()
    assert np.array_equal(run["paths"][far].astype(np.int64), run["item"][far]), np.argwhere(far & (run["paths"] != run["item"]))[:8]
    return far


@pytest.mark.parametrize("variant", ["plain", "exclusions", "offer", "exact", "arrival"])
def test_loops_equal_the_host_stepped_loop(golden, variant):
    t = _tiny(golden)
    eng = t["eng"]
    seq, usr, hep = _inputs(t, USERS6)
    B = len(seq)
    host, loop, sm, k = {}, {}, SM, 100
    if variant == "exclusions":
        free = _loop(eng, seq, usr, hep, P8, SM, 21)
        excl = np.full((B, 6), -1, dtype=np.int64)
        excl[:, :3] = free["paths"][:, [0, 2, 5]].astype(np.int64) - 1  # what the free search chose goes on the list
        host, loop = dict(excl=excl, no_repeat=True), dict(exclude=_t(excl), no_repeat=True)
    elif variant == "offer":
        offer = np.arange(0, t["cfg"].n_item, 2, dtype=np.int64)
        host, loop = dict(offer=offer), dict(offer=_t(offer))
    elif variant == "exact":
        sm, k = Sampler(3, 1.5, 0.9), 3  # three candidates: a window that hides one starves the row of its third
        host, loop = dict(exact=True), dict(exact_candidates=True)
    elif variant == "arrival":
        host, loop = dict(arrive_rank=10), dict(trace=True, arrive_rank=10)
    want = _host_stepped(eng, seq, usr, hep, P8, sm, 21, k=k, **host)
    _check_against_statement(want)
    stream = _loop(eng, seq, usr, hep, P8, sm, 21, k=k, **loop)
    _equal_runs(stream, want, "stream")
    _equal_runs(_loop(eng, seq, usr, hep, P8, sm, 21, k=k, use_graph=True, **loop), want, "captured")
    _equal_runs(_loop(eng, seq, usr, hep, P8, sm, 21, k=k, **loop), stream, "again")  # no atomics: identical bytes
    assert not (want["status"] & IRS_ROW_NO_CANDIDATE).any() and (want["paths"] != 0).all()
    other = _loop(eng, seq, usr, hep, P8, sm, 22, k=k, **loop)
    drew = stream["support"] > 1  # (an offered row records u = 0 under every seed)
    assert (other["paths"] != stream["paths"]).any() and (other["u"] != stream["u"])[drew].all(), "another seed, other draws"
    for b in range(B):
        for i in range(P8):
            assert _b32(want["u"][b, i]) == _b32(ref.draw(21, b, i)) or (want["status"][b] & IRS_ROW_OFFERED)
    if variant == "exclusions":
        for b in range(B):
            assert not set((host["excl"][b, :3] + 1).tolist()) & set(stream["paths"][b].tolist()), "a listed item is never drawn"
            assert len(set(stream["paths"][b].tolist())) == P8, "no_repeat: nothing is offered twice"
    if variant == "offer":
        assert ((stream["paths"].astype(np.int64) - 1) % 2 == 0).all(), "every drawn item is of the set"
    if variant == "exact":
        assert (want["status"] & IRS_ROW_RESCUED).any()
    if variant == "arrival":
        offered = (stream["status"] & IRS_ROW_OFFERED) != 0
        assert offered.any() and not offered.all()
        for b in np.where(offered)[0]:
            i = int(np.where(stream["paths"][b] == seq[b, -1])[0][0])
            assert (stream["u"][b, i], stream["lq"][b, i], stream["support"][b, i]) == (0, 0, 1), "the arrival rule had chosen"
    if variant == "plain":
        # (the tiny model's best logits lie close together: the nucleus keeps all five here; the kernel cases cut it)
        assert (want["index"] > 0).any() and (want["support"] > 1).all() and (want["lq"] < 0).all()


def test_loop_above_the_small_plan_switch(golden):
    """70 users: beyond the 64 rows of the single-workgroup plan, so the step counter moves by its own launch behind the step."""
    t = _tiny(golden)
    eng = make_engine(t["cfg"], t["sd"], max_rows=160, max_seqs=160)
    seq, usr, hep = _inputs(t, np.arange(70) % 12)
    want = _host_stepped(eng, seq, usr, hep, 3, SM, 5)
    _equal_runs(_loop(eng, seq, usr, hep, 3, SM, 5), want, "stream")
    _equal_runs(_loop(eng, seq, usr, hep, 3, SM, 5, use_graph=True), want, "captured")
    assert (want["u"][12:24] != want["u"][:12]).all(), "equal users in other rows draw apart"


def _bounds(sd, lse_abs):
    logit = 4e-5 * float(np.abs(sd["project.weight"]).sum(axis=1).max())
    return logit, 2 * logit + 4e-6 * max(1.0, lse_abs)


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


UNTIL_USERS, UNTIL_SEED, UNTIL_RANK = [0, 1, 3, 6, 8, 11], 59, 10
UNTIL_SM = Sampler(8, 2.0, 0.95)


def oracle_until(oracle, t, users, seed, P, sm, rank_max):
    """The sampled until search with the arrival rule at rank <= rank_max, stepped by sampler_ref on the float64 oracle.  Returns
    (live steps per user, near -- the smallest distance of a draw to a cumulative bound or of top_p to a prefix share --, gap --
    the smallest gap between neighbouring logits among the kept candidates and the next one --, tgap -- the smallest gap between
    the target's logit and any other admissible item's: the rank the rule reads is decided by more than that)."""
    seq, usr, hep = _inputs(t, users)
    W, bias = t["sd"]["project.weight"].astype(np.float64), t["sd"]["project.bias"].astype(np.float64)
    inv_t = np.float32(1.0) / np.float32(sm.temperature)
    live, near, gap, tgap = [], np.inf, np.inf, np.inf
    for b in range(len(seq)):
        w, h, tgt, n = seq[b].copy(), int(hep[b]), int(seq[b, -1]), P
        for i in range(P):
            x, _ = oracle.decode(t["sd"], t["cfg"], w, int(usr[b]), dtype=np.float64)
            lg = W @ x[h] + bias
            inwin = {int(v) for v in w[:h + 1]}
            offered = False
            if tgt not in inwin:
                others = np.array([lg[j] for j in range(len(lg)) if (j + 1) not in inwin and j != tgt - 1])
                tgap = min(tgap, float(np.abs(others - lg[tgt - 1]).min()))
                offered = 1 + int((others > lg[tgt - 1]).sum()) <= rank_max
            item = tgt
            if not offered:
                order = np.lexsort((np.arange(len(lg)), -lg))[:100]
                kept = ref.walk(w[:h + 1], lg[order], order, sm.top_k + 1)
                v = np.array([kv[0] for kv in kept])
                gap = min(gap, float(np.min(-np.diff(v))))
                c = ref.choose64(v[:sm.top_k], inv_t, sm.top_p, ref.draw(seed, b, i))
                near = min(near, c["near_u"], c["near_p"])
                item = int(order[kept[c["index"]][1]]) + 1
            if item == tgt:
                n = i + 1
                break
            w, h = path_ref.advance(w, h, item)
        live.append(n)
    return live, near, gap, tgap


@pytest.mark.parametrize("check_every", [1, 3])
def test_until_loop_equals_the_plain_loop_cut_on_the_host(golden, oracle, check_every):
    """The draws are keyed by the caller's row, so u is the plain loop's bit for bit.  After a compaction the decode runs on fewer
    rows and a score may move within LOGIT, which could move a choice only where a draw lies within slack = TOL + 2 LP / T = 3.0e-4
    of a bound, where two neighbouring logits lie within 2 LOGIT = 2.2e-4 (the list order), or where the target's logit lies that
    near another item's (the rank the arrival rule reads).  Users [0, 1, 3, 6, 8, 11], seed 59, top_k = 8, T = 2, top_p = 0.95 and
    the arrival rule at rank 10 were chosen on the CPU (oracle_np.decode in float64, stepped by sampler_ref; seeds 1 .. 60 over
    three user sets) so that NOBODY is excused: on the oracle the smallest distance of a draw to a bound is 5.4e-3, the smallest
    gap between neighbouring kept logits 5.3e-4, between the target's logit and another item's 1.1e-3, and users 0, 6 and 11
    arrive at steps 4, 2 and 4 (counted from 1) while users 1, 3 and 8 never do: two compactions.  The test asserts those margins on
    the oracle AND on the device's own lists, then compares every user: paths id for id, u and support exactly, records zero behind
    the arrival.  lq = log(w_i / S): each argument (v_i - v_0) / T moves by at most 2 LOGIT / T and so does log S, so lq is held to
    4 LOGIT / T <= 2 LP / T."""
    t = _tiny(golden)
    eng = t["eng"]
    sm, seed, rule = UNTIL_SM, UNTIL_SEED, dict(trace=True, arrive_rank=UNTIL_RANK)
    seq, usr, hep = _inputs(t, UNTIL_USERS)
    B = len(seq)
    targets = seq[:, -1].copy()
    LOGIT, LP = _bounds(t["sd"], 8.0)  # (|lse| of the tiny model stays below 6)
    slack = TOL + 2 * LP / sm.temperature
    live, near, gap, tgap = oracle_until(oracle, t, UNTIL_USERS, seed, P8, sm, UNTIL_RANK)
    print(f"oracle: live steps {live}, draw to bound {near:.3g}, logit gap {gap:.3g}, target gap {tgap:.3g}; slack {slack:.3g}, 2 LOGIT {2 * LOGIT:.3g}")
    assert near > slack and gap > 2 * LOGIT and tgap > 2 * LOGIT, "users and seed were chosen for their margins: nobody is excused"
    assert 2 <= sum(v < P8 for v in live) < B and len({v for v in live if v < P8}) >= 2, live  # two compactions, not everybody
    host = _host_stepped(eng, seq, usr, hep, P8, sm, seed, arrive_rank=UNTIL_RANK)
    plain = _loop(eng, seq, usr, hep, P8, sm, seed, **rule)
    _equal_runs(plain, host, "plain")
    n, (w_paths, w_u, w_lq, w_sup) = _cut(plain["paths"], targets, [plain[k] for k in ("paths", "u", "lq", "support")])
    assert n.tolist() == live, (n, live)
    dev_near = [float(host["near"][b, :n[b]].min()) for b in range(B)]
    print(f"device: live steps {n.tolist()}, smallest distance of a draw to a bound per user {dev_near}")
    assert min(dev_near) > slack, "every user is compared"
    got = _loop(eng, seq, usr, hep, P8, sm, seed, until=True, check_every=check_every, **rule)
    assert np.array_equal(_bits(got["u"]), _bits(w_u)), "the draws are the caller's rows': equal bits, zero behind the arrival"
    assert np.array_equal(got["paths"], w_paths), (got["paths"], w_paths)
    assert np.array_equal(got["support"], w_sup)
    for b in range(B):
        assert not got["lq"][b, n[b]:].any(), "zero behind the arrival"
    assert np.abs(got["lq"].astype(np.float64) - w_lq.astype(np.float64)).max() <= 2 * LP / sm.temperature
    # targets that never arrive (the last item of the history: the window holds it for all 8 steps): nothing is compacted, the
    # same launches on the same bytes
    far = seq.copy()
    far[:, -1] = far[:, -2]
    want = _loop(eng, far, usr, hep, P8, sm, seed, **rule)
    assert not (want["paths"] == far[:, -1:]).any()
    got = _loop(eng, far, usr, hep, P8, sm, seed, until=True, check_every=check_every, **rule)
    _same([got[k] for k in ("paths", "status", "u", "lq", "support")], [want[k] for k in ("paths", "status", "u", "lq", "support")],
          ("paths", "status", "u", "lq", "support"))


# ============================================================================ 3. meaning, against the float64 oracle
def oracle_paths(oracle, t, users, seed, P, sm, k=100):
    """The sampled search stepped by sampler_ref on the float64 oracle.  Returns (paths [B, P], near_u, near_p, gap -- the smallest
    distance of a draw to a cumulative bound, of top_p to a prefix share, and between neighbouring logits among the kept
    candidates and the next one --, the largest |lse|)."""
    seq, usr, hep = _inputs(t, users)
    W, bias = t["sd"]["project.weight"].astype(np.float64), t["sd"]["project.bias"].astype(np.float64)
    paths = np.zeros((len(seq), P))
    near_u = near_p = gap = np.inf
    lse_abs = 0.0
    inv_t = np.float32(1.0) / np.float32(sm.temperature)
    for b in range(len(seq)):
        w, h = seq[b].copy(), int(hep[b])
        for i in range(P):
            x, _ = oracle.decode(t["sd"], t["cfg"], w, int(usr[b]), dtype=np.float64)
            lg = W @ x[h] + bias
            lse_abs = max(lse_abs, abs(lg.max() + np.log(np.exp(lg - lg.max()).sum())))
            order = np.lexsort((np.arange(len(lg)), -lg))[:k]
            kept = ref.walk(w[:h + 1], lg[order], order, sm.top_k + 1)
            v = np.array([kv[0] for kv in kept])
            gap = min(gap, float(np.min(-np.diff(v)))) if len(v) > 1 else gap
            kept = kept[:sm.top_k]
            c = ref.choose64(v[:sm.top_k], inv_t, sm.top_p, ref.draw(seed, b, i))
            near_u, near_p = min(near_u, c["near_u"]), min(near_p, c["near_p"])
            item = int(order[kept[c["index"]][1]]) + 1
            paths[b, i] = item
            w, h = path_ref.advance(w, h, item)
    return paths, near_u, near_p, gap, lse_abs


SM_ORACLE = Sampler(5, 1.0, 0.9)
ORACLE_SEEDS = (8, 18, 23)
USERS_ORACLE = [0, 1, 3, 6, 8, 11]


@pytest.mark.parametrize("seed", ORACLE_SEEDS)
def test_paths_are_the_float64_oracles(golden, oracle, seed):
    t = _tiny(golden)
    want, near_u, near_p, gap, lse_abs = oracle_paths(oracle, t, USERS_ORACLE, seed, P8, SM_ORACLE)
    LOGIT, LP = _bounds(t["sd"], lse_abs)
    print(f"seed {seed}: draw to bound {near_u:.3g}, top_p to share {near_p:.3g}, logit gap {gap:.3g}; TOL + 2 LP {TOL + 2 * LP:.3g}, "
          f"2 LOGIT {2 * LOGIT:.3g}, |lse| <= {lse_abs:.3g}")
    assert near_u > TOL + 2 * LP and near_p > TOL + 2 * LP and gap > 2 * LOGIT, "the seed was chosen for its margins"
    seq, usr, hep = _inputs(t, USERS_ORACLE)
    got = _loop(t["eng"], seq, usr, hep, P8, SM_ORACLE, seed)
    assert np.array_equal(got["paths"].astype(np.float64), want), (got["paths"], want)
    greedy = t["eng"].generate_paths(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16)[0]
    assert (_n(greedy) != got["paths"]).any(), "the draws did choose: a candidate other than the first, somewhere"


# ============================================================================ 4. refusals and state
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
    INVALID, STATE, UNSUPPORTED = -1, -2, -4
    for T in (0.0, -1.0, float("inf"), float("nan")):
        refused(INVALID, "irs_bind_sampler", "temperature")(lambda: eng.bind_sampler(3, T, 1.0))
    for p in (0.0, 1.5, float("nan")):
        refused(INVALID, "irs_bind_sampler", "top_p")(lambda: eng.bind_sampler(3, 1.0, p))
    for top_k in (-1, 101, 257):
        refused(UNSUPPORTED, "irs_bind_sampler", "top_k")(lambda: eng.bind_sampler(top_k))
    with pytest.raises(IrsError, match="record=True needs users >= 1 and ld >= 1"):
        eng.bind_sampler(3, record=True)
    table = torch.zeros((t["cfg"].n_item + 1, 4), device=DEV)
    eng.bind_guide(table, 3)
    try:
        refused(UNSUPPORTED, "irs_bind_sampler", "irs_bind_guide")(lambda: eng.bind_sampler(3))
    finally:
        eng.unbind_guide()
    eng.bind_lookahead(3, 6, 8)
    try:
        refused(UNSUPPORTED, "irs_bind_sampler", "irs_bind_lookahead")(lambda: eng.bind_sampler(3))
    finally:
        eng.unbind_lookahead()
    refused(STATE, "irs_sampler_choose", "no sampler is bound")(
        lambda: eng.sampler_choose(_t(seq), _t(hep), torch.zeros((6, 100), device=DEV), torch.zeros((6, 100), dtype=torch.int64, device=DEV),
                                   0, 1, torch.zeros(6, dtype=torch.int32, device=DEV)))
    eng.bind_sampler(5, 0.7, 0.9, 6, 8, record=True)
    try:
        refused(UNSUPPORTED, "irs_bind_guide", "irs_bind_sampler")(lambda: eng.bind_guide(table, 3))
        refused(UNSUPPORTED, "irs_bind_lookahead", "irs_bind_sampler")(lambda: eng.bind_lookahead(3, 6, 8))
        gp = lambda **kw: eng.generate_paths(_t(seq), _t(usr), _t(hep), kw.pop("P", P8), sweep=IRS_SWEEP_BF16, **kw)  # noqa: E731
        refused(INVALID, "irs_generate_paths", "two samplers")(lambda: gp(sample=True))
        refused(INVALID, "irs_generate_paths_until", "two samplers")(
            lambda: eng.generate_paths_until(_t(seq), _t(usr), _t(hep), P8, sample=True))
        refused(INVALID, "irs_generate_paths", "k=4 < top_k=5")(lambda: gp(k=4))
        refused(INVALID, "irs_generate_paths", "[6, 8]")(lambda: gp(P=9))
        seq7, usr7, hep7 = _inputs(t, USERS6 + [1])
        refused(INVALID, "[6, 8]")(lambda: eng.generate_paths(_t(seq7), _t(usr7), _t(hep7), P8))
        refused(UNSUPPORTED, "irs_beam_search", "greedy loops only")(lambda: eng.beam_search(_t(seq), _t(usr), _t(hep), 3, 2))
        refused(UNSUPPORTED, "irs_beam_search_until", "irs_bind_sampler")(lambda: eng.beam_search_until(_t(seq), _t(usr), _t(hep), 3, 2))
        B, W, L = 2, 2, seq.shape[1]
        st = (torch.zeros((B, W, L), dtype=torch.int64, device=DEV), torch.zeros((B, W), dtype=torch.int32, device=DEV),
              torch.zeros((B, W), dtype=torch.float64, device=DEV), torch.zeros((B, W, 3), dtype=torch.float32, device=DEV))
        so = tuple(torch.zeros_like(a) for a in st)
        lists = (torch.zeros((B * W, 10), device=DEV), torch.zeros((B * W, 10), dtype=torch.int64, device=DEV))
        lse = (torch.zeros(B * W, device=DEV), torch.ones(B * W, device=DEV))
        refused(UNSUPPORTED, "irs_beam_step", "irs_bind_sampler")(
            lambda: eng.beam_step(st, lists[0], lists[1], lse, 0, so, torch.zeros(B, dtype=torch.int32, device=DEV)))
    finally:
        torch.cuda.synchronize()
        eng.unbind_sampler()
    # top_k > 32 with a survivor scratch
    scratch = torch.empty(eng.survivor_scratch_bytes(len(seq), 32), dtype=torch.uint8, device=DEV)
    eng._check(eng.lib.irs_bind_survivor_scratch(eng.h, scratch.data_ptr(), scratch.numel()))
    eng.bind_sampler(33)
    try:
        refused(UNSUPPORTED, "irs_generate_paths", "irs_bind_sampler", "32")(lambda: eng.generate_paths(_t(seq), _t(usr), _t(hep), 2))
    finally:
        eng.unbind_sampler()
        eng._check(eng.lib.irs_bind_survivor_scratch(eng.h, None, 0))
    # nothing stayed bound
    eng.generate_paths(_t(seq), _t(usr), _t(hep), 2, sample=True, sample_k=3, seed=5)
    torch.cuda.synchronize()


def test_a_sharded_context_refuses_the_binding():
    cfg = synth.make_config("tiny")
    eng = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=64, max_seqs=64, rank=0, world=2)
    with pytest.raises(IrsError) as e:
        eng.bind_sampler(3)
    assert "error -4:" in str(e.value) and "whole catalog" in str(e.value)


def test_unbind_restores_a_fresh_engines_bytes_and_binding_drops_the_captured_step(golden):
    t = _tiny(golden)
    eng = t["eng"]
    seq, usr, hep = _inputs(t, USERS6)

    def plain(e, **kw):
        d_seq, d_hep = _t(seq), _t(hep)
        paths, status = e.generate_paths(d_seq, _t(usr), d_hep, P8, k=100, sweep=IRS_SWEEP_BF16, **kw)
        return _n(paths), _n(status), _n(d_seq), _n(d_hep)
    new = make_engine(t["cfg"], t["sd"], max_rows=64, max_seqs=64)
    fresh, fresh_sampled = plain(new), plain(new, sample=True, sample_k=3, seed=9)
    names = ("paths", "status", "seq", "hep")
    _same(plain(eng, use_graph=True), fresh, names)  # a captured unbound step ...
    want = _host_stepped(eng, seq, usr, hep, P8, SM, 6)
    rec = eng.bind_sampler(SM.top_k, SM.temperature, SM.top_p, len(seq), P8, record=True)  # ... a binding of the caller's own drops it ...
    try:
        bound = plain(eng, use_graph=True, seed=6)
        _same(bound, [want[k] for k in names], names)
        _same(tuple(_n(a) for a in rec), (want["u"], want["lq"], want["support"]), ("u", "lq", "support"))
        _same(plain(eng, use_graph=True, seed=6), bound, names)  # replayed
        assert (plain(eng, use_graph=True, seed=7)[0] != bound[0]).any(), "the seed is part of the captured step's key"
    finally:
        torch.cuda.synchronize()
        eng.unbind_sampler()
    _same(plain(eng, use_graph=True), fresh, names)  # ... and the unbound calls are a fresh engine's again
    _same(plain(eng), fresh, names)
    _same(plain(eng, sample=True, sample_k=3, seed=9), fresh_sampled, names)
    assert (bound[0] != fresh[0]).any()


# ============================================================================ 5. the front end
def test_front_end_sampler(golden, oracle):
    """torch.manual_seed(27) gives the front end the draw seed 1426978528, chosen on the CPU oracle like the until test's: over users
    [0, 1, 3, 6, 8, 11] the smallest distance of a draw to a bound is 1.2e-2, the smallest gap between neighbouring kept logits
    7.8e-4 (slack = TOL + 2 LP / 1.5 = 3.9e-4, 2 LOGIT = 2.2e-4), and user 6 draws its target at step 2, so stop_at_target=True
    compacts once.  Asserted below; then stop_at_target=True returns the paths of stop_at_target=False for every user."""
    t = _tiny(golden)
    cfg = t["cfg"]
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in t["sd"].items()})
    net.to(DEV)
    irn = IRSNN(cfg, net, DEV)
    irn.eval()
    seq, usr, hep = _inputs(t, UNTIL_USERS)
    targets = seq[:, -1].copy()
    kw = dict(temperature=1.5, top_p=0.9, draw_k=5)
    torch.manual_seed(27)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())  # (what the front end draws for the call)
    live, near, gap, _ = oracle_until(oracle, t, UNTIL_USERS, seed, P8, Sampler(5, 1.5, 0.9), 0)
    LOGIT, LP = _bounds(t["sd"], 8.0)
    assert near > TOL + 2 * LP / 1.5 and gap > 2 * LOGIT and 1 <= sum(v < P8 for v in live) < len(seq), (seed, live, near, gap)
    with torch.no_grad():
        torch.manual_seed(27)
        paths, tg, hist, early = irn.get_seq_in_batch(_t(seq), _t(usr), _t(targets), P8, 0, draw_record=True, **kw)
        rec = irn.last_draws
        torch.manual_seed(27)
        until = irn.get_seq_in_batch(_t(seq), _t(usr), _t(targets), P8, 0, stop_at_target=True, draw_record=True, **kw)[0]
        rec_until = irn.last_draws
        torch.manual_seed(4)
        other = irn.get_seq_in_batch(_t(seq), _t(usr), _t(targets), P8, 0, **kw)[0]
        one = irn.get_seq_in_batch(_t(seq), _t(usr), _t(targets), P8, 0, draw_k=1)[0]
        greedy = irn.get_seq_in_batch(_t(seq), _t(usr), _t(targets), P8, 0)[0]
    assert np.array_equal(one, greedy), "draw_k = 1 is the greedy search"
    assert (paths != greedy).any() and (other != paths).any() and np.array_equal(tg, targets)
    assert set(rec) == {"u", "lq", "support"} and rec["u"].shape == (len(seq), P8) and rec["support"].dtype == np.int32
    assert np.array_equal(_bits(rec["u"]), _bits(rec_until["u"])), "the same seed, the same rows, the same draws"
    assert np.array_equal(until, paths)
    assert [int(np.where(paths[b] == targets[b])[0][0]) + 1 if (paths[b] == targets[b]).any() else P8 for b in range(len(seq))] == live
    for b in range(len(seq)):
        pos = np.where(paths[b] == targets[b])[0]
        n = pos[0] + 1 if len(pos) else P8
        assert (rec["support"][b, :n] >= 1).all() and (rec["lq"][b, :n] <= 0).all()
        assert not rec["u"][b, n:].any() and not rec["lq"][b, n:].any() and not rec["support"][b, n:].any(), "cut after the arrival"
    assert early == int(sum((paths[b] == targets[b]).any() for b in range(len(seq))))
