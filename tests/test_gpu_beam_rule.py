"""-m gpu: the beam rule (include/irs_hip.h, "beam rule"): irs_beam_search / irs_beam_search_until under irs_set_beam_rule and a
bound beam trace against the step-by-step composition of the public calls (decode, irs_score_target_trace, irs_score_topk_lse,
irs_beam_step_ruled, irs_beam_trace_carry); irs_beam_step_ruled against the CPU statement of tests/beam_rule_ref.py on the
engine's own step inputs and on crafted ones; against irs_beam_step_linked where nothing can fire and lambda is 0; W = 1 against
the greedy loop under irs_set_arrival_rule; what the rule changes; the front end and the rule's lifetime.

Bounds.  Bit for bit wherever both sides run the same launches on the same bytes (the loop and the composition, graph and
stream, the ruled and the linked step, W = 1 and the greedy loop).  Against the CPU statement: links, items, fin, done and
status exact, cum within 1e-9 (the device's log() may differ from libm's in its last bits: tests/test_gpu_beam_trace.py's
bound) -- under the precondition, asserted on the CPU side from the device's own float32 inputs, that no two candidate keys of a
user of which one survives lie within 1e-9 of each other.  The crafted cases use values whose every sum is exact, so there the
ties are exact and the index decides them on both sides.  Where the until loop decodes a compacted batch (check_every = 1) the
rank entries may differ under tests/test_gpu_beam_trace.py's _ranks_agree.

What the CPU statement gives on the oracle's exact logits (tests/test_beam_rule_host.py asserts it): users 0, 2, 3, 6, 10, 11,
W 4, stop rule BEST, P 8 -- without a rule the users are live for 8, 5, 8, 5, 3, 8 steps, with rank_max 10 and lambda 0.5 for
8, 4, 8, 5, 3, 4; the returned beams of every user differ from those under lambda 0."""
import numpy as np
import pytest
import torch

import beam_rule_ref as ref
import test_gpu_beam_trace as bt
from gpu_util import make_engine
from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_BEAM_STOP_ALL, IRS_BEAM_STOP_BEST, IRS_ROW_OFFERED, IRS_SWEEP_BF16
from influentialrs_amd.engine import IrsError
from influentialrs_amd.model.influentialRS import BEAM_STOP_CHECK_EVERY, IRSNN, InfluentialNet, beam_rule_summary, beam_trace_summary

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
USERS6 = [0, 2, 3, 6, 10, 11]
P8 = 8
RULE = (10, None, 0.5)  # rank_max, lp_min, lambda: chosen on the CPU statement (the module's docstring)
NAN, INF = float("nan"), float("inf")
_t, _n, _bits = bt._t, bt._n, bt._bits


def _kw(rule):
    return dict(arrive_rank=rule[0] or None, arrive_lp=rule[1], target_weight=rule[2])


def _loop(eng, seq, usr, hep, W, P, rule, stop=None, check_every=1, k=100, **kw):
    return bt._loop(eng, seq, usr, hep, W, P, stop, check_every=check_every, k=k, **_kw(rule), **kw)


def _compose(eng, seq0, usr0, hep0, W, P, rule, stop=None, k=100, record=None):
    """The ruled search from the public calls: decode -> score_target_trace -> score_topk_lse (W = 1: score_topk) ->
    beam_step_ruled -> beam_trace_carry, P times.  record (a list): per step, numpy copies of the step's inputs and outputs."""
    B, L = seq0.shape
    until = stop is not None
    state = [_t(a) for a in bt.ref.initial_state(seq0, hep0, W, P, until)]
    users = _t(np.repeat(usr0, W))
    arrays = [torch.zeros((B, W, P), dtype=dt, device=DEV) for dt in (torch.float32, torch.float32, torch.int32)]
    done = torch.zeros(B, dtype=torch.int32, device=DEV) if until else None
    status = torch.zeros(B, dtype=torch.int32, device=DEV)
    for i in range(P):
        rows_seq, rows_hep = state[0].view(B * W, L), state[1].view(B * W)
        _, xr, _ = eng.decode(rows_seq, users, want_x=False, pos=rows_hep)
        mx, sm, ts, rk = eng.score_target_trace(xr, rows_seq, rows_hep)
        if W > 1:
            val, ids, _, lmax, lsum = eng.score_topk_lse(xr, k, IRS_SWEEP_BF16)
            lse = (lmax, lsum)
        else:
            val, ids, _ = eng.score_topk(xr, k, IRS_SWEEP_BF16)
            lse = None
        out = [torch.empty_like(t) for t in state]
        done_in, status_in = (_n(done).copy() if until else None), _n(status).copy()
        link, link_val = eng.beam_step_ruled(state, val, ids, lse, i, out, status, mx, sm, ts, rk, done=done,
                                             stop_rule=stop if until else IRS_BEAM_STOP_BEST, rank_max=rule[0], lp_min=rule[1],
                                             target_weight=rule[2])
        eng.beam_trace_carry(link, link_val, mx, sm, ts, rk, i, *arrays)
        if record is not None:
            record.append(dict(state_in=[_n(t) for t in state], done_in=done_in, status_in=status_in, val=_n(val), ids0=_n(ids),
                               lse=(None, None) if lse is None else (_n(lmax), _n(lsum)), sweep=tuple(_n(a) for a in (mx, sm, ts, rk)),
                               state_out=[_n(t) for t in out], done_out=_n(done).copy() if until else None, status_out=_n(status).copy(),
                               link=_n(link), link_val=_n(link_val)))
        state = out
    fin = _n(state[4]) if until else None
    return _n(state[3]), _n(state[2]), _n(status), fin, tuple(_n(a) for a in arrays)


# ============================================================================ 1. the loop equals the composition, bit for bit
@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("stop", [None, IRS_BEAM_STOP_ALL, IRS_BEAM_STOP_BEST])
def test_loop_equals_composition(golden, W, stop):
    g = golden("irn_tiny")
    eng = bt._engine()
    seq, usr, hep = bt._inputs(g, USERS6)
    want = _compose(eng, seq, usr, hep, W, P8, RULE, stop)
    got = _loop(eng, seq, usr, hep, W, P8, RULE, stop, check_every=P8)  # (nothing is compacted: the same launches on the same bytes)
    bt._assert_equal_runs(got, want)
    assert (got[2] & IRS_ROW_OFFERED).any(), "the rule fires for somebody"
    if stop is None:
        graph = _loop(eng, seq, usr, hep, W, P8, RULE, use_graph=True)
        bt._assert_equal_runs(graph, got)
    else:
        every = _loop(eng, seq, usr, hep, W, P8, RULE, stop, check_every=1)  # compacted batches: other decodes
        assert np.array_equal(every[0], got[0]) and np.array_equal(every[3], got[3]) and np.array_equal(every[2], got[2])
        bt._ranks_agree(every[4], got[4])
        for c in (0, 1):
            print(f"check_every 1 array {c}: max difference {np.abs(every[4][c] - got[4][c]).max():.3g}")
            assert np.allclose(every[4][c], got[4][c], rtol=1e-5, atol=2e-5) and np.array_equal(every[4][c] == 0, got[4][c] == 0)


# ============================================================================ 2. the step equals the CPU statement on the engine's inputs
def _against_statement(r, step, P, rule, stop, n_item, **kw):
    """One recorded (or crafted) step against ref.ruled_step: exact but for cum (1e-9)."""
    state_out, link, link_val, done_out, status, offered = ref.ruled_step(r["state_in"], r["done_in"], r["val"], r["ids0"], *r["lse"],
                                                                          r["sweep"], rule, n_item, step, P, stop,
                                                                          status=r["status_in"], **kw)
    for c, (a, b) in enumerate(zip(state_out, r["state_out"])):
        if c == 2:
            assert np.allclose(a, b, rtol=0, atol=1e-9) and np.array_equal(a > -np.inf, b > -np.inf), (step, "cum", a, b)
        else:
            assert np.array_equal(a, b), (step, c, np.argwhere(a != b).tolist()[:5])
    assert np.array_equal(link, r["link"]), (step, link.tolist(), r["link"].tolist())
    assert np.array_equal(_bits(link_val), _bits(r["link_val"])), step
    assert (done_out is None and r["done_out"] is None) or np.array_equal(done_out, r["done_out"]), step
    assert np.array_equal(status, r["status_out"]), (step, status, r["status_out"])
    return offered


@pytest.mark.parametrize("lam", [0.5, 4.0])
@pytest.mark.parametrize("stop", [None, IRS_BEAM_STOP_ALL])
def test_step_equals_the_cpu_statement_on_the_engines_own_inputs(golden, lam, stop):
    g = golden("irn_tiny")
    eng = bt._engine()
    cfg = synth.make_config("tiny")
    seq, usr, hep = bt._inputs(g, USERS6)
    W, rule = 4, (10, None, lam)
    rec = []
    _compose(eng, seq, usr, hep, W, P8, rule, stop, record=rec)
    fired = 0
    for i, r in enumerate(rec):
        gap = ref.min_key_gap(r["state_in"], r["done_in"], r["val"], r["ids0"], *r["lse"], r["sweep"], rule, cfg.n_item, i)
        print(f"lambda {lam} step {i}: smallest key gap next to a survivor {gap:.3g}")
        assert gap > 1e-9, "precondition: choose other users"
        fired += int(_against_statement(r, i, P8, rule, stop, cfg.n_item).sum())
    assert fired >= 2


# ============================================================================ 3. crafted steps: every branch at its smallest shape
def _craft(B=2, W=3, L=12, P=4, k=5, until=True):
    """Exact values throughout: lists 2, 1.5, 1, ... on ids0 20.., lse pair (2, 1) -> norm 2, sweep (2, 1, -1, rank 50) -> lp_target
    -3, target 7, windows of items 100.. that no list holds, scores -0.25 j - b."""
    seq = np.zeros((B, W, L), dtype=np.int64)
    seq[:, :, L - 12:L - 1] = 100 + np.arange(11)
    seq[:, :, L - 1] = 7
    hep = np.full((B, W), L - 2, dtype=np.int32)
    cum = -0.25 * np.arange(W)[None, :] - np.arange(B)[:, None].astype(np.float64)
    paths = np.zeros((B, W, P), dtype=np.float32)
    paths[:, :, 0] = 50 + np.arange(W)
    state = [seq, hep, cum, paths] + ([np.zeros((B, W), dtype=np.int32)] if until else [])
    val = np.tile((2.0 - 2.0 ** -5 * np.arange(k) * (16 if k <= 8 else 1)).astype(np.float32), (B * W, 1))
    ids0 = np.tile(20 + np.arange(k, dtype=np.int64), (B * W, 1))
    f = lambda v: np.full(B * W, v, dtype=np.float32)  # noqa: E731
    return dict(state_in=state, done_in=np.zeros(B, dtype=np.int32) if until else None, status_in=np.zeros(B, dtype=np.int32), val=val,
                ids0=ids0, lse=(f(2.0), f(1.0)) if W > 1 else (None, None), sweep=(f(2.0), f(1.0), f(-1.0), np.full(B * W, 50, dtype=np.int32)))


def _run_crafted(eng, c, step, rule, stop, n_item, excl=None, no_repeat=False, offer=None):
    """c through irs_beam_step_ruled under the given bindings, then against the statement.  Returns the offered bits."""
    state = [_t(a) for a in c["state_in"]]
    out = [torch.empty_like(t) for t in state]
    done = None if c["done_in"] is None else _t(c["done_in"])
    status = _t(c["status_in"])
    lse = None if c["lse"][0] is None else tuple(_t(a) for a in c["lse"])
    B, W, P = c["state_in"][3].shape
    held = []
    try:
        if excl is not None or no_repeat:
            held.append(eng.bind_exclusions(None if excl is None else _t(excl), B, no_repeat))
        if offer is not None:
            held.append(eng.bind_offer_set(_t(np.asarray(offer, dtype=np.int64)), B * W))
        link, link_val = eng.beam_step_ruled(state, _t(c["val"]), _t(c["ids0"]), lse, step, out, status, *(_t(a) for a in c["sweep"]),
                                             done=done, stop_rule=IRS_BEAM_STOP_ALL if stop is None else stop, rank_max=rule[0],
                                             lp_min=rule[1], target_weight=rule[2])
        torch.cuda.synchronize()
    finally:
        if excl is not None or no_repeat:
            eng.unbind_exclusions()
        if offer is not None:
            eng.unbind_offer_set()
    c = dict(c, state_out=[_n(t) for t in out], done_out=None if done is None else _n(done), status_out=_n(status), link=_n(link),
             link_val=_n(link_val))
    return _against_statement(c, step, P, rule, stop, n_item, excl=excl, no_repeat=no_repeat, offer=offer), c


CASES = ["fires_on_one_beam", "target_in_window", "target_in_list", "target_on_own_path", "target_outside_offer_set", "no_target",
         "nan_sumexp", "finished_beam", "dead_beam", "done_user", "k_1", "plain_form", "W_1", "W_32", "long_window"]


@pytest.mark.parametrize("case", CASES)
def test_crafted_step_cases(case):
    cfg = synth.make_config("tiny")
    N, ALL = cfg.n_item, IRS_BEAM_STOP_ALL
    eng = bt._engine(16, max_len=320) if case == "long_window" else bt._engine()
    rule, stop, kw, step = (2, None, 1.0), ALL, {}, 1
    c = _craft(L=320) if case == "long_window" else _craft()
    seq, _, cum, paths = c["state_in"][:4]
    mx, sm, ts, rank = c["sweep"]
    W = seq.shape[1]
    # in every case: user 0's beam 0 has lp_target -3.5, so that its children (0 - 3.5, -0.5 - 3.5) and beam 2's (-0.5 - 3, -1 - 3)
    # tie on the key pair by pair and the index decides between two parents
    ts[0] = -1.5
    if case == "fires_on_one_beam":
        rank[1], ts[1] = 1, 2.0  # lp_target 0: the target's key -0.25 + (2 - 2) + 0 is the best of the user
        want = [[False, True, False], [False] * 3]
    elif case == "target_in_window":
        rank[:] = 1
        seq[0, 0, 5] = 7
        want = [[False, True, True], [True] * 3]
    elif case == "target_in_list":
        rank[:] = 1
        kw = dict(excl=np.array([[3, 6], [-1, -1]], dtype=np.int64))
        want = [[False] * 3, [True] * 3]
    elif case == "target_on_own_path":
        rank[:] = 1
        paths[0, 1, 0] = 7
        kw = dict(no_repeat=True)
        want = [[True, False, True], [True] * 3]
    elif case == "target_outside_offer_set":
        rank[:] = 1
        kw = dict(offer=[5, 20, 21, 22, 23, 24, 30])
        want = [[False] * 3] * 2
    elif case == "no_target":
        rank[:] = 0
        rule = (2, -INF, 1.0)
        want = [[False] * 3] * 2
    elif case == "nan_sumexp":
        sm[[0, 4]] = NAN
        rule = (0, -INF, 1.0)
        want = [[False, True, True], [True, False, True]]
    elif case == "finished_beam":
        c["state_in"][4][0, 0] = 1
        paths[0, 0, 0] = 7
        rank[2] = 2
        want = [[False, False, True], [False] * 3]
    elif case == "dead_beam":
        cum[0, 2] = -np.inf
        rank[:] = 1
        want = [[True, True, False], [True] * 3]
    elif case == "done_user":
        c["done_in"][1] = 1
        rank[:] = 1
        want = [[True] * 3, [False] * 3]
    elif case == "k_1":
        c = dict(c, val=c["val"][:, :1].copy(), ids0=c["ids0"][:, :1].copy())
        rank[4] = 2
        want = [[False] * 3, [False, True, False]]
    elif case == "plain_form":
        c = dict(_craft(until=False), sweep=c["sweep"])
        rank[1] = 1
        stop = None
        want = [[False, True, False], [False] * 3]
    elif case == "W_1":
        c = _craft(B=3, W=1)
        c["sweep"][3][1] = 2
        want = [[False], [True], [False]]
    elif case == "W_32":  # 32 x 32 candidates fill the LDS arrays; scores -0.25 j + 2^-5 c: ties between many parents
        c = _craft(B=2, W=32, k=34)
        c["sweep"][3][[3, 40]] = 1
        c["sweep"][2][:32] = -1.0 - 0.25 * (np.arange(32) % 3)
        want = np.zeros((2, 32), dtype=bool)
        want[0, 3] = want[1, 8] = True
    elif case == "long_window":  # the target stands in window slot 300 of beam 0: only the 16-register image sees it
        rank[:] = 1
        seq[0, 0, 300] = 7
        want = [[False, True, True], [True] * 3]
    offered, got = _run_crafted(eng, c, step, rule, stop, N, **kw)
    assert np.array_equal(offered, np.asarray(want, dtype=bool)), offered.tolist()
    assert np.array_equal((got["status_out"] & IRS_ROW_OFFERED) != 0, offered.any(axis=1))
    link = got["link"]
    if case == "fires_on_one_beam":  # the fired beam gave ONE child, the best; the tie between two parents went to the lower index
        assert link[0].tolist() == [1, 0, 2] and got["state_out"][3][0, :, 1].tolist() == [7, 21, 21], (link[0], got["state_out"][3][0])
        assert got["state_out"][4][0].tolist() == [1, 0, 0] and got["state_out"][2][0].tolist() == [-0.25, 0.0, -0.5]
    if case == "finished_beam":
        assert link[0, 0] == (ref.COPY | 0) and got["state_out"][4][0].tolist() == [1, 0, 0]
    if case == "done_user":
        assert link[1].tolist() == [ref.COPY | j for j in range(W)]
    if case == "no_target":  # bonus 0: the key is the score, the order the linked step's
        assert link[0].tolist() == [0, 1, 0]


def test_crafted_fired_beam_under_the_until_form_is_finished_and_stops_under_best():
    eng = bt._engine()
    c = _craft()
    c["sweep"][3][:] = 1
    _, got = _run_crafted(eng, c, 1, (1, None, 0.0), IRS_BEAM_STOP_BEST, synth.make_config("tiny").n_item)
    assert got["state_out"][4].all() and got["done_out"].all() and (got["state_out"][3][:, :, 1] == 7).all()
    assert np.array_equal(_bits(got["link_val"]), _bits(np.full((2, 3), -1.0, dtype=np.float32)))


# ============================================================================ 4. lambda 0 and nothing that can fire: the linked step
@pytest.mark.parametrize("W,stop", [(4, None), (4, IRS_BEAM_STOP_ALL), (1, IRS_BEAM_STOP_BEST)])
def test_with_lambda_0_and_no_clause_that_can_hold_the_ruled_step_is_the_linked_step(golden, W, stop):
    """irs_beam_step_ruled refuses all three off (IRS_E_INVALID), so the clauses are made unable to hold: once by ranks of 0 (no
    target) under an always-true probability clause, once by the engine's own sweep values with every rank moved beyond rank_max."""
    g = golden("irn_tiny")
    eng = bt._engine()
    seq, usr, hep = bt._inputs(g, USERS6)
    rec = []
    _compose(eng, seq, usr, hep, W, 3, (0, None, 0.5), stop, record=rec)  # a few real steps to take inputs from
    for i, r in enumerate(rec):
        lse = None if r["lse"][0] is None else tuple(_t(a) for a in r["lse"])
        outs = []
        mx, sm, ts, rk = r["sweep"]
        for sweep, rule in (((mx, sm, ts, np.zeros_like(rk)), dict(rank_max=5, lp_min=-INF)), ((mx, sm, ts, np.where(rk > 0, rk + 1000, 0).astype(np.int32)), dict(rank_max=1000)), (None, None)):
            state = [_t(a) for a in r["state_in"]]
            out = [torch.empty_like(t) for t in state]
            done = None if r["done_in"] is None else _t(r["done_in"])
            status = _t(r["status_in"])
            common = dict(done=done, stop_rule=stop if stop is not None else IRS_BEAM_STOP_BEST)
            if rule is None:
                link = eng.beam_step_linked(state, _t(r["val"]), _t(r["ids0"]), lse, i, out, status, **common)
            else:
                link = eng.beam_step_ruled(state, _t(r["val"]), _t(r["ids0"]), lse, i, out, status, *(_t(a) for a in sweep), **common, **rule)
            outs.append([_n(t) for t in out] + [_n(a) for a in link] + [_n(status)] + ([] if done is None else [_n(done)]))
        for ruled in outs[:2]:
            assert len(ruled) == len(outs[2]) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ruled, outs[2])), i
    state = [_t(a) for a in rec[0]["state_in"]]
    with pytest.raises(IrsError, match=r"error -1\b.*all clauses are off"):
        eng.beam_step_ruled(state, _t(rec[0]["val"]), _t(rec[0]["ids0"]), lse, 0, [torch.empty_like(t) for t in state],
                            _t(rec[0]["status_in"]), *(_t(a) for a in rec[0]["sweep"]), done=None if stop is None else _t(rec[0]["done_in"]))


# ============================================================================ 5. W = 1 with a rule is the greedy loop under the arrival rule
@pytest.mark.parametrize("rank_max,lp_min", [(10, None), (None, -4.0), (10, -4.0)])
def test_one_beam_with_a_rule_equals_the_greedy_loop_under_the_arrival_rule(golden, rank_max, lp_min):
    g = golden("irn_tiny")
    eng = bt._engine()
    seq, usr, hep = bt._inputs(g, USERS6)
    got = _loop(eng, seq, usr, hep, 1, P8, (rank_max, lp_min, 0.0), IRS_BEAM_STOP_BEST, check_every=P8)
    paths, status, _, _, tr = eng.generate_paths_until(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16, check_every=P8, trace=True,
                                                       arrive_rank=rank_max, arrive_lp=lp_min)
    assert np.array_equal(got[0][:, 0], _n(paths)) and np.array_equal(got[2], _n(status)) and (got[2] & IRS_ROW_OFFERED).any()
    assert bt._same_bits([a[:, 0] for a in got[4]], [_n(a) for a in tr])
    plain = _loop(eng, seq, usr, hep, 1, P8, (rank_max, lp_min, 0.0))  # the plain forms search on behind the arrival
    paths_p, status_p, tr_p = eng.generate_paths(_t(seq), _t(usr), _t(hep), P8, k=100, sweep=IRS_SWEEP_BF16, trace=True, arrive_rank=rank_max,
                                                 arrive_lp=lp_min)
    assert np.array_equal(plain[0][:, 0], _n(paths_p)) and np.array_equal(plain[2], _n(status_p))
    assert bt._same_bits([a[:, 0] for a in plain[4]], [_n(a) for a in tr_p])


# ============================================================================ 6. the rule does something
def _done_step(run, targets):
    """Under BEST a user is done at the step its beam 0 chose the target (P: never)."""
    paths = run[0]
    return np.array([next((i + 1 for i in range(paths.shape[2]) if paths[b, 0, i] == targets[b]), paths.shape[2]) for b in range(len(targets))])


def test_the_rule_does_something(golden):
    g = golden("irn_tiny")
    eng = bt._engine()
    seq, usr, hep = bt._inputs(g, USERS6)
    targets = seq[:, -1]
    W, BEST = 4, IRS_BEAM_STOP_BEST
    base = bt._loop(eng, seq, usr, hep, W, P8, BEST, check_every=P8)
    arrive = _loop(eng, seq, usr, hep, W, P8, (RULE[0], None, 0.0), BEST, check_every=P8)
    both = _loop(eng, seq, usr, hep, W, P8, RULE, BEST, check_every=P8)
    steps = [_done_step(r, targets) for r in (base, arrive, both)]
    print("done at step, no rule / arrival / arrival + weight:", [s.tolist() for s in steps], "status", both[2].tolist())
    assert (steps[2] < steps[0]).any(), "somebody finishes earlier than without the rule"
    assert any(not np.array_equal(both[0][b], arrive[0][b]) for b in range(len(USERS6))), "somebody's returned beams differ from lambda 0"
    assert not base[2].any()
    lp_i, lp_t, rk = both[4]
    bts = beam_trace_summary(lp_i, lp_t, rk, both[0], both[1], targets)
    extra = beam_rule_summary(bts, targets, RULE[0], RULE[1])
    offered, at = extra["offered"], extra["arrival_step"]
    want, at_ref = ref.replay_offered(both[0], lp_t, rk, targets, RULE[0], RULE[1])
    live = both[1] > -np.inf
    assert np.array_equal(offered, want & live) and np.array_equal(at, np.where(live, at_ref, -1)) and offered.sum() >= 2
    for b, j in zip(*np.where(offered)):  # an offered beam: lp_item == lp_target bit for bit at its arrival step, and it ended there
        assert _bits(lp_i)[b, j, at[b, j]] == _bits(lp_t)[b, j, at[b, j]] and both[3][b, j] == 1 and rk[b, j, at[b, j]] <= RULE[0]
    assert np.array_equal(offered.any(axis=1), (both[2] & IRS_ROW_OFFERED) != 0), (offered.tolist(), both[2].tolist())
    # scores are acceptance sums: each equals its own beam's recorded lp_item sum within the two log-sum-exps' tolerance
    for b in range(len(USERS6)):
        for j in range(W):
            if live[b, j]:
                n = int(bts["n_steps"][b, j])
                assert abs(float(bts["lp_item"][b, j, :n].astype(np.float64).sum()) - both[1][b, j]) <= n * 2e-5, (b, j)


# ============================================================================ 7. the front end and the rule's lifetime
def test_front_end_takes_the_keywords_and_refuses_without_the_trace(golden):
    g = golden("irn_tiny")
    cfg = synth.make_config("tiny")
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    net.to(DEV)
    irn = IRSNN(cfg, net, DEV).eval()
    seq, usr, tgt = (torch.from_numpy(g[k][USERS6]).to(DEV) for k in ("seqs", "users", "targets"))
    B, W = len(USERS6), 4
    kw = dict(beam_width=W, beam_stop="best", beam_arrive_rank=RULE[0], beam_target_weight=RULE[2])
    with torch.no_grad():
        with pytest.raises(IrsError, match=r"error -2\b.*irs_set_beam_rule.*irs_bind_beam_trace"):
            irn.get_seq_in_batch(seq, usr, tgt, P8, 0, **kw)
        plain = irn.get_seq_in_batch(seq, usr, tgt, P8, 0, beam_width=W, beam_stop="best", beam_trace=True)
        assert sorted(irn.last_beam_trace) == ["lp_item", "lp_target", "n_steps", "paths", "picked", "rank_target", "scores"]
        ruled = irn.get_seq_in_batch(seq, usr, tgt, P8, 0, beam_trace=True, **kw)
        lbt = irn.last_beam_trace
        again = irn.get_seq_in_batch(seq, usr, tgt, P8, 0, beam_width=W, beam_stop="best", beam_trace=True)
    assert sorted(lbt) == ["arrival_step", "lp_item", "lp_target", "n_steps", "offered", "paths", "picked", "rank_target", "scores"]
    assert lbt["offered"].shape == (B, W) and lbt["offered"].dtype == bool and lbt["arrival_step"].shape == (B, W)
    assert np.array_equal(plain[0], again[0]) and plain[3] == again[3], "the rule lasts for the call"
    assert ruled[3] >= plain[3] and lbt["offered"].any()
    # the same search through the engine: its status bit per user is what `offered` says
    eng = net._hip.get(B * W, B * W)
    hep = torch.full((B,), cfg.max_len - 2, dtype=torch.int32, device=DEV)
    out = eng.beam_search_until(seq.contiguous(), usr, hep, P8, W, k=100, sweep=net._hip.sweep, stop_rule=IRS_BEAM_STOP_BEST, trace=True,
                                check_every=BEAM_STOP_CHECK_EVERY, **_kw(RULE))
    assert np.array_equal(_n(out[0]), lbt["paths"]) and np.array_equal(lbt["offered"].any(axis=1), (_n(out[2]) & IRS_ROW_OFFERED) != 0)
    arrived = lbt["arrival_step"] >= 0
    assert np.array_equal(arrived, (lbt["paths"] == g["targets"][USERS6][:, None, None]).any(axis=2) & (lbt["scores"] > -np.inf))


def test_clearing_restores_the_bytes_and_a_rule_change_recaptures(golden):
    g = golden("irn_tiny")
    eng = bt._engine()
    seq, usr, hep = bt._inputs(g, USERS6)
    B, W = len(seq), 4
    cfg = synth.make_config("tiny")

    def search(e, graph=True):
        return [_n(t) for t in e.beam_search(_t(seq), _t(usr), _t(hep), P8, W, k=100, sweep=IRS_SWEEP_BF16, use_graph=graph)[:3]]
    before = search(eng)
    until_before = [_n(t) for t in eng.beam_search_until(_t(seq), _t(usr), _t(hep), P8, W, k=100, sweep=IRS_SWEEP_BF16)[:4]]
    held = eng.bind_beam_trace(B, W, P8)
    try:
        traced = search(eng)
        eng.set_beam_rule(10, None, 0.5)
        first = search(eng) + [_n(a).copy() for a in held[:3]]
        eng.set_beam_rule(3, None, 4.0)  # another rule between two use_graph calls: the captured steps are dropped
        second = search(eng) + [_n(a).copy() for a in held[:3]]
        with pytest.raises(IrsError, match=r"error -4\b.*irs_generate_paths: a beam trace is bound"):
            eng.generate_paths(_t(seq), _t(usr), _t(hep), P8)
        eng.set_beam_rule(None, None, 0.0)
        cleared = search(eng)
    finally:
        eng.set_beam_rule(None, None, 0.0)
        eng.unbind_beam_trace()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, traced)) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, cleared))
    assert not np.array_equal(first[0], second[0]) and not np.array_equal(first[0], before[0])
    fresh = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=128, max_seqs=128)
    for rule, got in (((10, None, 0.5), first), ((3, None, 4.0), second)):
        want = _loop(fresh, seq, usr, hep, W, P8, rule)  # stream launches on an engine that never captured anything
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got[:3], want[:3])), rule
        assert bt._same_bits(got[3:], want[4]), rule
    # a rule set by hand and no trace: refused before any launch; cleared: the loops return what they returned before it was set
    eng.set_beam_rule(10, None, 0.5)
    try:
        with pytest.raises(IrsError, match=r"error -2\b.*irs_beam_search: a beam rule is set \(irs_set_beam_rule\) and no beam trace is bound"):
            search(eng)
        with pytest.raises(IrsError, match=r"error -4\b.*irs_generate_paths: a beam rule is set"):
            eng.generate_paths(_t(seq), _t(usr), _t(hep), P8)
    finally:
        eng.set_beam_rule(None, None, 0.0)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, search(eng)))
    until_after = [_n(t) for t in eng.beam_search_until(_t(seq), _t(usr), _t(hep), P8, W, k=100, sweep=IRS_SWEEP_BF16)[:4]]
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(until_before, until_after))
