"""Beam rule, the parts that need no GPU: properties of the numpy statement (tests/beam_rule_ref.py) on the oracle's logits of the
tiny golden, the statement by hand, the new symbols in header, library and ctypes table, the setter's and the stand-alone step's
argument checks and every entry point's answer while a rule is set (through the library, on contexts created without a device,
as tests/test_search_options_host.py does), and the front end's keywords."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arrival_ref  # noqa: E402
import beam_rule_ref as ref  # noqa: E402
import beam_trace_ref  # noqa: E402
import beam_until_ref  # noqa: E402
import test_search_options_host as options_host  # noqa: E402

from influentialrs_amd import _lib, synth  # noqa: E402
from influentialrs_amd.model.influentialRS import (IRSNN, InfluentialNet, SearchOptions, beam_rule_kwargs, beam_rule_summary,  # noqa: E402
                                                   search_option_kwargs)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, UNSUPPORTED = -1, -2, -4
NAN, INF = float("nan"), float("inf")
P_ = ctypes.c_void_p(4096)  # a fake non-null address: every call here is refused before anything is dereferenced or launched
USERS6 = [0, 2, 3, 6, 10, 11]
P8 = 8
DEAD, COPY = ref.DEAD, ref.COPY
_CACHE = {}


def _ctx(world=1):
    return options_host._ctx(world)


def _model(golden):
    g = golden("irn_tiny")
    cfg = synth.make_config("tiny")
    sd = synth.irn_state_dict(cfg, 1234)
    seqs, users = g["seqs"][USERS6], g["users"][USERS6]
    return cfg, sd, seqs, users, np.full(len(USERS6), cfg.max_len - 2, dtype=np.int32)


def _search(oracle, golden, W, rule, stop_rule):
    cfg, sd, seqs, users, hep0 = _model(golden)
    key = (W, rule, stop_rule)
    if key not in _CACHE:
        _CACHE[key] = ref.search(oracle, sd, cfg, seqs, users, hep0, W, P8, rule, stop_rule=stop_rule, cache=_CACHE.setdefault("rows", {}))
    return _CACHE[key]


# ---------------------------------------------------------------- the statement on the oracle's logits
@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("stop_rule", [0, 1])
def test_all_clauses_off_is_the_until_step_exactly(oracle, golden, W, stop_rule):
    cfg, sd, seqs, users, _ = _model(golden)
    got = _search(oracle, golden, W, (0, None, 0.0), stop_rule)
    paths, scores, fins, steps = beam_until_ref.beam_search_until(oracle, sd, cfg, seqs, users, P8, W, stop_rule)
    assert np.array_equal(got["paths"], paths) and np.array_equal(got["scores"].view(np.uint64), scores.view(np.uint64))
    assert np.array_equal(got["fin"], fins) and np.array_equal(got["steps"], steps)
    assert not got["status"].any() and not got["offered"].any() and not got["offered_own"].any()


def test_one_step_with_the_clauses_off_equals_the_until_step_and_its_links():
    rng = np.random.default_rng(3)
    B, W, L, P, k, N = 3, 3, 6, 4, 5, 40
    seq = rng.integers(1, 9, (B, W, L)).astype(np.int64)
    hep = np.full((B, W), L - 2, dtype=np.int32)
    cum = -rng.random((B, W))
    cum[1, 2] = -np.inf
    paths = np.zeros((B, W, P), dtype=np.float32)
    paths[:, :, 0] = seq[:, :, L - 2]
    fin = np.zeros((B, W), dtype=np.int32)
    fin[0, 1] = 1
    done = np.array([0, 0, 1], dtype=np.int32)
    val = -np.sort(rng.random((B * W, k)).astype(np.float32), axis=1)
    ids0 = np.stack([rng.permutation(N)[:k] for _ in range(B * W)]).astype(np.int64)
    lmax, lsum = np.zeros(B * W, dtype=np.float32), np.full(B * W, 7.5, dtype=np.float32)
    sweep = (lmax, lsum, np.full(B * W, -2.0, dtype=np.float32), np.full(B * W, 3, dtype=np.int32))
    want, done_w, status_w = beam_until_ref.beam_step_until((seq, hep, cum, paths, fin), done, val, ids0, lmax, lsum, 1, P, 0)
    link_w, val_w, _ = beam_trace_ref.step_links((seq, hep, cum, paths, fin), done, val, ids0, lmax, lsum, True)
    got, link, link_val, done_g, status, offered = ref.ruled_step((seq, hep, cum, paths, fin), done, val, ids0, lmax, lsum, sweep,
                                                                   (0, None, 0.0), N, 1, P, 0)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(link, link_w) and np.array_equal(link_val, val_w) and np.array_equal(done_g, done_w)
    assert np.array_equal(status, status_w) and not offered.any()


def test_one_beam_is_the_greedy_search_under_the_arrival_rule_id_for_id(oracle, golden):
    cfg, sd, seqs, users, hep0 = _model(golden)
    off = _search(oracle, golden, 1, (0, None, 0.0), 1)
    rank_max, lp_min = 10, -4.0
    fired_somewhere = False
    for rule in ((rank_max, None), (0, lp_min), (rank_max, lp_min)):
        want, trace, n_steps, arrived, offered = arrival_ref.replay(seqs, hep0, off["paths"][:, 0], tuple(a[:, 0] for a in off["arrays"]),
                                                                    rule[0], NAN if rule[1] is None else rule[1], cfg.n_item)
        got = _search(oracle, golden, 1, rule + (0.0,), 1)
        assert np.array_equal(got["paths"][:, 0], want), rule
        for a, b in zip(got["arrays"], trace):
            assert np.array_equal(a[:, 0].view(np.uint32), b.view(np.uint32)), rule
        assert np.array_equal(got["fin"][:, 0] != 0, arrived) and np.array_equal(got["offered_own"][:, 0], offered)
        assert np.array_equal(got["status"] != 0, offered)
        # a weight changes nothing where there is one beam: one parent, one term common to all its children
        again = _search(oracle, golden, 1, rule + (4.0,), 1)
        assert np.array_equal(again["paths"], got["paths"]) and np.array_equal(again["scores"], got["scores"])
        fired_somewhere |= bool(offered.any())
    assert fired_somewhere


@pytest.mark.parametrize("W", [2, 4])
def test_an_always_true_clause_ends_every_admissible_user_at_step_0(oracle, golden, W):
    cfg, sd, seqs, users, hep0 = _model(golden)
    got = _search(oracle, golden, W, (0, -INF, 0.0), 0)
    adm = np.array([arrival_ref.admissible(s[-1], s[:h + 1], cfg.n_item) for s, h in zip(seqs, hep0)])
    assert adm.any()
    for b in range(len(seqs)):
        if adm[b]:
            assert got["steps"][b] == 1 and got["fin"][b].tolist() == [1] + [0] * (W - 1)
            assert got["paths"][b, 0].tolist() == [seqs[b, -1]] + [0] * (P8 - 1)
            assert not (got["scores"][b, 1:] > -np.inf).any() and not got["paths"][b, 1:].any()
            assert got["status"][b] == arrival_ref.OFFERED and got["offered_own"][b].tolist() == [True] + [False] * (W - 1)
            assert got["arrays"][0][b, 0, 0] == got["arrays"][1][b, 0, 0] < 0  # lp_item == lp_target at the fired step


@pytest.mark.parametrize("W,stop_rule,rule", [(4, 1, (10, None, 0.5)), (4, 0, (5, None, 4.0)), (2, 1, (3, -6.0, 0.5)), (4, None, (10, None, 0.0))])
def test_replaying_offered_from_the_arrays_reproduces_the_statements_own_bits(oracle, golden, W, stop_rule, rule):
    got = _search(oracle, golden, W, rule, stop_rule)
    assert got["offered_own"].any(), "the case shows something"
    assert np.array_equal(got["offered"], got["offered_own"])
    lp_i, lp_t, rk = got["arrays"]
    targets = _model(golden)[2][:, -1]
    _, at = ref.replay_offered(got["paths"], lp_t, rk, targets, rule[0], rule[1])
    for b, j in zip(*np.where(got["offered"])):
        assert lp_i[b, j, at[b, j]].view(np.uint32) == lp_t[b, j, at[b, j]].view(np.uint32)
    # the front end's host summary says the same from the same arrays
    from influentialrs_amd.model.influentialRS import beam_trace_summary
    bt = beam_trace_summary(lp_i, lp_t, rk, got["paths"], got["scores"], targets)
    extra = beam_rule_summary(bt, targets, rule[0], rule[1])
    live = got["scores"] > -np.inf
    assert np.array_equal(extra["offered"], got["offered"] & live) and np.array_equal(extra["arrival_step"], np.where(live, at, -1))


def test_the_rule_does_something(oracle, golden):
    """What tests/test_gpu_beam_rule.py asserts on the device, here on the oracle's exact logits: W 4, stop rule BEST, rank_max
    10, lambda 0.5 on users 0, 2, 3, 6, 10, 11."""
    base = _search(oracle, golden, 4, (0, None, 0.0), 1)
    arrive = _search(oracle, golden, 4, (10, None, 0.0), 1)
    both = _search(oracle, golden, 4, (10, None, 0.5), 1)
    print("steps without / with the rule:", base["steps"].tolist(), both["steps"].tolist())
    assert (both["steps"] < base["steps"]).any(), "somebody finishes earlier"
    assert any(not np.array_equal(both["paths"][b], arrive["paths"][b]) for b in range(len(USERS6))), "the weight changes a beam set"
    assert np.array_equal(both["offered"].any(axis=1), (both["status"] & arrival_ref.OFFERED) != 0)
    # scores stay acceptance sums: with a weight they need not be descending, and here they are not
    live = both["scores"] > -np.inf
    assert any((np.diff(both["scores"][b][live[b]]) > 0).any() for b in range(len(USERS6)))


# ---------------------------------------------------------------- the statement, by hand
def _hand():
    """Two users, W = 2, L = 5, window items 90..; beam 0 and beam 1 of user 0 are live with equal scores, user 1 has one live
    beam.  Lists: items 21, 22, 23 with values 2, 1, 0.5; lse pair (2, 1) -> norm 2."""
    W, L, P, k = 2, 5, 4, 3
    seq = np.full((2, W, L), 90, dtype=np.int64)
    seq[:, :, L - 1] = 7
    hep = np.full((2, W), L - 2, dtype=np.int32)
    cum = np.array([[-1.0, -1.0], [0.0, -np.inf]])
    paths = np.zeros((2, W, P), dtype=np.float32)
    val = np.tile(np.array([2.0, 1.0, 0.5], dtype=np.float32), (2 * W, 1))
    ids0 = np.tile(np.array([20, 21, 22], dtype=np.int64), (2 * W, 1))
    lmax, lsum = np.full(2 * W, 2.0, dtype=np.float32), np.ones(2 * W, dtype=np.float32)
    return (seq, hep, cum, paths), val, ids0, lmax, lsum


def test_by_hand_fire_on_one_beam_weight_reorders_and_the_index_breaks_a_tie():
    state, val, ids0, lmax, lsum = _hand()
    ts = np.array([-1.0, -3.0, -2.0, 0.0], dtype=np.float32)
    rank = np.array([2, 9, 5, 0], dtype=np.int32)
    sweep = (lmax, lsum, ts, rank)  # lp_target = ts - 2: -3, -5, -4
    # rank_max 2: beam 0 of user 0 fires (one candidate: the target at -1 + (-1 - 2) = -4); beam 1 walks: -1, -2
    out, link, link_val, done, status, offered = ref.ruled_step(state, None, val, ids0, lmax, lsum, sweep, (2, None, 0.0), 40, 0, 4)
    assert offered.tolist() == [[True, False], [False, False]] and status.tolist() == [arrival_ref.OFFERED, 0]
    assert out[3][0, :, 0].tolist() == [21, 22] and link[0].tolist() == [1, 1] and out[2][0].tolist() == [-1.0, -2.0]
    # lambda 1: keys are -4 - 3 = -7 for the target, -1 - 5 = -6 and -2 - 5 = -7 for beam 1's children: the tie at -7 goes to the
    # lower index, the fired beam's 0 * W + 0
    out, link, link_val, _, _, _ = ref.ruled_step(state, None, val, ids0, lmax, lsum, sweep, (2, None, 1.0), 40, 0, 4)
    assert out[3][0, :, 0].tolist() == [21, 7] and link[0].tolist() == [1, 0] and out[2][0].tolist() == [-1.0, -4.0]
    assert link_val[0].tolist() == [2.0, -1.0]
    # no clause, lambda 1: beam 0's children carry -3, beam 1's -5: both survivors come from beam 0, scores unchanged
    out, link, _, _, status, offered = ref.ruled_step(state, None, val, ids0, lmax, lsum, sweep, (0, None, 1.0), 40, 0, 4)
    assert link[0].tolist() == [0, 0] and out[2][0].tolist() == [-1.0, -2.0] and not status.any() and not offered.any()
    # user 1: rank 5 > 2 does not fire; its dead beam stays dead
    assert link[1].tolist() == [0, 0] and out[3][1, :, 0].tolist() == [21, 22]


def test_by_hand_what_never_fires_and_what_the_bonus_is_then():
    state, val, ids0, lmax, lsum = _hand()
    seq = state[0]
    ts = np.full(4, -1.0, dtype=np.float32)
    rank = np.ones(4, dtype=np.int32)
    always = (1, -INF, 0.0)

    def fired(state=state, sweep=None, **kw):
        return ref.ruled_step(state, None, val, ids0, lmax, lsum, sweep or (lmax, lsum, ts, rank), always, 40, 1, 4, **kw)[5]
    assert fired().tolist() == [[True, True], [True, False]]
    in_window = seq.copy()
    in_window[0, 0, 2] = 7
    assert fired((in_window,) + state[1:]).tolist() == [[False, True], [True, False]]
    behind_hep = (in_window, np.where(np.arange(2)[:, None] == 0, 1, state[1]).astype(np.int32)) + state[2:]
    assert fired(behind_hep)[0, 0], "a slot behind hep does not count"
    assert fired(excl=np.array([[6, -1], [-1, -1]])).tolist() == [[False, False], [True, False]]
    walked = state[3].copy()
    walked[0, 1, 0] = 7
    assert fired(state[:3] + (walked,), no_repeat=True).tolist() == [[True, False], [True, False]]
    assert not fired(offer=[3, 4, 20, 21, 22]).any() and fired(offer=[6]).tolist() == [[True, True], [True, False]]
    outside = seq.copy()
    outside[:, :, -1] = 41
    assert not fired((outside,) + state[1:]).any()
    assert not fired(sweep=(lmax, lsum, ts, np.zeros(4, dtype=np.int32))).any(), "rk = 0: no target"
    # a NaN lp_target fires by rank only, and weighs nothing
    nan_sum = np.full(4, NAN, dtype=np.float32)
    assert not ref.ruled_step(state, None, val, ids0, lmax, lsum, (lmax, nan_sum, ts, rank), (0, -INF, 0.0), 40, 1, 4)[5].any()
    assert ref.bonus(-1.0, 2.0, NAN, 1) == 0.0 and ref.bonus(-1.0, 2.0, 1.0, 0) == 0.0 and ref.bonus(-1.0, 2.0, 1.0, 1) == -3.0
    assert ref.key_of(-2.0, 0.0, -INF) == -2.0 and ref.key_of(-2.0, 0.5, -4.0) == -4.0


def test_by_hand_finished_dead_and_done():
    (seq, hep, cum, paths), val, ids0, lmax, lsum = _hand()
    fin = np.array([[1, 0], [0, 0]], dtype=np.int32)
    paths = paths.copy()
    paths[0, 0, 0] = 7
    done = np.array([0, 1], dtype=np.int32)
    ts, rank = np.full(4, -1.0, dtype=np.float32), np.full(4, 50, dtype=np.int32)
    # lambda 1, lp_target -3: the finished beam 0 (score -1, bonus 0, key -1) against beam 1's children with keys -1 - 3, -2 - 3
    out, link, _, done_o, status, offered = ref.ruled_step((seq, hep, cum, paths, fin), done, val, ids0, lmax, lsum, (lmax, lsum, ts, rank),
                                                           (1, None, 1.0), 40, 1, 4, 0)
    assert link[0].tolist() == [COPY | 0, 1] and out[4][0].tolist() == [1, 0] and out[2][0].tolist() == [-1.0, -1.0]
    assert link[1].tolist() == [COPY | 0, COPY | 1] and done_o.tolist() == [0, 1] and not offered.any() and not status.any()
    # stop rule BEST: output beam 0 is finished
    assert ref.ruled_step((seq, hep, cum, paths, fin), done, val, ids0, lmax, lsum, (lmax, lsum, ts, rank), (1, None, 1.0), 40, 1, 4, 1)[3].tolist() == [1, 1]


# ---------------------------------------------------------------- declared, exported, bound
def test_names_in_header_exports_and_ctypes_table():
    lib = _lib.load()
    txt = open(os.path.join(REPO, "include", "irs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("irs_set_beam_rule", 4), ("irs_beam_step_ruled", 32)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    for phrase in ("need not be descending", "no longer holds", "0 * -inf is never formed", "names both calls", "never silently ignored"):
        assert phrase in txt, phrase
    from influentialrs_amd.engine import Engine
    for fn in (Engine.beam_search, Engine.beam_search_until):
        sig = inspect.signature(fn).parameters
        assert sig["arrive_rank"].default is None and sig["arrive_lp"].default is None and sig["target_weight"].default == 0.0
    assert hasattr(Engine, "set_beam_rule") and hasattr(Engine, "beam_step_ruled")


def test_setter_checks():
    lib, h = _ctx()
    try:
        s = lib.irs_set_beam_rule
        assert s(None, 1, NAN, 0.0) == INVALID
        assert s(h, -1, NAN, 0.0) == INVALID and b"rank_max must be >= 0" in lib.irs_last_error(h)
        for w in (-0.5, NAN, INF, -INF):
            assert s(h, 1, NAN, w) == INVALID and b"target_weight must be finite and >= 0" in lib.irs_last_error(h), w
        for args in ((3, NAN, 0.0), (0, -2.0, 0.0), (0, -INF, 0.0), (0, NAN, 0.5), (0, 1.0, 0.5), (2, 0.0, 4.0)):
            assert s(h, *args) == 0, args
            assert lib.irs_beam_search(h, P_, P_, P_, 2, 2, 3, 10, 0, 0, P_, P_, None, P_, None) == STATE
            assert b"irs_set_beam_rule" in lib.irs_last_error(h)
        for args in ((0, NAN, 0.0), (0, 1.0, 0.0)):  # all three off clears the rule
            assert s(h, 2, NAN, 0.0) == 0 and s(h, *args) == 0
            assert lib.irs_beam_search(h, P_, P_, P_, 2, 2, 3, 10, 0, 0, P_, P_, None, P_, None) == STATE
            assert lib.irs_last_error(h) == b"weights not finalized (irs_finalize_weights)"
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        assert lib.irs_set_beam_rule(h, 3, NAN, 0.0) == UNSUPPORTED
        assert lib.irs_last_error(h) == b"irs_set_beam_rule needs the whole catalog on one device"
        assert lib.irs_set_beam_rule(h, 0, NAN, 0.0) == 0  # clearing what is not set is no error anywhere
    finally:
        lib.irs_destroy(h)


def _step_ruled(lib, h, **kw):
    a = dict(fin_in=None, fin_out=None, done=None, link=P_, W=33, rule=0, mx=P_, rank_max=2, lp_min=NAN, weight=0.0, lse=P_)
    a.update(kw)
    return lib.irs_beam_step_ruled(h, P_, P_, P_, P_, a["fin_in"], P_, P_, a["lse"], a["lse"], 2, a["W"], 10, 0, 3, a["rule"], P_, P_, P_, P_,
                                   a["fin_out"], a["done"], P_, a["link"], P_, a["mx"], P_, P_, P_, a["rank_max"], a["lp_min"], a["weight"])


def test_stand_alone_step_argument_checks():
    lib, h = _ctx()
    try:
        assert _step_ruled(lib, h, link=None) == INVALID and _step_ruled(lib, h, mx=None) == INVALID
        assert _step_ruled(lib, h, fin_in=P_) == INVALID and b"go together" in lib.irs_last_error(h)
        assert _step_ruled(lib, h, lse=None) == INVALID and b"W > 1 needs the row log-sum-exp" in lib.irs_last_error(h)
        assert _step_ruled(lib, h, fin_in=P_, fin_out=P_, done=P_, rule=2) == INVALID and b"stop_rule" in lib.irs_last_error(h)
        assert _step_ruled(lib, h, rank_max=-1) == INVALID and b"rank_max" in lib.irs_last_error(h)
        for w in (-1.0, NAN, INF):
            assert _step_ruled(lib, h, weight=w) == INVALID and b"target_weight" in lib.irs_last_error(h)
        assert _step_ruled(lib, h, rank_max=0) == INVALID and lib.irs_last_error(h) == b"irs_beam_step_ruled: all clauses are off"
        assert _step_ruled(lib, h, rank_max=0, lp_min=2.0) == INVALID and b"all clauses are off" in lib.irs_last_error(h)
        # admitted: every form ends at the launcher's own width check (W = 33), as irs_beam_step_linked does
        for kw in ({}, dict(rank_max=0, lp_min=-1.0), dict(rank_max=0, weight=0.5), dict(fin_in=P_, fin_out=P_, done=P_, rule=1)):
            assert _step_ruled(lib, h, **kw) == UNSUPPORTED and lib.irs_last_error(h) == b"beam width 33 outside [1, 32]", kw
        # it refuses what irs_beam_step_linked refuses, and looks at neither a set rule nor a bound beam trace
        assert lib.irs_set_beam_rule(h, 2, NAN, 0.0) == 0
        assert lib.irs_bind_beam_trace(h, P_, P_, P_, 4, 2, 8, P_, lib.irs_beam_trace_scratch_bytes(h, 4, 2)) == 0
        assert _step_ruled(lib, h) == UNSUPPORTED and lib.irs_last_error(h) == b"beam width 33 outside [1, 32]"
        assert lib.irs_bind_path_trace(h, P_, P_, P_, 8, 4, P_, lib.irs_path_trace_scratch_bytes(h, 8)) == 0
        assert _step_ruled(lib, h) == UNSUPPORTED
        assert lib.irs_last_error(h) == b"irs_beam_step_ruled: a path trace is bound (irs_bind_path_trace): greedy and sampled loops only"
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        assert _step_ruled(lib, h) == UNSUPPORTED and lib.irs_last_error(h) == b"irs_beam_step_ruled needs the whole catalog on one device"
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- every entry point while a rule is set
def _calls(lib, h):
    c = dict(options_host._calls(lib, h, False))
    c["irs_path_step"] = lambda: lib.irs_path_step(h, P_, P_, 4, P_, P_, 4, 0, P_, 3, 0, 0, 0, P_, None)
    c["irs_beam_step_linked"] = lambda: lib.irs_beam_step_linked(h, P_, P_, P_, P_, None, P_, P_, P_, P_, 2, 33, 10, 0, 3, 0, P_, P_, P_, P_,
                                                                 None, None, P_, P_, P_)
    return c


def test_a_rule_without_a_trace_and_every_refusing_entry_point_by_name():
    lib, h = _ctx()
    try:
        assert lib.irs_set_beam_rule(h, 3, NAN, 0.5) == 0
        for name, thunk in _calls(lib, h).items():
            rc, msg = thunk(), lib.irs_last_error(h).decode()
            fn = name.split()[0]
            if fn in ("irs_beam_search", "irs_beam_search_until"):
                assert (rc, msg) == (STATE, f"{fn}: a beam rule is set (irs_set_beam_rule) and no beam trace is bound (irs_bind_beam_trace): "
                                            "the rule reads what the trace sweep leaves"), name
            else:
                assert (rc, msg) == (UNSUPPORTED, f"{fn}: a beam rule is set (irs_set_beam_rule): irs_beam_search and "
                                                  "irs_beam_search_until only"), (name, rc, msg)
        # with the trace bound the loops admit (they end at readiness on a context without weights); the others name the trace first
        assert lib.irs_bind_beam_trace(h, P_, P_, P_, 4, 2, 8, P_, lib.irs_beam_trace_scratch_bytes(h, 4, 2)) == 0
        for name, thunk in _calls(lib, h).items():
            rc, msg = thunk(), lib.irs_last_error(h).decode()
            fn = name.split()[0]
            if fn in ("irs_beam_search", "irs_beam_search_until"):
                assert (rc, msg) == (STATE, "weights not finalized (irs_finalize_weights)"), name
            elif fn == "irs_beam_step_linked":
                assert (rc, msg) == (UNSUPPORTED, f"{fn}: a beam rule is set (irs_set_beam_rule): irs_beam_search and irs_beam_search_until only")
            else:
                assert rc == UNSUPPORTED and msg.startswith(f"{fn}: a beam trace is bound (irs_bind_beam_trace)"), (name, msg)
        # the greedy arrival rule is still refused by the beam loops with the message it always had, and comes first
        assert lib.irs_set_arrival_rule(h, 3, NAN) == 0
        assert lib.irs_beam_search(h, P_, P_, P_, 2, 2, 3, 10, 0, 0, P_, P_, None, P_, None) == UNSUPPORTED
        assert lib.irs_last_error(h) == b"irs_beam_search: an arrival rule is set (irs_set_arrival_rule): greedy and sampled loops only"
        assert lib.irs_set_arrival_rule(h, 0, NAN) == 0
        # cleared and unbound: what a context with nothing bound answers
        assert lib.irs_set_beam_rule(h, 0, NAN, 0.0) == 0 and lib.irs_bind_beam_trace(h, None, None, None, 0, 0, 0, None, 0) == 0
        seen = [(w, t()) for w, t in options_host._calls(lib, h, False).items()]
        assert [(w, rc) for w, rc in seen] == [(w, rc) for w, rc, _ in options_host.EXPECTED[()]]
    finally:
        lib.irs_destroy(h)


@pytest.mark.parametrize("bound", options_host.SCENARIOS, ids=lambda b: "+".join(b) or "nothing")
def test_scenarios_that_do_not_set_the_rule_answer_as_today(bound):
    """Setting and clearing a beam rule first leaves every recorded answer of tests/test_search_options_host.py in place."""
    lib, h = _ctx()
    try:
        assert lib.irs_set_beam_rule(h, 2, -1.0, 0.5) == 0 and lib.irs_set_beam_rule(h, 0, NAN, 0.0) == 0
        seen = options_host._observe(lib, h, bound, lambda guide_bound: options_host._calls(lib, h, guide_bound))
    finally:
        lib.irs_destroy(h)
    assert seen == options_host.EXPECTED[bound]


def test_the_sharded_loops_refuse_by_name_in_the_rule_table():
    """irs_set_beam_rule refuses a sharded context itself, so the sharded loops' refusal can never be needed; it exists so that
    the rule could not be ignored if that ever changed."""
    src = open(os.path.join(REPO, "influentialrs_amd", "csrc", "capi.hip")).read()
    assert "a beam rule (irs_set_beam_rule) needs the whole catalog on one device" in src
    for at in ("AT_GREEDY_LOOP ", "AT_PATH_STEP   ", "AT_BEAM_STEP   ", "AT_BEAM_LOOP   ", "AT_SHARDED_LOOP", "AT_BEAM_STEP_LINKED"):
        assert "OPT_BRULE" in re.search(r"/\* " + at + r" \*/ \{([^}]*)\}", src).group(1), at
    assert "OPT_BRULE" not in re.search(r"/\* AT_BEAM_STEP_RULED \*/ \{([^}]*)\}", src).group(1)
    assert re.search(r"enum \{ OPT_SURV, OPT_EXCL, OPT_TRACE, OPT_GUIDE, OPT_LOOK, OPT_ARRIVE, OPT_BTRACE, OPT_OFFER, OPT_BRULE, OPT_N \}", src)
    for bound in options_host.SHARDED_SCENARIOS:
        assert options_host.observe_sharded(bound) == options_host.EXPECTED_SHARDED[bound]


# ---------------------------------------------------------------- Python layers
def test_front_end_keywords_and_their_value_checks():
    sig = inspect.signature(IRSNN.get_seq_in_batch, follow_wrapped=False).parameters
    for name, default in (("beam_arrive_rank", None), ("beam_arrive_lp", None), ("beam_target_weight", 0.0)):
        assert sig[name].default == default and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
        assert getattr(SearchOptions(), name) == default
    assert list(inspect.signature(IRSNN.get_seq_in_batch).parameters)[-1] == "beam_stop"
    assert beam_rule_kwargs(SearchOptions(), 4, 1) == {} and beam_rule_kwargs(SearchOptions(), 1, 2) == {}
    assert beam_rule_kwargs(SearchOptions(beam_arrive_rank=3, beam_target_weight=0.5), 4, 1) == dict(arrive_rank=3, arrive_lp=None,
                                                                                                    target_weight=0.5)
    assert beam_rule_kwargs(SearchOptions(beam_arrive_lp=-2), 4, 1) == dict(arrive_rank=None, arrive_lp=-2.0, target_weight=0.0)
    for bad, match in ((dict(beam_arrive_rank=0), "beam_arrive_rank=0"), (dict(beam_arrive_rank=True), "beam_arrive_rank"),
                       (dict(beam_arrive_lp=0.5), "beam_arrive_lp=0.5"), (dict(beam_arrive_lp=NAN), "beam_arrive_lp"),
                       (dict(beam_target_weight=-1.0), "beam_target_weight"), (dict(beam_target_weight=INF), "beam_target_weight"),
                       (dict(beam_target_weight=NAN), "beam_target_weight")):
        with pytest.raises(ValueError, match=match):
            beam_rule_kwargs(SearchOptions(**bad), 4, 1)
    with pytest.raises(ValueError, match="need beam_width > 1"):
        beam_rule_kwargs(SearchOptions(beam_arrive_rank=3), 1, 1)
    with pytest.raises(ValueError, match="item-sharded"):
        beam_rule_kwargs(SearchOptions(beam_target_weight=1.0), 4, 2)
    # the greedy keywords answer a beam call as they always did
    with pytest.raises(ValueError, match="arrive_rank / arrive_lp is not built for beam search"):
        search_option_kwargs(SearchOptions(arrive_rank=3), 4, False, 1)
    cfg = synth.make_config("tiny")
    irn = IRSNN(cfg, InfluentialNet(cfg), "cpu")
    B, L = 2, cfg.max_len
    seqs, users, targets = torch.ones((B, L), dtype=torch.int64), torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.int64)
    with pytest.raises(ValueError, match="need beam_width > 1"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, beam_target_weight=0.5)
    assert irn._beam_target_weight == 0.0 and irn._beam_arrive_rank is None, "the switches last for the call"


def test_host_summary_by_hand():
    paths = np.array([[[5, 9, 0, 0], [4, 6, 8, 9], [9, 0, 0, 0], [0, 0, 0, 0]]], dtype=np.float32)
    scores = np.array([[-1.0, -2.0, -3.0, -np.inf]])
    rk = np.array([[[7, 3, 0, 0], [7, 8, 9, 4], [0, 0, 0, 0], [0, 0, 0, 0]]], dtype=np.int32)
    lp = np.array([[[-5, -2, 0, 0], [-5, -6, -7, -1], [0, 0, 0, 0], [0, 0, 0, 0]]], dtype=np.float32)
    n = np.array([[2, 4, 1, 0]])
    tr = dict(paths=paths, scores=scores, rank_target=rk, lp_target=lp, n_steps=n)
    got = beam_rule_summary(tr, np.array([9]), 3, None)
    assert got["arrival_step"].tolist() == [[1, 3, 0, -1]] and got["offered"].tolist() == [[True, False, False, False]]
    got = beam_rule_summary(tr, np.array([9]), None, -1.5)
    assert got["offered"].tolist() == [[False, True, False, False]] and got["offered"].dtype == bool
    assert beam_rule_summary(tr, np.array([8]), 50, -50.0)["arrival_step"].tolist() == [[-1, -1, -1, -1]]
    want, at = ref.replay_offered(paths, lp, rk, np.array([9]), 3, None)
    assert want.tolist() == [[True, False, False, False]] and at.tolist() == [[1, 3, 0, -1]]
