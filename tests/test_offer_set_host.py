"""not-gpu: the offer set's CPU statement, its scratch formula, and every argument check of its three entry points through the ABI on
contexts created without a device.

A successful irs_bind_offer_set launches its prepare kernel, so -- like exclusions in tests/test_search_options_host.py -- the
option's row at the search entry points while a set IS bound is left to tests/test_gpu_offer_set.py.  What can be stated here: a
context on which every bind was refused, and one that was unbound, answer every call of that module's scenarios exactly as
recorded there."""
import ctypes
import inspect

import numpy as np
import pytest

import offer_set_ref as ref
import test_search_options_host as SO
from influentialrs_amd import _lib
from influentialrs_amd.engine import Engine
from influentialrs_amd.model.evaluator import Evaluator
from influentialrs_amd.model.influentialRS import IRSNN, SearchOptions, offer_ids0, search_option_kwargs
from influentialrs_amd.model.rec2inf import Rec2Inf

INVALID, STATE, UNSUPPORTED = -1, -2, -4
P = ctypes.c_void_p(4096)
N_ITEM, MAX_ROWS = 1000, 64  # test_search_options_host._ctx


# ---------------------------------------------------------------- the statement
def test_statement_equals_a_brute_force_selection():
    g = np.random.default_rng(5)
    n = 97
    scores = g.standard_normal(n).astype(np.float32)
    scores[[3, 40, 41, 90]] = scores[7]      # ties inside and outside the set: the lower id first
    scores[11], scores[12] = 0.0, -0.0       # the order folds the two zeros
    scores[20] = -np.inf
    for C in (1, 2, 15, 64, 96, 97):
        s = np.sort(g.permutation(n)[:C])
        if C >= 15:
            s = np.unique(np.concatenate([s[:C - 6], [3, 7, 11, 12, 20, 41]]))
        for k in (1, 5, len(s) - 1, len(s), len(s) + 1, 128):
            if k < 1:
                continue
            val, ids, fewer = ref.topk(scores, s, k)
            b_val, b_ids = ref.brute_force(scores, s, k)
            assert np.array_equal(ids, b_ids), (C, k)
            assert np.array_equal(val.view(np.uint32), b_val.view(np.uint32)), (C, k)
            assert fewer == (k > len(s)) and (ids[:min(k, len(s))] >= 0).all() and (ids[len(s):] == -1).all()
            assert set(ids[ids >= 0].tolist()) <= set(s.tolist())
    # a hole (-1) of a sanitised array is no member
    val, ids, fewer = ref.topk(scores, np.array([2, -1, 9, -1]), 3)
    assert sorted(ids[:2].tolist()) == [2, 9] and ids[2] == -1 and fewer


def test_sanitise_counts_holes_by_the_predecessor_in_the_callers_array():
    ids, holes = ref.sanitise([0, 5, 5, 4, 9, 1000, -3, 12, 11, 999], N_ITEM)
    #                          ok ok rep desc ok  big  neg ok  desc ok
    assert ids.tolist() == [0, 5, -1, -1, 9, -1, -1, 12, -1, 999] and holes == 5
    assert ref.sanitise(np.arange(17), 17) == (pytest.approx(np.arange(17)), 0)
    assert ref.complement([1, 3], 5).tolist() == [0, 2, 4]


# ---------------------------------------------------------------- the scratch size
def test_scratch_bytes_values_and_zeros():
    lib, h = SO._ctx()
    try:
        f = lib.irs_offer_set_scratch_bytes
        assert f(None, 10, 4) == 0
        for n_ids, rows in ((0, 4), (-1, 4), (N_ITEM + 1, 4), (10, 0), (10, -1), (10, MAX_ROWS + 1)):
            assert f(h, n_ids, rows) == 0 == ref.scratch_bytes(n_ids, rows, N_ITEM, MAX_ROWS), (n_ids, rows)
        assert f(h, 1, 1) == 256 + 512 + 4 * 64 and f(h, 64, 1) == 256 + 512 + 4 * 64
        assert f(h, 65, 3) == 256 + 1024 + 4 * 3 * 128
        assert f(h, N_ITEM, MAX_ROWS) == 256 + 8192 + 4 * 64 * 1024
        for n_ids, rows in ((1, 1), (63, 7), (64, 64), (65, 2), (257, 33), (999, 64), (1000, 1)):
            assert f(h, n_ids, rows) == ref.scratch_bytes(n_ids, rows, N_ITEM, MAX_ROWS) and f(h, n_ids, rows) % 16 == 0
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- refusals, before any launch
def test_bind_refusals_without_a_device():
    lib, h = SO._ctx()
    try:
        f = lib.irs_bind_offer_set
        big = 1 << 26
        assert f(None, P, 10, P, big) == INVALID
        assert f(h, None, 0, None, 0) == 0, "unbinding what was never bound is fine"
        assert f(h, None, 10, P, big) == INVALID and b"go together" in lib.irs_last_error(h)
        for n_ids in (0, -1, N_ITEM + 1):
            assert f(h, P, n_ids, P, big) == INVALID and b"n_ids must be in [1, n_item=1000]" in lib.irs_last_error(h), n_ids
        need1 = lib.irs_offer_set_scratch_bytes(h, 10, 1)
        assert f(h, P, 10, P, need1 - 1) == INVALID and b"too small" in lib.irs_last_error(h)
        assert f(h, P, 10, None, big) == INVALID
        assert f(h, P, 10, P, 0) == INVALID
        assert f(h, P, 10, ctypes.c_void_p(4096 + 8), big) == INVALID and b"aligned" in lib.irs_last_error(h)
        # nothing of the above bound anything: the kernel alone says so once the context could run, and stops at the unbound
        # weights before that; a loop gets as far as the unbound weights too
        assert lib.irs_score_topk_offer(h, P, 1, 10, P, P, P) == STATE and b"not finalized" in lib.irs_last_error(h)
        assert lib.irs_generate_paths(h, P, P, P, 4, 3, 10, 0, 0, 0, 0, 0, P, P, None) == STATE
    finally:
        lib.irs_destroy(h)
    lib, h = SO._ctx(world=2)
    try:
        assert lib.irs_bind_offer_set(h, P, 10, P, 1 << 26) == UNSUPPORTED and b"whole catalog" in lib.irs_last_error(h)
        assert lib.irs_bind_offer_set(h, None, 0, None, 0) == 0
    finally:
        lib.irs_destroy(h)


def test_score_topk_offer_refusals_without_a_device():
    lib, h = SO._ctx()
    try:
        f = lib.irs_score_topk_offer
        err = lambda: lib.irs_last_error(h)  # noqa: E731
        assert f(None, P, 1, 10, P, P, P) == INVALID
        # the argument checks come before the readiness check: a context without weights reaches every one of them
        assert f(h, None, 1, 10, P, P, P) == INVALID and b"irs_score_topk_offer: bad arguments" in err()
        for M in (0, -1):
            assert f(h, P, M, 10, P, P, P) == INVALID and b"irs_score_topk_offer: bad arguments" in err(), M
        assert f(h, P, MAX_ROWS + 1, 10, P, P, P) == INVALID and b"M=65 exceeds max_rows=64" in err()
        for k in (0, -1, 101, 1025, 1 << 20):  # (max_k = 100: k bounds the selection's LDS buffer)
            assert f(h, P, 1, k, P, P, P) == INVALID and b"irs_score_topk_offer: k must be in [1, 100]" in err(), k
        for outs in ((None, P, P), (P, None, P), (P, P, None)):
            assert f(h, P, 1, 10, *outs) == INVALID and b"irs_score_topk_offer: null output" in err(), outs
        # every argument valid, at both ends of k and M: the context's state is the next thing asked about
        for M, k in ((1, 1), (MAX_ROWS, 100)):
            assert f(h, P, M, k, P, P, P) == STATE and b"not finalized" in err(), (M, k)
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- nothing bound: every recorded answer stands
@pytest.mark.parametrize("bound", SO.SCENARIOS, ids=lambda b: "+".join(b) or "none")
def test_unbound_context_answers_the_recorded_scenarios(bound, monkeypatch):
    """The scenarios of tests/test_search_options_host.py on a context that saw a refused bind and an unbind of an offer set
    first: the recorded answers, text for text."""
    real = SO._ctx

    def ctx_with_history(world=1):
        lib, h = real(world)
        assert lib.irs_bind_offer_set(h, P, 0, P, 1 << 20) == INVALID
        assert lib.irs_bind_offer_set(h, None, 0, None, 0) == 0
        return lib, h

    monkeypatch.setattr(SO, "_ctx", ctx_with_history)
    assert SO.observe_single(bound) == SO.EXPECTED[bound]


@pytest.mark.parametrize("bound", SO.SHARDED_SCENARIOS, ids=lambda b: "+".join(b) or "none")
def test_unbound_sharded_context_answers_the_recorded_scenarios(bound, monkeypatch):
    real = SO._ctx

    def ctx_with_history(world=1):
        lib, h = real(world)
        assert lib.irs_bind_offer_set(h, P, 10, P, 1 << 20) == UNSUPPORTED
        assert lib.irs_bind_offer_set(h, None, 0, None, 0) == 0
        return lib, h

    monkeypatch.setattr(SO, "_ctx", ctx_with_history)
    assert SO.observe_sharded(bound) == SO.EXPECTED_SHARDED[bound]


# ---------------------------------------------------------------- the Python layers
def test_symbols_and_keywords_of_the_python_layers():
    sig = _lib.SIGNATURES
    assert sig["irs_offer_set_scratch_bytes"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32])
    assert sig["irs_bind_offer_set"][0] is ctypes.c_int32 and len(sig["irs_bind_offer_set"][1]) == 5  # (no stream: the null stream)
    assert sig["irs_score_topk_offer"][0] is ctypes.c_int32 and len(sig["irs_score_topk_offer"][1]) == 7
    for name in ("offer_set_scratch_bytes", "bind_offer_set", "unbind_offer_set", "score_topk_offer"):
        assert hasattr(Engine, name), name
    for fn in (Engine.generate_paths, Engine.generate_paths_until, Engine.beam_search, Engine.beam_search_until, Engine._search_options):
        assert inspect.signature(fn).parameters["offer"].default is None, fn
    assert "offer" not in inspect.signature(Engine.generate_paths_sharded).parameters
    # the front ends take the keyword in a wrapper: off by default, keyword only, the declared parameters as they were
    for fn in (IRSNN.get_seq_in_batch, IRSNN.predict_next, Evaluator.predict_next, Rec2Inf.get_seq_in_batch):
        par = inspect.signature(fn, follow_wrapped=False).parameters
        assert par["offer"].default is None and par["offer"].kind is inspect.Parameter.KEYWORD_ONLY, fn
        assert "offer" not in inspect.signature(fn).parameters, fn
    assert SearchOptions().offer is None
    with pytest.raises(ValueError, match="item-sharded"):
        search_option_kwargs(SearchOptions(offer=[1, 2]), 1, False, 2)
    assert search_option_kwargs(SearchOptions(offer=[1, 2]), 1, False, 1) == dict(exact_candidates=False, trace=False)


def test_offer_ids0_takes_one_based_ids():
    assert offer_ids0(None, 10, "cpu") is None
    assert offer_ids0([3, 1, 10], 10, "cpu").tolist() == [2, 0, 9]
    assert offer_ids0(np.array([[1, 2], [3, 4]]), 10, "cpu").tolist() == [0, 1, 2, 3]
    for bad in ([0, 1], [11], [], [1.5]):
        with pytest.raises(ValueError, match="offer"):
            offer_ids0(bad, 10, "cpu")
