"""not-gpu: the admissible rank (include/irs_hip.h, "admissible rank") -- tests/admissible_ref.py on hand examples, the new names
in the header, the exports and the ctypes table, the ABI's refusals on a context without a device, and the Python layers'
ValueErrors."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import admissible_ref as ref
import path_trace_ref
from influentialrs_amd import _lib
from influentialrs_amd.engine import Engine, arrive_among_kind, check_rank_options
from influentialrs_amd.model.influentialRS import (IRSNN, SearchOptions, path_trace_summary, search_option_kwargs, slate_steps)
from influentialrs_amd.model.rec2inf import Rec2Inf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
INVALID, STATE, UNSUPPORTED = -1, -2, -4
P = ctypes.c_void_p(4096)  # a fake non-null, 16-byte aligned address: every call here is refused before anything is dereferenced


# ---------------------------------------------------------------- the statement on hand examples
#            item: 1    2    3    4    5    6    7    8
LOGITS = np.array([9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0], dtype=np.float32)


def test_nothing_hidden_is_the_trace_rank():
    for t in range(0, 10):
        for window in ([], [0, 0, 2], [2, 2, 5], [t]):
            assert ref.target_rank_admissible(LOGITS, window, t, set()) == path_trace_ref.target_rank(LOGITS, window, t)
    assert ref.target_rank_admissible(LOGITS, [], 0, {1, 2}) == 0 and ref.target_rank_admissible(LOGITS, [], 9, {1}) == 0


def test_a_duplicate_across_list_window_and_path_counts_once():
    # target 6 (rank 6 in the catalog).  Item 2 is in the list twice, in the window twice and on the path: one item gone.
    excl = np.array([1, 1, -1, 7, 8], dtype=np.int64)  # 0-based: item 2 twice, a hole, item 8, and an id outside the catalog
    path = np.array([2, 0, 3, 2, 4], dtype=np.float32)  # entries [0, 4): items 2, 3, 2 (a zero between); entry 4 is not walked yet
    h = ref.hidden(excl, 8, path, 4)
    assert h == {2, 8, 3}
    assert ref.target_rank_admissible(LOGITS, [0, 2, 2, 1], 6, h) == 6 - 3  # items 1, 2, 3 gone; 8 ranks behind the target
    assert ref.target_rank_admissible(LOGITS, [0, 2, 2, 1], 6, ref.hidden(excl, 8, path, 5)) == 6 - 4  # entry 4 walked: item 4
    assert ref.target_rank_admissible(LOGITS, [0, 2, 2, 1], 6, ref.hidden(excl, 8)) == 6 - 2  # no path given: the list alone


def test_the_target_inside_h_still_has_a_rank():
    for h, window in (({6}, []), (set(), [6]), ({6, 1}, [6, 1])):
        assert ref.target_rank_admissible(LOGITS, window, 6, h) == 6 - (1 in h)
    assert ref.slate_position(LOGITS, [], 6, {6}) is None and ref.slate_position(LOGITS, [6], 6, set()) is None
    assert ref.slate_position(LOGITS, [1], 6, {2}) == 3 == ref.target_rank_admissible(LOGITS, [1], 6, {2}) - 1


def test_ties_go_by_id_and_the_two_zeros_are_one():
    tie = np.array([1.0, 5.0, 5.0, 5.0, 0.5], dtype=np.float32)  # items 2, 3, 4 tie: the lower id ranks first
    assert [ref.target_rank_admissible(tie, [], t, set()) for t in (2, 3, 4)] == [1, 2, 3]
    assert ref.target_rank_admissible(tie, [], 4, {2}) == 2 and ref.target_rank_admissible(tie, [], 3, {4}) == 2
    zeros = np.array([-0.0, 0.0, -0.0, 0.0], dtype=np.float32)
    assert [ref.target_rank_admissible(zeros, [], t, set()) for t in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert ref.target_rank_admissible(zeros, [2], 4, {1}) == 2


def test_an_offer_set_with_the_target_outside_it():
    offer = np.array([0, 2, 4, 7, -1, 99], dtype=np.int64)  # items 1, 3, 5, 8; a hole and an id outside the catalog
    assert ref.target_rank_admissible(LOGITS, [], 6, set(), offer) == 1 + 3  # 1, 3, 5 stand before item 6, which is not in the set
    assert ref.target_rank_admissible(LOGITS, [3], 6, {2, 5}, offer) == 1 + 1  # 3 and 5 gone; 2 was never offered
    assert ref.target_rank_admissible(LOGITS, [], 5, set(), offer) == 3  # the target inside the set
    assert ref.slate_position(LOGITS, [], 6, set(), offer) is None and ref.slate_position(LOGITS, [], 5, set(), offer) == 2
    full = np.arange(8)
    for t in range(1, 9):
        assert ref.target_rank_admissible(LOGITS, [2], t, {4}, full) == ref.target_rank_admissible(LOGITS, [2], t, {4})


def test_rows_reads_the_list_through_the_map():
    logits = np.stack([LOGITS, LOGITS])
    seq = np.array([[0, 1, 6], [0, 1, 6]], dtype=np.int64)
    hep = np.array([1, 0], dtype=np.int32)  # row 1: item 1 lies behind hep
    excl = np.array([[1, -1], [2, 3]], dtype=np.int64)
    assert ref.rows(logits, seq, hep, excl).tolist() == [6 - 2, 6 - 2]
    assert ref.rows(logits, seq, hep, excl, user_of=[1, 0]).tolist() == [6 - 3, 6 - 1]


def test_replay_fires_on_the_admissible_rank():
    seq = np.array([[0, 10, 11, 5], [0, 10, 11, 6]], dtype=np.int64)
    hep = np.array([2, 2], dtype=np.int32)
    paths = np.array([[1, 2, 3], [1, 2, 3]], dtype=np.float32)
    lp = np.full((2, 3), -3.0, dtype=np.float32)
    rank_t = np.array([[9, 9, 9], [9, 9, 9]], dtype=np.int32)
    rank_a = np.array([[4, 2, 1], [4, 3, 3]], dtype=np.int32)
    out = ref.replay(seq, hep, paths, (lp, lp, rank_t), rank_a, 2, NAN, 20)
    assert out[0].tolist() == [[1, 5, 0], [1, 2, 3]] and out[2].tolist() == [2, 3] and out[4].tolist() == [True, False]
    assert out[1][3].tolist() == [[4, 2, 0], [4, 3, 3]] and out[1][2].tolist() == [[9, 9, 0], [9, 9, 9]]
    # the window's rank would never have fired; a target outside the offer set is never offered
    assert not ref.replay(seq, hep, paths, (lp, lp, rank_t), rank_t, 2, NAN, 20)[4].any()
    assert not ref.replay(seq, hep, paths, (lp, lp, rank_t), rank_a, 2, NAN, 20, offer=[0, 1, 2, 5])[4][0]
    assert ref.replay(seq, hep, paths, (lp, lp, rank_t), rank_a, 2, NAN, 20, offer=[0, 1, 2, 4])[4][0]
    listed = np.array([[4], [-1]], dtype=np.int64)  # the target in the user's list: not admissible, whatever its rank
    assert not ref.replay(seq, hep, paths, (lp, lp, rank_t), rank_a, 2, NAN, 20, excl=listed)[4].any()


def test_ml1m_shaped_lists():
    ex = ref.ml1m_lists(96, 500, 3)
    n = (ex >= 0).sum(axis=1)
    assert ex.shape[0] == 96 and n.max() == round(2276 * 500 / 3415) + 1 and 8 <= np.median(n) <= 24
    assert all(len(set(r[r >= 0].tolist())) == (r >= 0).sum() - 1 for r in ex if (r >= 0).sum() >= 3)


# ---------------------------------------------------------------- declared, exported, bound
NEW = {"irs_admissible_scratch_bytes": 2, "irs_score_target_rank_admissible": 17, "irs_bind_trace_admissible": 6,
       "irs_set_arrival_rule_ex": 4}


def test_names_in_header_exports_and_ctypes_table():
    lib = _lib.load()
    txt = open(os.path.join(REPO, "include", "irs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert re.search(r"#define\s+IRS_RANK_WINDOW\s+0\b", code) and re.search(r"#define\s+IRS_RANK_ADMISSIBLE\s+1\b", code)
    assert (_lib.IRS_RANK_WINDOW, _lib.IRS_RANK_ADMISSIBLE) == (0, 1)
    assert _lib.SIGNATURES["irs_admissible_scratch_bytes"][0] is ctypes.c_size_t
    for phrase in ("admissible rank", "U \\ H", "rank_target in every cell", "rank_adm - 1"):
        assert phrase in txt, phrase
    assert "admissible.hip" in open(os.path.join(REPO, "influentialrs_amd", "build.py")).read()


# ---------------------------------------------------------------- the ABI without a device
def _ctx(world=1):
    lib = _lib.load()
    h = ctypes.c_void_p()
    dims = _lib.IrsDims(n_item=1000, n_user=10, d=30, max_len=60, n_heads=6, ffn_dim=256, n_layers=2, u_dim=10, mask_mode=0,
                        max_rows=64, max_k=100, max_seqs=0)
    shard = _lib.IrsShard(0, world, 0, 1000 // world) if world > 1 else None
    assert lib.irs_create(ctypes.byref(h), ctypes.byref(dims), ctypes.byref(shard) if shard else None) == 0
    return lib, h


def _trace(lib, h, users=8, ld=4):
    return lib.irs_bind_path_trace(h, P, P, P, users, ld, P, lib.irs_path_trace_scratch_bytes(h, users))


def _paths(lib, h):
    return lib.irs_generate_paths(h, P, P, P, 4, 3, 10, 0, 0, 3, 0, 0, P, P, None)


def _until(lib, h):
    return lib.irs_generate_paths_until(h, P, P, P, 4, 3, 10, 0, 0, 3, 0, 1, P, P, None, None)


def test_scratch_bytes_and_the_binding():
    lib, h = _ctx()
    try:
        f = lib.irs_admissible_scratch_bytes
        assert f(None, 8) == 0 and f(h, 0) == 0 and f(h, 65) == 0
        assert f(h, 1) == 256 and f(h, 64) == 256
        b = lib.irs_bind_trace_admissible
        assert b(None, P, 8, 4, P, 256) == INVALID
        assert b(h, P, 8, 4, P, 256) == STATE and b"irs_bind_path_trace" in lib.irs_last_error(h)
        assert b(h, None, 0, 0, None, 0) == 0  # nothing to unbind is fine
        assert _trace(lib, h) == 0
        assert b(h, P, 7, 4, P, 256) == INVALID and b(h, P, 8, 5, P, 256) == INVALID
        assert b"[8, 4]" in lib.irs_last_error(h)
        assert b(h, P, 8, 4, P, 255) == INVALID and b(h, P, 8, 4, None, 256) == INVALID
        assert b(h, P, 8, 4, ctypes.c_void_p(4100), 256) == INVALID
        assert b(h, P, 8, 4, P, 256) == 0
        # the loops admit it: they end at the readiness check, as with the trace alone
        assert _paths(lib, h) == STATE and b"not finalized" in lib.irs_last_error(h)
        # every entry point that refuses the trace still answers for the trace
        assert lib.irs_beam_step(h, P, P, P, P, P, P, P, P, 2, 33, 10, 0, 3, P, P, P, P, P, None) == UNSUPPORTED
        assert b"irs_bind_path_trace" in lib.irs_last_error(h)
    finally:
        lib.irs_destroy(h)


def test_an_admissible_rule_needs_the_binding_and_rebinding_the_trace_drops_it():
    lib, h = _ctx()
    try:
        ex = lib.irs_set_arrival_rule_ex
        assert ex(None, 3, NAN, 1) == INVALID
        assert ex(h, 3, NAN, 2) == INVALID and b"rank_kind" in lib.irs_last_error(h)
        assert ex(h, -1, NAN, 1) == INVALID
        assert ex(h, 3, NAN, 1) == 0

        def named():
            return (_paths(lib, h) == STATE and b"irs_bind_trace_admissible" in lib.irs_last_error(h)
                    and _until(lib, h) == STATE and b"irs_bind_trace_admissible" in lib.irs_last_error(h))

        def admitted():
            return _paths(lib, h) == STATE and b"not finalized" in lib.irs_last_error(h)

        # without a trace the rule answers as it always did
        assert _paths(lib, h) == STATE and b"irs_bind_path_trace" in lib.irs_last_error(h)
        assert b"irs_bind_trace_admissible" not in lib.irs_last_error(h)
        assert _trace(lib, h) == 0
        assert named()
        assert lib.irs_bind_trace_admissible(h, P, 8, 4, P, 256) == 0
        assert admitted()
        assert _trace(lib, h) == 0  # rebinding the trace drops the admissible binding
        assert named()
        assert lib.irs_bind_trace_admissible(h, P, 8, 4, P, 256) == 0 and admitted()
        assert lib.irs_bind_path_trace(h, None, None, None, 0, 0, None, 0) == 0  # so does unbinding it
        assert _trace(lib, h) == 0 and named()
        # kind WINDOW is irs_set_arrival_rule: no binding needed, through either entry
        assert ex(h, 3, NAN, 0) == 0 and admitted()
        assert ex(h, 3, NAN, 1) == 0 and named()
        assert lib.irs_set_arrival_rule(h, 3, NAN) == 0 and admitted()
        assert ex(h, 0, NAN, 1) == 0 and admitted()  # both clauses off clears the rule, whatever the kind
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        assert lib.irs_set_arrival_rule_ex(h, 3, NAN, 1) == UNSUPPORTED
        assert lib.irs_set_arrival_rule_ex(h, 0, NAN, 1) == 0
    finally:
        lib.irs_destroy(h)


def test_the_standalone_call_checks_its_arguments_first():
    lib, h = _ctx()
    try:
        f = lib.irs_score_target_rank_admissible
        tb, ab = lib.irs_path_trace_scratch_bytes(h, 4), lib.irs_admissible_scratch_bytes(h, 4)

        def call(x=P, M=4, paths=None, ld=0, step=0, ts=P, tbytes=tb, sc=P, bytes_=ab, out=P):
            return f(h, x, P, P, M, paths, ld, step, ts, tbytes, sc, bytes_, P, P, P, P, out)

        assert f(None, P, P, P, 4, None, 0, 0, P, tb, P, ab, P, P, P, P, P) == INVALID
        for bad in (dict(x=None), dict(M=0), dict(M=65), dict(out=None), dict(ts=None), dict(tbytes=tb - 1), dict(sc=None),
                    dict(bytes_=ab - 1), dict(sc=ctypes.c_void_p(4100)), dict(step=-1), dict(paths=P, ld=0, step=0),
                    dict(paths=P, ld=8, step=9), dict(paths=P, ld=100, step=65)):
            assert call(**bad) == INVALID, bad
        assert call() == STATE and call(paths=P, ld=8, step=8) == STATE  # valid arguments end at the readiness check
        # no search option refuses it
        assert lib.irs_set_arrival_rule(h, 3, NAN) == 0 and lib.irs_bind_survivor_scratch(h, P, 1 << 20) == 0
        assert call() == STATE and b"not finalized" in lib.irs_last_error(h)
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        tb, ab = lib.irs_path_trace_scratch_bytes(h, 4), lib.irs_admissible_scratch_bytes(h, 4)
        assert lib.irs_score_target_rank_admissible(h, P, P, P, 4, None, 0, 0, P, tb, P, ab, P, P, P, P, P) == UNSUPPORTED
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- Python layers
def test_value_errors_and_keywords():
    assert arrive_among_kind("window") == 0 and arrive_among_kind("admissible") == 1
    for bad in ("slate", None, 1):
        with pytest.raises(ValueError, match="arrive_among"):
            arrive_among_kind(bad)
    check_rank_options(True, True, "admissible")
    check_rank_options(False, False, "window")
    with pytest.raises(ValueError, match="rank_admissible=True"):
        check_rank_options(True, False, "admissible")
    with pytest.raises(ValueError, match="trace=True"):
        check_rank_options(False, True, "window")
    for fn in (Engine.generate_paths, Engine.generate_paths_until, Engine._search_options):
        par = inspect.signature(fn).parameters
        assert par["rank_admissible"].default is False and par["arrive_among"].default == "window", fn
    for fn in (Engine.beam_search, Engine.beam_search_until, Engine.generate_paths_sharded):
        assert "rank_admissible" not in inspect.signature(fn).parameters, fn
    for name in ("admissible_scratch_bytes", "bind_trace_admissible", "unbind_trace_admissible", "score_target_rank_admissible"):
        assert hasattr(Engine, name), name
    assert inspect.signature(Engine.set_arrival_rule).parameters["among"].default == "window"
    for fn in (IRSNN.get_seq_in_batch, Rec2Inf.get_seq_in_batch.__wrapped__):  # (Rec2Inf's outermost wrapper takes offer)
        sig = inspect.signature(fn, follow_wrapped=False).parameters
        for name, default in (("rank_admissible", False), ("arrive_among", "window")):
            assert sig[name].default == default and sig[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn, name)
        assert "rank_admissible" not in inspect.signature(fn).parameters  # the declared parameter lists are what they were


def test_front_end_options():
    kw = search_option_kwargs(SearchOptions(trace=True, rank_admissible=True), 1, False, 1)
    assert kw["rank_admissible"] is True and "arrive_among" not in kw
    kw = search_option_kwargs(SearchOptions(arrive_rank=3, rank_admissible=True, arrive_among="admissible"), 1, False, 1)
    assert kw["trace"] is True and kw["rank_admissible"] is True and kw["arrive_among"] == "admissible" and kw["arrive_rank"] == 3
    assert "rank_admissible" not in search_option_kwargs(SearchOptions(trace=True), 1, False, 1)
    with pytest.raises(ValueError, match="rank_admissible=True"):
        search_option_kwargs(SearchOptions(arrive_rank=3, arrive_among="admissible"), 1, False, 1)
    with pytest.raises(ValueError, match="arrive_among"):
        search_option_kwargs(SearchOptions(trace=True, arrive_among="slate"), 1, False, 1)
    with pytest.raises(ValueError, match="trace=True"):
        search_option_kwargs(SearchOptions(rank_admissible=True), 1, False, 1)
    with pytest.raises(ValueError, match="beam search"):
        search_option_kwargs(SearchOptions(trace=True, rank_admissible=True), 4, False, 1)
    with pytest.raises(ValueError, match="item-sharded"):
        search_option_kwargs(SearchOptions(trace=True, rank_admissible=True), 1, False, 2)


def test_summary_cuts_rank_adm_and_gives_the_slate_step():
    z = np.zeros((3, 4), dtype=np.float32)
    rank_t = np.full((3, 4), 9, dtype=np.int32)
    rank_a = np.array([[5, 3, 2, 1], [7, 6, 6, 6], [2, 2, 2, 2]], dtype=np.int32)
    paths = np.array([[4, 5, 9, 6], [4, 5, 6, 7], [4, 5, 6, 7]], dtype=np.float32)
    tr = path_trace_summary(z, z, rank_t, paths, np.array([9, 1, 1]), rank_adm=rank_a)
    assert tr["n_steps"].tolist() == [3, 4, 4]
    assert tr["rank_adm"].tolist() == [[5, 3, 2, 0], [7, 6, 6, 6], [2, 2, 2, 2]]
    assert tr["slate_step"](3).tolist() == [1, -1, 0] and tr["slate_step"](1).tolist() == [-1, -1, -1]
    assert tr["slate_step"](6).tolist() == [0, 1, 0]
    assert slate_steps(rank_a, np.array([1, 1, 0]), 6).tolist() == [0, -1, -1]
    assert "rank_adm" not in path_trace_summary(z, z, rank_t, paths, np.array([9, 1, 1]))
