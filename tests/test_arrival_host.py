"""Arrival rule, the parts that need no GPU: the numpy statement (tests/arrival_ref.py) by hand on 3-row examples, the new
symbols and the status bit in header, library and ctypes table, the setter's and the stand-alone kernel's argument checks on a
context created without a device (refused before any launch), and the front end's refusals."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arrival_ref as ref  # noqa: E402

from influentialrs_amd import _lib  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, UNSUPPORTED = -1, -2, -4
NAN, INF = float("nan"), float("inf")
L, N, K = 6, 40, 4  # window length, catalog, list length of the hand examples


def _ctx(world=1, **kw):
    lib = _lib.load()
    h = ctypes.c_void_p()
    base = dict(n_item=1000, n_user=10, d=30, max_len=60, n_heads=6, ffn_dim=256, n_layers=2, u_dim=10, mask_mode=0,
                max_rows=64, max_k=100, max_seqs=0)
    base.update(kw)
    dims = _lib.IrsDims(**base)
    shard = _lib.IrsShard(0, world, 0, base["n_item"] // world) if world > 1 else None
    assert lib.irs_create(ctypes.byref(h), ctypes.byref(dims), ctypes.byref(shard) if shard else None) == 0
    return lib, h


# ---------------------------------------------------------------- the statement, by hand
def _lists():
    """Three rows of a ranked list that nobody may touch unless the rule fires: ids 30, 31, 32, 33 with falling scores."""
    val = np.tile(np.array([4.0, 3.0, 2.0, 1.0], dtype=np.float32), (3, 1))
    ids0 = np.tile(np.array([30, 31, 32, 33], dtype=np.int64), (3, 1))
    return val, ids0, np.array([0, 2, 8], dtype=np.int32)  # status words with bits of other kernels in them


def _rows(targets, windows, heps):
    seq = np.zeros((3, L), dtype=np.int64)
    for m in range(3):
        seq[m, :len(windows[m])] = windows[m]
        seq[m, L - 1] = targets[m]
    return seq, np.array(heps, dtype=np.int32)


def _untouched(got, val, ids0, status, m):
    return (np.array_equal(got[0][m].view(np.uint32), val[m].view(np.uint32)) and np.array_equal(got[1][m], ids0[m])
            and got[2][m] == status[m] and not got[3][m])


def _offered(got, val, ids0, status, m, ts, t):
    return (got[0][m, 0].view(np.uint32) == np.float32(ts).view(np.uint32) and got[1][m, 0] == t - 1
            and got[0][m, 1] == -np.inf and got[1][m, 1] == -1
            and np.array_equal(got[0][m, 2:], val[m, 2:]) and np.array_equal(got[1][m, 2:], ids0[m, 2:])
            and got[2][m] == (status[m] | 16) and got[3][m])


def test_rank_clause_at_r_and_r_plus_one_and_no_target():
    val, ids0, status = _lists()
    seq, hep = _rows([7, 8, 0], [[1, 2], [1, 2], [1, 2]], [1, 1, 1])
    mx, sm = np.full(3, 5.0, np.float32), np.full(3, 2.0, np.float32)
    ts = np.array([1.5, 1.25, -np.inf], dtype=np.float32)
    rank = np.array([5, 6, 0], dtype=np.int32)  # exactly r, r + 1, no target
    got = ref.offer(seq, hep, mx, sm, ts, rank, val, ids0, status, 5, NAN, N)
    assert _offered(got, val, ids0, status, 0, 1.5, 7)
    assert _untouched(got, val, ids0, status, 1) and _untouched(got, val, ids0, status, 2)
    # rk = 0 fires under no clause: not even lp_min = -inf, whose lp >= lp_min holds for every number
    got = ref.offer(seq, hep, mx, sm, ts, rank, val, ids0, status, 1000, -INF, N)
    assert got[3].tolist() == [True, True, False]
    # k = 1: entry 0 only
    got = ref.offer(seq, hep, mx, sm, ts, rank, val[:, :1], ids0[:, :1], status, 5, NAN, N)
    assert got[0].shape == (3, 1) and got[1][:, 0].tolist() == [6, 30, 30] and got[2].tolist() == [16, 2, 8]


def test_probability_clause_at_lp_min_one_ulp_below_and_nan():
    val, ids0, status = _lists()
    seq, hep = _rows([7, 8, 9], [[1, 2], [1, 2], [1, 2]], [1, 1, 1])
    mx, sm = np.full(3, 5.0, np.float32), np.full(3, 1.0, np.float32)  # log(1) = 0: lp = ts - 5 exactly
    lp_min = np.float32(-2.75)
    below = np.nextafter(np.float32(2.25), np.float32(-np.inf))  # lp one ulp of 2.25 below -2.75 ...
    assert np.float32(np.float64(below) - 5.0) < lp_min  # ... still below after the one rounding to float32
    ts = np.array([2.25, below, np.nan], dtype=np.float32)
    rank = np.array([50, 50, 50], dtype=np.int32)
    assert ref.lp_value(ts[0], mx[0], sm[0], 50) == lp_min and ref.lp_value(ts[0], mx[0], sm[0], 0) == 0
    got = ref.offer(seq, hep, mx, sm, ts, rank, val, ids0, status, 0, float(lp_min), N)
    assert _offered(got, val, ids0, status, 0, 2.25, 7)
    assert _untouched(got, val, ids0, status, 1) and _untouched(got, val, ids0, status, 2)  # a NaN lp never fires
    # both clauses: the rank clause fires the NaN row all the same (its entry 0 carries the NaN score)
    got = ref.offer(seq, hep, mx, sm, ts, rank, val, ids0, status, 50, float(lp_min), N)
    assert got[3].all() and np.isnan(got[0][2, 0])
    # the clauses' switches
    assert ref.clauses(0, NAN) == (False, False) and ref.clauses(1, 0.5) == (True, False)
    assert ref.clauses(0, 0.0) == (False, True) and ref.clauses(0, -INF) == (False, True)
    assert not ref.fires(3, -1.0, 0, NAN) and ref.fires(3, -1.0, 0, -1.0) and ref.fires(3, -1.0, 3, 0.5)


def test_admissibility_window_exclusion_list_and_path():
    val, ids0, status = _lists()
    # row 0: the target inside the live window; row 1: the target in a window slot beyond hep (admissible); row 2: plain
    seq, hep = _rows([7, 8, 9], [[1, 7, 2], [1, 2, 8], [1, 2]], [2, 1, 1])
    mx, sm = np.full(3, 5.0, np.float32), np.full(3, 2.0, np.float32)
    ts = np.array([1.0, 2.0, 3.0], dtype=np.float32)
    rank = np.array([1, 1, 1], dtype=np.int32)
    got = ref.offer(seq, hep, mx, sm, ts, rank, val, ids0, status, 1, NAN, N)
    assert _untouched(got, val, ids0, status, 0)
    assert _offered(got, val, ids0, status, 1, 2.0, 8) and _offered(got, val, ids0, status, 2, 3.0, 9)
    # the exclusion list of the row's USER: 0-based ids, user 0 lists item 8, user 1 items 8 and 4, user 2 nothing.  First rows
    # 0, 1, 2 belong to users 2, 0, 1
    excl = np.array([[7, -1], [7, 3], [-1, -1]], dtype=np.int64)
    got = ref.offer(seq, hep, mx, sm, ts, rank, val, ids0, status, 1, NAN, N, excl=excl, user_of=[2, 0, 1])
    assert got[3].tolist() == [False, False, True] and _untouched(got, val, ids0, status, 1)
    got = ref.offer(seq, hep, mx, sm, ts, rank, val, ids0, status, 1, NAN, N, excl=excl)  # the identity: row 1 is user 1
    assert got[3].tolist() == [False, False, True]
    got = ref.offer(seq, hep, mx, sm, ts, rank, val, ids0, status, 1, NAN, N, excl=excl, user_of=[0, 2, 1])
    assert got[3].tolist() == [False, True, True]
    # the path under no_repeat: entries [0, step) only
    paths = np.array([[5, 9, 9], [5, 6, 8], [9, 6, 0]], dtype=np.float32)
    got = ref.offer(seq, hep, mx, sm, ts, rank, val, ids0, status, 1, NAN, N, no_repeat=True, paths=paths, step=2)
    assert got[3].tolist() == [False, True, False]  # row 1: 8 sits at entry 2, not yet walked; row 2: 9 at entry 0
    got = ref.offer(seq, hep, mx, sm, ts, rank, val, ids0, status, 1, NAN, N, no_repeat=True, paths=paths, step=3)
    assert got[3].tolist() == [False, False, False]
    got = ref.offer(seq, hep, mx, sm, ts, rank, val, ids0, status, 1, NAN, N, no_repeat=False, paths=paths, step=3)
    assert got[3].tolist() == [False, True, True]
    # a finished row, and a target outside the catalog
    got = ref.offer(seq, hep, mx, sm, ts, rank, val, ids0, status, 1, NAN, N, fin=[0, 1, 0])
    assert got[3].tolist() == [False, False, True]
    got = ref.offer(seq, hep, mx, sm, ts, rank, val, ids0, status, 1, NAN, 8)
    assert got[3].tolist() == [False, True, False]


def test_replay_and_until_stats():
    P = 4
    seq, hep = _rows([7, 8, 9], [[1, 2], [1, 8], [1, 2]], [1, 1, 1])
    paths = np.array([[3, 4, 7, 5], [3, 4, 5, 6], [3, 4, 5, 6]], dtype=np.float32)  # user 0 arrives by itself at step 2
    lp_t = np.array([[-5, -4, -1, -3], [-1, -1, -1, -1], [-6, -3, -2, -2]], dtype=np.float32)
    lp_i = np.full((3, P), -0.5, dtype=np.float32)
    lp_i[0, 2] = -1
    rk = np.array([[9, 4, 1, 6], [1, 1, 1, 1], [20, 7, 2, 2]], dtype=np.int32)
    # rank <= 4: user 0 fires at step 1 (before its own arrival), user 1 never (its target sits in its window), user 2 at step 2
    got, tr, n, arrived, offered = ref.replay(seq, hep, paths, (lp_i, lp_t, rk), 4, NAN, N)
    assert got.tolist() == [[3, 7, 0, 0], [3, 4, 5, 6], [3, 4, 9, 0]]
    assert n.tolist() == [2, 4, 3] and arrived.tolist() == [True, False, True] and offered.tolist() == [True, False, True]
    assert tr[0].tolist() == [[-0.5, -4, 0, 0], [-0.5] * 4, [-0.5, -0.5, -2, 0]]  # lp_item of a fired step is lp_target
    assert tr[1].tolist() == [[-5, -4, 0, 0], [-1] * 4, [-6, -3, -2, 0]] and tr[2].tolist() == [[9, 4, 0, 0], [1] * 4, [20, 7, 2, 0]]
    # rank <= 1: at step 2 user 0's target is the best item the window leaves -- the search chose it anyway, and the rule fired
    got, tr, n, arrived, offered = ref.replay(seq, hep, paths, (lp_i, lp_t, rk), 1, NAN, N)
    assert got.tolist() == [[3, 4, 7, 0], [3, 4, 5, 6], [3, 4, 5, 6]] and offered.tolist() == [True, False, False]
    assert n.tolist() == [3, 4, 4] and tr[0][0].tolist() == [-0.5, -0.5, -1, 0]
    # the probability clause: lp >= -3 -> user 0 at step 2, user 2 at step 1
    got, _, n, _, offered = ref.replay(seq, hep, paths, (lp_i, lp_t, rk), 0, -3.0, N)
    assert n.tolist() == [3, 4, 2] and got[2].tolist() == [3, 9, 0, 0]
    # the loop's counts: check_every 1: 3 rows, 3 rows, 2 rows (user 0 left), 1 row (user 2 left)
    n, arrived = np.array([2, 4, 3]), np.array([True, False, True])
    assert ref.until_stats(n, arrived, P, 1) == (4, 3 + 3 + 2 + 1)
    assert ref.until_stats(n, arrived, P, 3) == (4, 3 + 3 + 3 + 1)
    assert ref.until_stats(np.array([1, 1]), np.array([True, True]), P, 1) == (1, 2)
    assert ref.until_stats(np.array([1, 1]), np.array([True, True]), P, 3) == (3, 6)


# ---------------------------------------------------------------- declared, exported, bound
def test_names_and_status_bit_in_header_exports_and_ctypes_table():
    lib = _lib.load()
    txt = open(os.path.join(REPO, "include", "irs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("irs_set_arrival_rule", 3), ("irs_arrival_offer", 20)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["irs_set_arrival_rule"][1][2] is ctypes.c_float
    assert re.search(r"#define\s+IRS_ROW_OFFERED\s+16\b", code) and _lib.IRS_ROW_OFFERED == 16 == ref.OFFERED
    bits = [_lib.IRS_ROW_FALLBACK, _lib.IRS_ROW_NO_CANDIDATE, _lib.IRS_ROW_FEWER_THAN_K, _lib.IRS_ROW_RESCUED, _lib.IRS_ROW_OFFERED]
    assert sorted(bits) == [1, 2, 4, 8, 16]
    for phrase in ("rk <= rank_max", "lp >= lp_min", "a NaN lp never fires", "(-inf, -1)", "out of scope"):
        assert phrase in txt, phrase


# ---------------------------------------------------------------- the setter and the loops' state check, without a device
def test_setter_checks_and_the_loops_need_a_trace():
    lib, h = _ctx()
    p = ctypes.c_void_p
    q = p(4096)
    try:
        ws = lib.irs_workspace_bytes(h)
        f = lib.irs_set_arrival_rule
        assert f(None, 1, NAN) == INVALID
        assert f(h, -1, NAN) == INVALID and b"rank_max" in lib.irs_last_error(h)
        assert f(h, -1, -1.0) == INVALID

        def paths():
            return lib.irs_generate_paths(h, q, q, q, 4, 3, 10, 0, 0, 0, 0, 0, q, q, None)

        def until():
            return lib.irs_generate_paths_until(h, q, q, q, 4, 3, 10, 0, 0, 0, 0, 1, q, q, None, None)

        def refused():
            return (paths() == STATE and b"irs_bind_path_trace" in lib.irs_last_error(h)
                    and until() == STATE and b"irs_set_arrival_rule" in lib.irs_last_error(h))

        def clear():  # no rule: the loops get as far as the missing weights, another message
            return (paths() == STATE and b"irs_set_arrival_rule" not in lib.irs_last_error(h)
                    and until() == STATE and b"irs_set_arrival_rule" not in lib.irs_last_error(h))

        assert clear()
        for rank_max, lp_min in ((1, NAN), (0, 0.0), (0, -INF), (3, -2.5), (7, 1.0)):
            assert f(h, rank_max, lp_min) == 0 and refused(), (rank_max, lp_min)
        for rank_max, lp_min in ((0, NAN), (0, 0.5), (0, INF)):  # both clauses off: the rule is cleared
            assert f(h, 2, -1.0) == 0 and refused()
            assert f(h, rank_max, lp_min) == 0 and clear(), (rank_max, lp_min)
        # with a trace bound the loops get past the rule's check (to the missing weights); the beam loops refuse the rule itself
        assert f(h, 2, NAN) == 0
        assert lib.irs_beam_search(h, q, q, q, 2, 2, 3, 10, 0, 0, q, q, None, q, None) == UNSUPPORTED
        assert b"irs_set_arrival_rule" in lib.irs_last_error(h)
        need = lib.irs_path_trace_scratch_bytes(h, 8)
        assert lib.irs_bind_path_trace(h, q, q, q, 8, 4, q, need) == 0
        assert clear()
        assert lib.irs_bind_path_trace(h, None, None, None, 0, 0, None, 0) == 0
        assert refused()
        assert f(h, 0, NAN) == 0 and f(h, 0, NAN) == 0 and clear()
        assert lib.irs_workspace_bytes(h) == ws
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        assert lib.irs_set_arrival_rule(h, 1, NAN) == UNSUPPORTED and lib.irs_set_arrival_rule(h, 0, -1.0) == UNSUPPORTED
        assert lib.irs_set_arrival_rule(h, 0, NAN) == 0  # nothing to clear is fine anywhere
    finally:
        lib.irs_destroy(h)


def test_stand_alone_kernel_argument_checks():
    lib, h = _ctx()
    p = ctypes.c_void_p
    q = p(4096)
    f = lib.irs_arrival_offer

    def call(**kw):
        a = dict(seq=q, hep=q, M=8, mx=q, sm=q, ts=q, rank=q, fin=None, val=q, ids0=q, k=10, rank_max=1, lp_min=NAN, paths=None,
                 path_ld=0, step=0, row_map=None, status=q)
        a.update(kw)
        return f(h, a["seq"], a["hep"], a["M"], a["mx"], a["sm"], a["ts"], a["rank"], a["fin"], a["val"], a["ids0"], a["k"],
                 a["rank_max"], a["lp_min"], a["paths"], a["path_ld"], a["step"], a["row_map"], a["status"], None)

    try:
        assert f(None, q, q, 8, q, q, q, q, None, q, q, 10, 1, NAN, None, 0, 0, None, q, None) == INVALID
        for name in ("seq", "hep", "mx", "sm", "ts", "rank", "val", "ids0", "status"):
            assert call(**{name: None}) == INVALID and b"null" in lib.irs_last_error(h), name
        for bad in (dict(M=0), dict(M=-3), dict(k=0), dict(k=101), dict(rank_max=-1), dict(rank_max=0, lp_min=NAN),
                    dict(rank_max=0, lp_min=0.25), dict(step=-1), dict(paths=q, path_ld=0), dict(paths=q, path_ld=4, step=5)):
            assert call(**bad) == INVALID, bad
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        assert f(h, q, q, 8, q, q, q, q, None, q, q, 10, 1, NAN, None, 0, 0, None, q, None) == UNSUPPORTED
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- Python layers
def test_keywords_are_off_by_default_and_the_front_end_refuses_without_a_device():
    import inspect

    from influentialrs_amd import synth
    from influentialrs_amd.engine import Engine
    from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
    for fn in (Engine.generate_paths, Engine.generate_paths_until):
        par = inspect.signature(fn).parameters
        assert par["arrive_rank"].default is None and par["arrive_lp"].default is None, fn
    assert hasattr(Engine, "set_arrival_rule") and hasattr(Engine, "arrival_offer")
    sig = inspect.signature(IRSNN.get_seq_in_batch, follow_wrapped=False).parameters
    for name in ("arrive_rank", "arrive_lp"):
        assert sig[name].default is None and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
    # the positional signature is what it was
    assert list(inspect.signature(IRSNN.get_seq_in_batch).parameters) == [
        "self", "seqs", "users", "targets", "max_path_len", "gap_len", "sample", "sample_k", "beam_width", "stop_at_target", "beam_stop"]
    cfg = synth.make_config("tiny")
    net = InfluentialNet(cfg)
    irn = IRSNN(cfg, net, "cpu")
    B = 2
    seqs, users, targets = torch.ones((B, cfg.max_len), dtype=torch.int64), torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.int64)
    for bad in (dict(arrive_rank=0), dict(arrive_rank=-2), dict(arrive_rank=1.5), dict(arrive_rank=True)):
        with pytest.raises(ValueError, match="arrive_rank="):
            irn.get_seq_in_batch(seqs, users, targets, 5, 0, **bad)
    for bad in (dict(arrive_lp=0.5), dict(arrive_lp=NAN), dict(arrive_rank=3, arrive_lp=INF)):
        with pytest.raises(ValueError, match="arrive_lp="):
            irn.get_seq_in_batch(seqs, users, targets, 5, 0, **bad)
    with pytest.raises(ValueError, match="arrive_rank / arrive_lp is not built for beam search"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, beam_width=2, arrive_rank=3)
    net.shard_items(0, 2, drop_full=False)
    with pytest.raises(ValueError, match="arrive_rank / arrive_lp is not built for an item-sharded catalog"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, arrive_lp=-1.0)
    assert irn._arrive_rank is None and irn._arrive_lp is None and irn._trace is False, "the switches last for the call"
