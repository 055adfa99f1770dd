"""not-gpu: the lookahead choice (irs_bind_lookahead): the numpy statement (tests/lookahead_ref.py) against path_ref's greedy
search, guided_ref's survivor collection and path_ref's window update; every choose rule on hand-made rows; the new symbols in
header, library and ctypes table; the scratch size; every refusal of the binding and of the bound entry points on a context
created without a device; and the Python layers."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import guided_ref
import lookahead_ref as ref
import path_ref
from influentialrs_amd import _lib, synth
from influentialrs_amd.engine import Engine
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, UNSUPPORTED = -1, -2, -4
NINF, NAN = np.float32(-np.inf), np.float32(np.nan)


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


def _lists(g, B, k, n_item):
    ids0 = np.stack([g.permutation(n_item)[:k] for _ in range(B)]).astype(np.int64)
    val = -np.sort(-g.standard_normal((B, k)).astype(np.float32), axis=1)
    return val, ids0


def _state(g, B, L, n_item, heps):
    seq = g.integers(1, n_item + 1, size=(B, L)).astype(np.int64)
    hep = np.array([heps[r % len(heps)] for r in range(B)], dtype=np.int32)
    return seq, hep


# ---------------------------------------------------------------- the statement
def _toy_model(n_item, seed):
    """A deterministic stand-in for decoder and catalog: the ranker orders the catalog by a hash of the window, the scorer gives
    the target a value that depends on the child's last chosen item."""
    w = np.random.default_rng(seed).standard_normal((n_item + 1, n_item + 1)).astype(np.float32)

    def last(seq_row, he):
        return int(seq_row[min(int(he), len(seq_row) - 2)])

    def ranker(seq, hep, users):
        B = len(seq)
        val = np.zeros((B, n_item), dtype=np.float32)
        ids0 = np.zeros((B, n_item), dtype=np.int64)
        for r in range(B):
            s = w[last(seq[r], hep[r]) % (n_item + 1), 1:]
            order = np.argsort(-s, kind="stable")
            val[r], ids0[r] = s[order], order
        return val[:, :12], ids0[:, :12]

    def scorer(c_seq, c_hep, c_user, c_tgt):
        n = len(c_seq)
        ts = np.array([w[last(c_seq[c], c_hep[c]) % (n_item + 1), int(c_tgt[c]) + 1] if c_tgt[c] >= 0 else NINF for c in range(n)],
                      dtype=np.float32)
        return ts, np.zeros(n, dtype=np.float32), np.ones(n, dtype=np.float32)
    return ranker, scorer


def _greedy_search(seq, hep, P, ranker):
    seq, hep = np.array(seq), np.array(hep)
    paths, status = np.zeros((len(seq), P), dtype=np.float32), np.zeros(len(seq), dtype=np.int32)
    for i in range(P):
        val, ids0 = ranker(seq, hep, None)
        seq, hep, paths, status = path_ref.path_step(seq, hep, val, ids0, i, paths, status)
    return paths, seq, hep, status


def test_k_c_one_is_the_greedy_search_and_a_larger_k_c_moves_it():
    g = np.random.default_rng(11)
    n_item, B, L, P = 40, 7, 8, 6
    seq, hep = _state(g, B, L, n_item, [1, L - 3, L - 2, 3])
    ranker, scorer = _toy_model(n_item, 5)
    want = _greedy_search(seq, hep, P, ranker)
    got = ref.search(seq, hep, None, P, 1, ranker, scorer)
    assert all(np.array_equal(a, b) for a, b in zip(want, got[:4]))
    assert (got[6] == 0).all() and (got[4][:, :, 0] == want[0].astype(np.int32)).all()
    moved = ref.search(seq, hep, None, P, 5, ranker, scorer)
    assert (moved[0] != want[0]).any() and (moved[6] > 0).any()
    # every choice is the best of its recorded row under the stated order, or the target itself
    for b in range(B):
        for i in range(P):
            items = [int(x) for x in moved[4][b, i] if x > 0]
            c = ref.choose_index(moved[5][b, i], items, int(seq[b, L - 1]))
            assert moved[0][b, i] == items[c] == items[moved[6][b, i]]


def test_until_freezes_a_user_behind_its_target():
    g = np.random.default_rng(2)
    n_item, B, L, P = 30, 6, 7, 6
    seq, hep = _state(g, B, L, n_item, [1, 2])
    ranker, scorer = _toy_model(n_item, 9)
    plain = ref.search(seq, hep, None, P, 4, ranker, scorer)
    seq[:, L - 1] = plain[0][:, 2]  # everybody arrives at step 2 at the latest
    plain = ref.search(seq, hep, None, P, 4, ranker, scorer)
    until = ref.search(seq, hep, None, P, 4, ranker, scorer, until=True)
    for b in range(B):
        n = int(np.where(plain[0][b] == seq[b, L - 1])[0][0]) + 1
        assert n <= 3 and np.array_equal(until[0][b, :n], plain[0][b, :n]) and not until[0][b, n:].any()
        assert np.array_equal(until[4][b, :n], plain[4][b, :n]) and not until[4][b, n:].any() and not until[5][b, n:].any()


def test_survivor_collection_is_the_guided_steps():
    """The candidates of expand are the survivors guided_ref's step chooses among: the same walk, exclusions and path included."""
    g = np.random.default_rng(4)
    n_item, B, L, k = 50, 9, 9, 14
    seq, hep = _state(g, B, L, n_item, [0, 2, L - 3, L - 2])
    val, ids0 = _lists(g, B, k, n_item)
    ids0[1, 4:] = -1
    ids0[2, :] = seq[2, 0] - 1  # only an item the window holds
    ids0[2, 1:] = -1
    for r in range(B):
        seq[r, :min(3, hep[r] + 1)] = ids0[r, :min(3, hep[r] + 1)] + 1  # the window hides leading candidates
    excl = g.integers(0, n_item, size=(B, 6)).astype(np.int64)
    excl[:, 0] = ids0[:, 3]
    paths = np.zeros((B, 4), dtype=np.float32)
    paths[:, 0] = ids0[:, 4] + 1
    for k_c in (1, 3, 14):
        for kw in (dict(), dict(excl=excl, n_item=n_item, paths=paths, step=1, no_repeat=True)):
            out = ref.expand(seq, hep, None, val, ids0, k_c, **kw)
            for r in range(B):
                v, i = val[r], ids0[r]
                if kw:
                    import exclusion_ref
                    v, i = exclusion_ref.strike(v, i, exclusion_ref.hidden(excl[r], n_item, paths[r], 1, True))
                surv = path_ref.survivors(seq[r, :hep[r] + 1], v, i, k_c)
                assert [int(x) + 1 for x in out[4][r] if x >= 0] == [s[0] for s in surv]
                assert (out[4][r, len(surv):] == -1).all() and (out[5][r, len(surv):] == NINF).all()
                assert [float(x) for x in out[5][r, :len(surv)]] == [float(s[1]) for s in surv]
    # and a table under which every distance ties makes the guided step take candidate 0 of expand
    table = np.zeros((n_item + 1, 3), dtype=np.float32)
    st = np.zeros(B, dtype=np.int32)
    guided = guided_ref.path_step(seq, hep, val, ids0, 1, paths, st, table, guided_ref.FLOAT, 5)
    c_ids = ref.expand(seq, hep, None, val, ids0, 5)[4]
    for r in range(B):
        assert guided[2][r, 1] == (c_ids[r, 0] + 1 if c_ids[r, 0] >= 0 else 0)
    assert guided[3][2] == path_ref.NO_CANDIDATE and (c_ids[2] == -1).all()


def test_child_window_is_the_path_steps_window():
    g = np.random.default_rng(6)
    n_item, L, k, k_c = 60, 10, 8, 4
    heps = [0, 3, L - 3, L - 2]  # three that grow (the last one into slot L - 2), one that shifts
    B = len(heps)
    seq, hep = _state(g, B, L, n_item, heps)
    seq[:, 0] = 0
    val, ids0 = _lists(g, B, k, n_item)
    users = np.arange(B, dtype=np.int64) + 3
    c_seq, c_hep, c_user, c_tgt, c_ids, c_val = ref.expand(seq, hep, users, val, ids0, k_c)
    for r in range(B):
        for j in range(k_c):
            c = r * k_c + j
            assert c_ids[r, j] >= 0 and c_user[c] == users[r] and c_tgt[c] == seq[r, L - 1] - 1
            one_v = np.array([[c_val[r, j], NINF]], dtype=np.float32)
            one_i = np.array([[c_ids[r, j], -1]], dtype=np.int64)
            s2, h2, p2, st2 = path_ref.path_step(seq[r:r + 1], hep[r:r + 1], one_v, one_i, 0, np.zeros((1, 2), dtype=np.float32),
                                                 np.zeros(1, dtype=np.int32))
            assert np.array_equal(c_seq[c], s2[0]) and c_hep[c] == h2[0] and p2[0, 0] == c_ids[r, j] + 1
            assert c_seq[c, L - 1] == seq[r, L - 1], "the target stays in slot L - 1"
    assert c_hep[0] == 1 and c_hep[2 * k_c] == L - 2 and c_hep[3 * k_c] == L - 2
    assert np.array_equal(c_seq[3 * k_c, :L - 3], seq[3, 1:L - 2]), "a shift moves every position"
    # a slot without a survivor: a copy of the parent, id -1
    ids0[1, 2:] = -1
    out = ref.expand(seq, hep, users, val, ids0, k_c)
    assert np.array_equal(out[0][1 * k_c + 3], seq[1]) and out[1][1 * k_c + 3] == hep[1] and out[4][1, 3] == -1
    # a finished row: no candidates at all
    out = ref.expand(seq, hep, users, val, ids0, k_c, fin=np.array([0, 0, 1, 0]))
    assert (out[4][2] == -1).all() and np.array_equal(out[0][2 * k_c], seq[2])


# ---------------------------------------------------------------- the choose rules
def _choose(lp_row, items, target, k=4):
    n, k_c = len(items), len(lp_row)
    seq = np.array([[7, 8, 0, target]], dtype=np.int64)
    c_ids = np.full((1, k_c), -1, dtype=np.int64)
    c_ids[0, :n] = np.array(items, dtype=np.int64) - 1
    c_val = np.full((1, k_c), NINF, dtype=np.float32)
    c_val[0, :n] = 10.0 - np.arange(n)
    val = np.arange(k, dtype=np.float32)[None, ::-1].copy()
    ids0 = np.arange(100, 100 + k, dtype=np.int64)[None].copy()
    return ref.choose(seq, c_ids, c_val, np.array([lp_row], dtype=np.float32), val, ids0), (val, ids0)


def test_choose_rules_on_hand_made_rows():
    (v, i, c), _ = _choose([-3, -2, -2.5], [11, 12, 13], 50)
    assert c[0] == 1 and i[0].tolist() == [11, -1, 102, 103] and v[0, 0] == 9.0 and v[0, 1] == NINF, "strict improvement"
    (v, i, c), _ = _choose([-3, -1, -1, -1], [11, 12, 13, 14], 50)
    assert c[0] == 1, "ties go to the better rank"
    (v, i, c), _ = _choose([-1, -1, -1], [11, 12, 13], 50)
    assert c[0] == 0
    (v, i, c), _ = _choose([NAN, -9, -8], [11, 12, 13], 50)
    assert c[0] == 2, "a NaN is replaced by anything that is not a NaN"
    (v, i, c), _ = _choose([-5, NAN, -6], [11, 12, 13], 50)
    assert c[0] == 0, "a NaN never replaces anything"
    (v, i, c), _ = _choose([NAN, NAN], [11, 12], 50)
    assert c[0] == 0
    (v, i, c), _ = _choose([NINF, NINF, NINF], [11, 12, 13], 0)
    assert c[0] == 0 and i[0, 0] == 10 and v[0, 0] == 10.0, "all -inf: the first survivor, the greedy choice"
    (v, i, c), _ = _choose([-1, -9, -2], [11, 50, 13], 50)
    assert c[0] == 1 and i[0, 0] == 49, "the target among the candidates is chosen outright"
    (v, i, c), _ = _choose([-4, -1, NINF, NINF], [11, 12], 50)
    assert c[0] == 1, "slots without a candidate do not compete"
    (v, i, c), (v0, i0) = _choose([NINF, NINF], [], 50)
    assert c[0] == -1 and np.array_equal(i, i0) and np.array_equal(v, v0), "no survivor: the list is not written"
    (v, i, c), _ = _choose([-3, -2], [11, 12], 50, k=1)
    assert c[0] == 1 and i.tolist() == [[11]], "k = 1 has no entry 1 to end the list at"
    seq = np.array([[1, 2, 3, 50]], dtype=np.int64)
    val, ids0 = np.array([[5.0, 4.0]], dtype=np.float32), np.array([[20, 21]], dtype=np.int64)
    v, i, c = ref.choose(seq, np.array([[30, 31]]), np.array([[5.0, 4.0]], dtype=np.float32), np.array([[-2.0, -1.0]], dtype=np.float32),
                         val, ids0, fin=np.array([1]))
    assert c[0] == -1 and np.array_equal(i, ids0) and np.array_equal(v, val), "a finished row stays untouched"


def test_lp_is_the_trace_expression():
    ts = np.array([[1.5, -np.inf, 2.0]], dtype=np.float32)
    mx = np.array([[3.0, 3.0, 3.0]], dtype=np.float32)
    sm = np.array([[7.0, 7.0, 7.0]], dtype=np.float32)
    lp = ref.lp_values(ts, mx, sm, np.array([[4, 5, -1]]))
    assert lp[0, 0] == np.float32(1.5 - (3.0 + np.log(7.0))) and lp[0, 1] == NINF and lp[0, 2] == NINF and lp.dtype == np.float32


# ---------------------------------------------------------------- symbols, scratch size
def test_new_symbols_in_header_library_table_and_build():
    txt = open(os.path.join(REPO, "include", "irs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = ("irs_lookahead_scratch_bytes", "irs_bind_lookahead", "irs_lookahead_expand", "irs_lookahead_choose")
    lib = _lib.load()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define IRS_MAX_LOOKAHEAD_KC 32\b", code) and _lib.IRS_MAX_LOOKAHEAD_KC == ref.MAX_KC == 32
    assert "lookahead choice" in txt and "irs_decoder_route_last reports the INNER decode" in txt
    sig = _lib.SIGNATURES
    assert sig["irs_lookahead_scratch_bytes"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32])
    assert len(sig["irs_bind_lookahead"][1]) == 8 and sig["irs_bind_lookahead"][1][3] is ctypes.c_size_t
    assert len(sig["irs_lookahead_expand"][1]) == 20 and len(sig["irs_lookahead_choose"][1]) == 15
    for name in ("irs_lookahead_expand", "irs_lookahead_choose"):  # the kernels alone are synchronous: no stream argument
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code).group(1)
        assert "stream" not in decl, name
    from influentialrs_amd import build
    assert "lookahead.hip" in build.SOURCES


def test_scratch_bytes_and_the_unchanged_workspace():
    lib, h = _ctx()
    try:
        f = lib.irs_lookahead_scratch_bytes
        assert f(None, 4, 3) == 0
        for rows, k_c in ((0, 3), (-1, 3), (4, 0), (4, -1), (4, 33)):
            assert f(h, rows, k_c) == 0, (rows, k_c)

        def up(v):
            return (v + 255) // 256 * 256
        for rows, k_c in ((1, 1), (6, 5), (64, 32), (70, 3)):
            N, L, d = rows * k_c, 60, 30
            want = up(N * L * 8) + 3 * up(N * 8) + 7 * up(N * 4) + up(N * d * 4) + up(rows * 4)
            assert f(h, rows, k_c) == want and want % 256 == 0, (rows, k_c)
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- refusals, before any launch
def test_bind_refusals_without_a_device():
    p = ctypes.c_void_p
    a, big = p(4096), 1 << 30
    lib, h = _ctx()
    try:
        f = lib.irs_bind_lookahead

        def err():
            return lib.irs_last_error(h)
        assert f(None, 3, a, big, None, None, 8, 4) == INVALID
        assert f(h, 0, None, 0, None, None, 0, 0) == 0, "unbinding what was never bound is fine"
        assert f(h, -1, a, big, None, None, 8, 4) == INVALID and b"irs_bind_lookahead" in err() and b"k_c" in err()
        assert f(h, 33, a, big, None, None, 8, 4) == INVALID and b"32" in err()
        assert f(h, 3, a, big, None, None, 0, 4) == INVALID and f(h, 3, a, big, None, None, 8, 0) == INVALID
        assert f(h, 3, a, big, a, None, 8, 4) == INVALID and b"go together" in err()
        need = lib.irs_lookahead_scratch_bytes(h, 8, 3)
        assert f(h, 3, a, need - 1, None, None, 8, 4) == INVALID and b"too small" in err() and b"irs_bind_lookahead" in err()
        assert f(h, 3, None, need, None, None, 8, 4) == INVALID
        assert f(h, 3, p(4096 + 8), big, None, None, 8, 4) == INVALID and b"aligned" in err()
        # nothing of the above bound anything: a sampled loop call gets as far as the unbound weights
        assert lib.irs_generate_paths(h, a, a, a, 8, 3, 100, 0, 1, 3, 0, 0, a, a, None) == STATE
        # one choice rule at a time, both ways round
        assert f(h, 3, a, need, None, None, 8, 4) == 0
        assert lib.irs_bind_guide(h, _lib.IRS_GUIDE_FLOAT, a, 8, 5, None, 0, None) == UNSUPPORTED and b"irs_bind_lookahead" in err()
        assert f(h, 0, None, 0, None, None, 0, 0) == 0
        assert lib.irs_bind_guide(h, _lib.IRS_GUIDE_FLOAT, a, 8, 5, None, 0, None) == 0
        assert f(h, 3, a, need, None, None, 8, 4) == UNSUPPORTED and b"irs_bind_guide" in err() and b"irs_bind_lookahead" in err()
        assert lib.irs_bind_guide(h, 0, None, 0, 0, None, 0, None) == 0
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        assert lib.irs_bind_lookahead(h, 3, a, big, None, None, 8, 4) == UNSUPPORTED
        assert b"irs_bind_lookahead" in lib.irs_last_error(h) and b"whole catalog" in lib.irs_last_error(h)
        assert lib.irs_bind_lookahead(h, 0, None, 0, None, None, 0, 0) == 0
    finally:
        lib.irs_destroy(h)


def test_bound_entry_points_refuse_without_a_device():
    """The binding launches nothing, so the checks of the bound entry points can be reached on a context that has no device: each
    names the binding, and none of them gets as far as the unbound weights."""
    p = ctypes.c_void_p
    a, big = p(4096), 1 << 30
    lib, h = _ctx()
    try:
        assert lib.irs_bind_lookahead(h, 5, a, big, a, a, 16, 4) == 0

        def err():
            return lib.irs_last_error(h)
        gp, gu = lib.irs_generate_paths, lib.irs_generate_paths_until
        assert gp(h, a, a, a, 8, 3, 100, 0, 1, 3, 0, 0, a, a, None) == UNSUPPORTED and b"sample" in err() and b"irs_generate_paths" in err()
        assert gp(h, a, a, a, 8, 3, 4, 0, 0, 0, 0, 1, a, a, None) == INVALID and b"k=4 < k_c=5" in err()
        assert gp(h, a, a, a, 17, 3, 100, 0, 0, 0, 0, 0, a, a, None) == INVALID and b"16 users" in err()
        assert gp(h, a, a, a, 8, 5, 100, 0, 0, 0, 0, 0, a, a, None) == INVALID and b"4 steps" in err()
        assert gp(h, a, a, a, 13, 3, 100, 0, 0, 0, 0, 0, a, a, None) == INVALID
        assert b"B*k_c=65" in err() and b"max_seqs=64" in err() and b"max_rows=64" in err()
        assert gu(h, a, a, a, 8, 3, 100, 0, 1, 3, 0, 1, a, a, None, None) == UNSUPPORTED and b"irs_generate_paths_until" in err()
        assert gu(h, a, a, a, 8, 3, 4, 0, 0, 0, 0, 1, a, a, None, None) == INVALID
        assert gu(h, a, a, a, 13, 3, 100, 0, 0, 0, 0, 1, a, a, None, None) == INVALID and b"B*k_c=65" in err()
        assert lib.irs_beam_step(h, a, a, a, a, a, a, a, a, 2, 2, 10, 0, 3, a, a, a, a, a, None) == UNSUPPORTED and b"irs_bind_lookahead" in err()
        assert lib.irs_beam_step_until(h, a, a, a, a, a, a, a, a, a, 2, 2, 10, 0, 3, 0, a, a, a, a, a, a, a, None) == UNSUPPORTED
        assert lib.irs_beam_search(h, a, a, a, 2, 2, 3, 100, 0, 0, a, a, None, a, None) == UNSUPPORTED and b"greedy loops only" in err()
        assert lib.irs_beam_search_until(h, a, a, a, 2, 2, 3, 100, 0, 0, 1, a, a, None, None, a, None, None) == UNSUPPORTED
        # accepted arguments get as far as the unbound weights
        assert gp(h, a, a, a, 8, 3, 100, 0, 0, 0, 0, 0, a, a, None) == STATE
        # without a record the path length is free
        assert lib.irs_bind_lookahead(h, 5, a, big, None, None, 16, 4) == 0
        assert gp(h, a, a, a, 8, 9, 100, 0, 0, 0, 0, 0, a, a, None) == STATE
        # and an unbind restores the unbound checks
        assert lib.irs_bind_lookahead(h, 0, None, 0, None, None, 0, 0) == 0
        assert gp(h, a, a, a, 8, 3, 4, 0, 1, 3, 0, 0, a, a, None) == STATE
        assert lib.irs_beam_search(h, a, a, a, 2, 2, 3, 100, 0, 0, a, a, None, a, None) == STATE
    finally:
        lib.irs_destroy(h)


def test_kernel_entry_points_refuse_without_a_device():
    p = ctypes.c_void_p
    a = p(4096)
    lib, h = _ctx()
    try:
        ex, ch = lib.irs_lookahead_expand, lib.irs_lookahead_choose

        def err():
            return lib.irs_last_error(h)
        ok = (a, a, a, 4, a, a, 10, 3, None, None, 0, 0, None, a, a, a, a, a, a)
        assert ex(None, *ok) == INVALID
        for at in (0, 1, 4, 5, 13, 14, 15, 16, 17, 18):  # every required pointer
            bad = list(ok)
            bad[at] = None
            assert ex(h, *bad) == INVALID and b"irs_lookahead_expand" in err(), at
        assert ex(h, a, a, None, 4, a, a, 10, 3, None, None, 0, 0, None, a, a, a, a, a, a) == INVALID and b"user" in err()
        assert ex(h, a, a, a, 0, a, a, 10, 3, None, None, 0, 0, None, a, a, a, a, a, a) == INVALID
        assert ex(h, a, a, a, 4, a, a, 101, 3, None, None, 0, 0, None, a, a, a, a, a, a) == INVALID and b"k must be" in err()
        for k_c in (0, -1, 11, 33):
            assert ex(h, a, a, a, 4, a, a, 10, k_c, None, None, 0, 0, None, a, a, a, a, a, a) == INVALID and b"k_c" in err()
        assert ex(h, a, a, a, 4, a, a, 10, 3, None, a, 4, 5, None, a, a, a, a, a, a) == INVALID and b"step" in err()
        assert ex(h, a, a, a, 4, a, a, 10, 3, None, None, 0, -1, None, a, a, a, a, a, a) == INVALID
        okc = (a, 4, 3, a, a, a, a, a, None, a, a, 10, a, a)
        for at in (0, 3, 4, 5, 6, 7, 9, 10, 12, 13):
            bad = list(okc)
            bad[at] = None
            assert ch(h, *bad) == INVALID and b"irs_lookahead_choose" in err(), at
        assert ch(h, a, 4, 11, a, a, a, a, a, None, a, a, 10, a, a) == INVALID and b"k_c" in err()
        assert ch(h, a, 0, 3, a, a, a, a, a, None, a, a, 10, a, a) == INVALID
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        assert lib.irs_lookahead_expand(h, a, a, a, 4, a, a, 10, 3, None, None, 0, 0, None, a, a, a, a, a, a) == UNSUPPORTED
        assert lib.irs_lookahead_choose(h, a, 4, 3, a, a, a, a, a, None, a, a, 10, a, a) == UNSUPPORTED
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- Python layers
def test_keywords_are_off_by_default_and_keyword_only():
    for fn in (Engine.generate_paths, Engine.generate_paths_until):
        par = inspect.signature(fn).parameters
        assert par["lookahead"].default is None and par["lookahead_record"].default is False, fn
    for fn in (Engine.beam_search, Engine.beam_search_until, Engine.generate_paths_sharded):
        assert "lookahead" not in inspect.signature(fn).parameters, fn
    for name in ("lookahead_scratch_bytes", "bind_lookahead", "unbind_lookahead", "lookahead_expand", "lookahead_choose", "_search_options"):
        assert hasattr(Engine, name), name
    par = inspect.signature(Engine.bind_lookahead).parameters
    assert list(par) == ["self", "k_c", "users", "ld", "record"] and par["record"].default is False
    sig = inspect.signature(IRSNN.get_seq_in_batch, follow_wrapped=False).parameters
    for name, default in (("lookahead", None), ("lookahead_record", False)):
        assert sig[name].default is default and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
    declared = list(inspect.signature(IRSNN.get_seq_in_batch).parameters)
    assert declared == ["self", "seqs", "users", "targets", "max_path_len", "gap_len", "sample", "sample_k", "beam_width", "stop_at_target",
                        "beam_stop"], "the positional signature is unchanged"


def test_irn_front_end_refuses_without_a_device():
    cfg = synth.make_config("tiny")
    irn = IRSNN(cfg, InfluentialNet(cfg), "cpu")
    B, L = 2, cfg.max_len
    seqs, users, targets = torch.ones((B, L), dtype=torch.int64), torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.int64)
    table = torch.zeros((cfg.n_item + 1, 4))
    for bad in (0, 33, -1, 2.0, "3", True):
        with pytest.raises(ValueError, match="lookahead=.*an int from 1 to 32"):
            irn.get_seq_in_batch(seqs, users, targets, 5, 0, lookahead=bad)
    with pytest.raises(ValueError, match="lookahead and guide"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, lookahead=3, guide=table)
    with pytest.raises(ValueError, match="lookahead is not built for the sampled search.*sample=False"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, sample=True, lookahead=3)
    with pytest.raises(ValueError, match="lookahead is not built for beam search.*beam_width=1"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, beam_width=4, lookahead=3)
    with pytest.raises(ValueError, match="lookahead_record=True needs lookahead"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, lookahead_record=True)
    assert irn._lookahead is None and irn._lookahead_record is False, "the switches last for the call"
    net = InfluentialNet(cfg)
    net.shard_items(0, 2, drop_full=False)
    irn = IRSNN(cfg, net, "cpu")
    with pytest.raises(ValueError, match="lookahead is not built for an item-sharded catalog"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, lookahead=3)
