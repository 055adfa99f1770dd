"""Path replay, the parts that need no GPU: the new symbols in header, library and ctypes table, the scratch size and every
refusal of the two entry points (all before any launch, on a context created without a device), the numpy statement
(tests/replay_ref.py) against path_ref's step rule and against the windows the oracle's evaluator walks, the fact that irr / ir
rest on (the two rank rows of eval_get_rr_increase are replay steps 0 and l_path - 1), and the front end's refusals."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import path_ref  # noqa: E402
import replay_ref as ref  # noqa: E402

from influentialrs_amd import _lib, build, harness, synth  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, UNSUPPORTED = -1, -2, -4
SLOT, FULL = _lib.IRS_REPLAY_SLOT, _lib.IRS_REPLAY_FULL


def _ctx(world=1, causal=False, **kw):
    lib = _lib.load()
    h = ctypes.c_void_p()
    base = dict(n_item=1000, n_user=10, d=30, max_len=60, n_heads=6, ffn_dim=256, n_layers=2, u_dim=10, mask_mode=0,
                max_rows=64, max_k=100, max_seqs=0)
    if causal:
        base.update(n_user=0, u_dim=0, mask_mode=1)
    base.update(kw)
    dims = _lib.IrsDims(**base)
    shard = _lib.IrsShard(0, world, 0, base["n_item"] // world) if world > 1 else None
    assert lib.irs_create(ctypes.byref(h), ctypes.byref(dims), ctypes.byref(shard) if shard else None) == 0
    return lib, h


# ---------------------------------------------------------------- declared, exported, bound, built
def test_names_in_header_exports_ctypes_table_and_sources():
    lib = _lib.load()
    txt = open(os.path.join(REPO, "include", "irs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("irs_replay_scratch_bytes", 2), ("irs_replay_windows", 17), ("irs_replay_paths", 21)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["irs_replay_scratch_bytes"][0] is ctypes.c_size_t
    assert re.search(r"#define\s+IRS_REPLAY_SLOT\s+0\b", code) and re.search(r"#define\s+IRS_REPLAY_FULL\s+1\b", code)
    assert (SLOT, FULL) == (0, 1) == (ref.SLOT, ref.FULL)
    assert "replay.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "replay.hip"))
    for phrase in ("REPLAY ROW", "IRS_REPLAY_SLOT", "IRS_REPLAY_FULL", "A row is INVALID", "replay chooses nothing"):
        assert phrase in txt, phrase


def test_scratch_bytes():
    lib, h = _ctx(max_rows=64, max_seqs=48)
    try:
        f = lib.irs_replay_scratch_bytes
        assert f(None, 4) == 0
        for chunk in (0, -1, 49, 64):  # min(max_rows, max_seqs) = 48
            assert f(h, chunk) == 0, chunk
        up = lambda v: (v + 255) // 256 * 256  # noqa: E731
        for chunk in (1, 33, 48):  # windows, three int64 rows, hep and item scores, x rows, the trace rows
            want = up(chunk * 60 * 8) + 3 * up(chunk * 8) + 2 * up(chunk * 4) + up(chunk * 30 * 4)
            assert f(h, chunk) == want + lib.irs_path_trace_scratch_bytes(h, chunk), chunk
        ws = lib.irs_workspace_bytes(h)
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(max_rows=64, max_seqs=48)
    try:
        assert lib.irs_workspace_bytes(h) == ws
    finally:
        lib.irs_destroy(h)


def test_every_refusal_before_any_launch():
    p = ctypes.c_void_p
    q = p(4096)
    lib, h = _ctx()  # an IRN context without weights: a complete call ends at IRS_E_STATE
    try:
        need = lib.irs_replay_scratch_bytes(h, 16)

        def win(layout=SLOT, seq0=q, hep0=q, user=q, B=4, paths=q, P=5, ld=5, ru=q, rs=q, R=8, so=q, ho=q, uo=q, st=q):
            return lib.irs_replay_windows(h, layout, seq0, hep0, user, B, paths, P, ld, ru, rs, R, so, ho, uo, st, None)

        def rep(layout=SLOT, seq0=q, hep0=q, user=q, target=None, B=4, paths=q, P=5, ld=5, ru=q, rs=q, R=8, chunk=16, sc=q,
                nb=need, li=q, lt=q, rk=q, st=q):
            return lib.irs_replay_paths(h, layout, seq0, hep0, user, target, B, paths, P, ld, ru, rs, R, chunk, sc, nb, li, lt, rk,
                                        st, None)

        bad_shapes = (dict(seq0=None), dict(paths=None), dict(ru=None), dict(rs=None), dict(st=None), dict(R=0), dict(R=-3),
                      dict(R=(1 << 24) + 1), dict(B=0), dict(P=-1), dict(P=6, ld=5), dict(layout=2), dict(layout=-1),
                      dict(layout=SLOT, hep0=None))
        for kw in bad_shapes:
            assert win(**kw) == INVALID, kw
            assert rep(**kw) == INVALID, kw
        assert win(so=None) == INVALID and win(ho=None) == INVALID
        for kw in (dict(li=None), dict(lt=None), dict(rk=None), dict(sc=None), dict(chunk=0), dict(chunk=65), dict(nb=need - 1),
                   dict(sc=p(4096 + 8)), dict(layout=SLOT, target=q), dict(layout=FULL, target=None), dict(user=None)):
            assert rep(**kw) == INVALID, kw
        assert rep(nb=need - 1) == INVALID and b"too small" in lib.irs_last_error(h)
        assert rep(sc=p(4096 + 8)) == INVALID and b"aligned" in lib.irs_last_error(h)
        assert rep(layout=FULL, target=q) == UNSUPPORTED and b"IRS_MASK_IRN" in lib.irs_last_error(h)
        assert rep() == STATE
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(causal=True)  # the evaluator's context: both layouts pass the checks, user may be NULL
    try:
        need = lib.irs_replay_scratch_bytes(h, 16)
        args = (4, q, 5, 5, q, q, 8, 16, q, need, q, q, q, q, None)
        assert lib.irs_replay_paths(h, FULL, q, None, None, q, *args) == STATE
        assert lib.irs_replay_paths(h, SLOT, q, q, None, None, *args) == STATE
        assert lib.irs_replay_paths(h, FULL, q, None, None, None, *args) == INVALID
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        need = lib.irs_replay_scratch_bytes(h, 16)
        assert lib.irs_replay_paths(h, SLOT, q, q, q, None, 4, q, 5, 5, q, q, 8, 16, q, need, q, q, q, q, None) == UNSUPPORTED
        assert b"whole catalog" in lib.irs_last_error(h)
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- the statement: the slot layout is path_ref's step rule
@pytest.mark.parametrize("L", [2, 3, 12, 64])
def test_slot_layout_is_i_applications_of_the_step_rule(L):
    rng = np.random.default_rng(L)
    P = 2 * L + 1
    for h0 in sorted({0, (L - 2) // 2, L - 2}):
        seq0 = np.zeros(L, dtype=np.int64)
        seq0[:h0 + 1] = rng.integers(1, 50, h0 + 1)
        seq0[0] = 0 if h0 > 0 else seq0[0]  # a leading pad
        seq0[L - 1] = 77
        path = rng.integers(1, 50, P).astype(np.int64)
        win, he = seq0.copy(), h0
        for i in range(P + 1):
            got, ghe = ref.replay_window(seq0, h0, path, i, ref.SLOT)
            assert np.array_equal(got, win) and ghe == he, (L, h0, i)
            if i < P:
                win, he = path_ref.advance(win, he, int(path[i]))
        assert he == L - 2 and (L < 3 or np.array_equal(win[:L - 1], path[P - (L - 1):]))  # the start window is shifted out


def test_validity_and_fallback_windows():
    seq0 = np.array([[3, 4, 0, 0], [0, 0, 0, 0]], dtype=np.int64)
    paths = np.array([[5, 0, 6], [7, 8, 9]], dtype=np.int64)
    ok = lambda b, i, lay=ref.FULL, hep0=None: ref.row_valid(seq0, hep0, paths, 3, 9, b, i, lay)  # noqa: E731
    assert ok(0, 0) and ok(0, 1) and not ok(0, 2) and not ok(0, 3)  # path[0][1] == 0 is no item to force
    assert not ok(1, 0) and ok(1, 1) and ok(1, 3) and not ok(1, 4) and not ok(2, 0) and not ok(-1, 0) and not ok(0, -1)
    assert not ref.row_valid(seq0, None, paths, 3, 8, 1, 3, ref.FULL)  # 9 outside the catalog
    assert ok(0, 1, ref.SLOT, [2, 0]) and not ok(0, 1, ref.SLOT, [3, 0]) and not ok(0, 1, ref.SLOT, [-1, 0])
    w, he = ref.fallback_window(seq0, None, 1, ref.FULL)
    assert w.tolist() == [1, 0, 0, 0] and he == 0
    w, he = ref.fallback_window(seq0, None, 7, ref.FULL)
    assert w.tolist() == [3, 4, 0, 0] and he == 1
    w, he = ref.fallback_window(seq0, [5, 0], 0, ref.SLOT)
    assert w.tolist() == [3, 4, 0, 0] and he == 2
    seq, hep, st = ref.replay_windows(seq0, None, paths, 3, 9, [0, 1, 1, 5], [1, 0, 3, 0], ref.FULL)
    assert st.tolist() == [0, 2, 0, 2] and hep.tolist() == [2, 0, 2, 1]
    assert seq.tolist() == [[3, 4, 5, 0], [1, 0, 0, 0], [7, 8, 9, 0], [3, 4, 0, 0]]


# ---------------------------------------------------------------- the statement: the full layout is the oracle's evaluator
class _Spy:
    """Stands in for the oracle's decoder and scorer while one of its evaluator functions runs: records every window the
    function decodes and which row of the result it consumes (row p of the fake x holds p), and scores with zeros."""

    def __init__(self, oracle, monkeypatch, n_item):
        self.windows, self.rows, self.hists = [], [], []
        monkeypatch.setattr(oracle, "decode", self._decode)
        monkeypatch.setattr(oracle, "score_chain", self._score)
        monkeypatch.setattr(oracle, "rank_of", self._rank)
        self.n_item = n_item

    def _decode(self, sd, cfg, seq, user, evaluator=False, dtype=np.float32):
        self.windows.append(np.array(seq, dtype=np.int64))
        return np.arange(len(seq), dtype=np.float32)[:, None], None

    def _score(self, x_row, W, b):
        self.rows.append(int(x_row[0]))
        return np.zeros(self.n_item, dtype=np.float32)

    def _rank(self, scores, label0, hist0):
        self.hists.append(np.array(hist0, dtype=np.int64) + 1)
        return 1


def _eval_inputs(g):
    return tuple(g[k] for k in ("histories", "new_seqs", "targets", "start_pos", "l_paths"))


def _paths_of(d, sp, lp):
    P = int(lp.max())
    paths = np.zeros((len(lp), P), dtype=np.int64)
    for b in range(len(lp)):
        paths[b, :lp[b]] = d[b, sp[b]:sp[b] + lp[b]]
    return paths


@pytest.mark.parametrize("name,cfgname", [("eval_tiny", "eval_tiny"), ("eval_default", "eval_default")])
def test_full_layout_is_the_window_walk_of_eval_get_grad(golden, oracle, monkeypatch, name, cfgname):
    g = golden(name)
    cfg = synth.make_config(cfgname)
    h, d, t, sp, lp = _eval_inputs(g)
    spy = _Spy(oracle, monkeypatch, cfg.n_item)
    sd = {"project.weight": None, "project.bias": None}
    oracle.eval_get_grad(sd, cfg, h, d, t, sp, lp)
    B, S = len(lp), int(lp.max())
    order = [(b, i) for i in range(S) for b in range(B) if i < lp[b]]  # the oracle's loop order
    assert len(spy.windows) == len(order) == int(lp.sum()) and len(spy.rows) == len(order)
    paths = _paths_of(d, sp, lp)
    seq0 = h[:, :-1]
    shifted = 0
    for (b, i), win, row in zip(order, spy.windows, spy.rows):
        assert ref.row_valid(seq0, None, paths, S, cfg.n_item, b, i, ref.FULL)
        got, hep = ref.replay_window(seq0[b], None, paths[b], i, ref.FULL)
        assert np.array_equal(got, win) and hep == row, (b, i)
        shifted += ref.first_zero(seq0[b]) + i > seq0.shape[1]
    assert shifted > 0  # both goldens hold full windows: rows that shift
    # the forced item of a row is the item the oracle scores there
    for b in range(B):
        assert (paths[b, :lp[b]] > 0).all() and not paths[b, lp[b]:].any()


@pytest.mark.parametrize("name,cfgname,users", [("eval_tiny", "eval_tiny", 8), ("eval_default", "eval_default", 6)])
def test_rank_rows_of_eval_get_rr_increase_are_replay_steps_0_and_last(golden, oracle, monkeypatch, name, cfgname, users):
    g = golden(name)
    cfg = synth.make_config(cfgname)
    h, d, t, sp, lp = _eval_inputs(g)
    B = len(lp)
    assert B == users
    spy = _Spy(oracle, monkeypatch, cfg.n_item)
    oracle.eval_get_rr_increase({"project.weight": None, "project.bias": None}, cfg, h, d, t)
    assert len(spy.windows) == len(spy.rows) == len(spy.hists) == 2 * B
    paths = _paths_of(d, sp, lp)
    for b in range(B):
        for k, i in enumerate((0, int(lp[b]) - 1)):  # the oracle decodes a user's begin row, then its end row
            win, row, hist = spy.windows[2 * b + k], spy.rows[2 * b + k], spy.hists[2 * b + k]
            got, hep = ref.replay_window(h[b, :-1], None, paths[b], i, ref.FULL)
            # the consumed row, the ids up to it (all a causal decoder sees) and the filter list of the rank are the replay's
            assert hep == row, (b, i, hep, row)
            assert np.array_equal(got[:hep + 1], win[:row + 1]) and np.array_equal(hist, got[:hep + 1]), (b, i)
            assert (got[:hep + 1] > 0).all()


# ---------------------------------------------------------------- Python layers
def test_front_end_is_off_by_default_and_refuses_without_a_device():
    from influentialrs_amd.engine import Engine
    from influentialrs_amd.model.evaluator import Evaluator
    from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
    from influentialrs_amd.model.uRS import SampleNet
    assert inspect.signature(harness.evaluate_prob).parameters["replay"].default is False
    for name in ("replay_scratch_bytes", "replay_windows", "replay_paths"):
        assert hasattr(Engine, name), name
    assert list(inspect.signature(Evaluator.get_path_metrics_in_batch).parameters) == [
        "self", "histories", "new_seqs", "targets", "start_pos", "l_paths"]
    assert list(inspect.signature(IRSNN.replay_paths).parameters) == ["self", "seqs", "users", "paths", "gap_len"]
    ecfg = synth.make_config("eval_tiny")
    snet = SampleNet(ecfg)
    ev = Evaluator(ecfg, snet, "cpu")
    L = ecfg.max_len
    h = torch.ones((2, L + 1), dtype=torch.int64)
    one = torch.ones(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="HIP engine only"):
        ev.get_path_metrics_in_batch(h, h, one, one, one)
    snet.shard_items(0, 2, drop_full=False)
    with pytest.raises(ValueError, match="not built for an item-sharded catalog"):
        ev.get_path_metrics_in_batch(h, h, one, one, one)
    cfg = synth.make_config("tiny")
    net = InfluentialNet(cfg)
    irn = IRSNN(cfg, net, "cpu")
    seqs = torch.ones((2, cfg.max_len), dtype=torch.int64)
    with pytest.raises(ValueError, match="HIP engine only"):
        irn.replay_paths(seqs, one, np.ones((2, 3), dtype=np.float32))
    net.shard_items(0, 2, drop_full=False)
    with pytest.raises(ValueError, match="not built for an item-sharded catalog"):
        irn.replay_paths(seqs, one, np.ones((2, 3), dtype=np.float32))
