"""Path trace, the parts that need no GPU: the numpy statement (tests/path_trace_ref.py) against float64 log_softmax and a
brute-force rank, the front end's cut and derived figures on hand-made arrays, the scratch size and the binding's argument
checks (refused before any launch), and the new symbols in header, library and ctypes table."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import path_trace_ref as ref  # noqa: E402

from influentialrs_amd import _lib  # noqa: E402
from influentialrs_amd.model.influentialRS import path_trace_summary  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, UNSUPPORTED = -1, -2, -4


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


# ---------------------------------------------------------------- the statement
def _brute_rank(logits, window, target):
    """Sort everything the window leaves (the target stays, wherever it is) by (score descending, id ascending)."""
    hidden = set(int(v) for v in window if v != 0) - {int(target)}
    rows = sorted((-(float(logits[j]) + 0.0), j) for j in range(len(logits)) if j + 1 not in hidden)
    return 1 + [j for _, j in rows].index(int(target) - 1)


def _cases():
    rng = np.random.default_rng(20)
    out = []
    for n, wl in ((7, 3), (40, 12), (129, 30), (300, 64)):
        for _ in range(6):
            logits = rng.normal(0, 3, n).astype(np.float32)
            t = int(rng.integers(1, n + 1))
            win = rng.integers(1, n + 1, wl).astype(np.int64)
            win[:int(rng.integers(0, wl // 2 + 1))] = 0  # leading pads
            win[-1] = win[wl // 2]  # a duplicate
            out.append((logits, win, t))
    # the target inside its own window
    logits = rng.normal(0, 1, 50).astype(np.float32)
    out.append((logits, np.array([0, 0, 9, 17, 9, 3], dtype=np.int64), 17))
    # exact ties on both sides of the target's id, one tied item in the window; -0 ties +0
    logits = rng.normal(0, 1, 50).astype(np.float32)
    logits[[4, 11, 20, 33, 41]] = np.float32(0.75)  # ids0 4, 11 < target 20 < 33, 41
    out.append((logits, np.array([0, 12, 5, 5, 34], dtype=np.int64), 21))  # items 12 (id0 11) and 34 (id0 33) hidden
    logits = rng.normal(0, 1, 30).astype(np.float32)
    logits[[2, 9, 15]] = np.float32(0.0)
    logits[[6, 20]] = np.float32(-0.0)
    out.append((logits, np.array([3, 0, 0], dtype=np.int64), 10))
    return out


def test_statement_against_float64_log_softmax_and_brute_force_rank():
    seen_tie = False
    for logits, win, t in _cases():
        lsm = torch.log_softmax(torch.from_numpy(logits).double(), dim=0).numpy()
        chosen = int(np.argmax(logits)) + 1
        lp_c, lp_t, rank = ref.step_values(logits, win, t, chosen)
        assert lp_c.dtype == np.float32 and lp_t.dtype == np.float32
        # float64 log_softmax rounded once: at most one float32 ulp from another float64 summation order
        assert abs(float(lp_t) - lsm[t - 1]) <= 2 * np.spacing(np.float32(abs(lsm[t - 1]))) + 1e-12
        assert abs(float(lp_c) - lsm[chosen - 1]) <= 2 * np.spacing(np.float32(abs(lsm[chosen - 1]))) + 1e-12
        assert rank == _brute_rank(logits, win, t), (win, t)
        seen_tie |= int((logits == logits[t - 1]).sum()) > 1
    assert seen_tie


def test_statement_edge_cases():
    logits = np.array([1.0, 3.0, 3.0, -2.0, 3.0], dtype=np.float32)
    # ties by id: before item 3 (id0 2) rank id0 1 only; item 2 hidden -> nobody
    assert ref.target_rank(logits, [], 3) == 2
    assert ref.target_rank(logits, [0, 2, 2], 3) == 1
    assert ref.target_rank(logits, [5], 3) == 2  # a hidden item behind the target changes nothing
    assert ref.target_rank(logits, [3, 3], 3) == 2  # the target in its own window keeps its rank
    assert ref.target_rank(logits, [0, 0], 4) == 5
    # no target: zeros; no choice: lp_item 0
    assert ref.step_values(logits, [1], 0, 2)[1:] == (np.float32(0), 0)
    assert ref.step_values(logits, [1], 3, 0)[0] == np.float32(0)
    lp = ref.trace_rows(logits[None], np.array([[0, 2, 0, 3]]), np.array([1]), np.array([5]))
    assert lp[2][0] == 1 and lp[0][0] == lp[1][0] == np.float32(3.0 - ref.lse64(logits))


# ---------------------------------------------------------------- the front end's cut and derived figures
def test_summary_cut_and_derived_figures():
    paths = np.array([[5, 9, 7, 0], [4, 6, 8, 2], [3, 1, 1, 1]], dtype=np.float32)
    targets = np.array([7, 11, 3])
    lp_item = -np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    lp_target = np.array([[-8, -6, -5, -4], [-9, -9.5, -7, -2], [-1, -3, -3, -3]], dtype=np.float32)
    rank = np.array([[40, 12, 3, 2], [90, 95, 30, 4], [1, 6, 6, 6]], dtype=np.int32)
    tr = path_trace_summary(lp_item, lp_target, rank, paths, targets)
    assert tr["n_steps"].tolist() == [3, 4, 1]
    assert np.array_equal(tr["lp_item"], np.array([[-1, -2, -3, 0], [-5, -6, -7, -8], [-9, 0, 0, 0]], dtype=np.float32))
    assert np.array_equal(tr["lp_target"], np.array([[-8, -6, -5, 0], [-9, -9.5, -7, -2], [-1, 0, 0, 0]], dtype=np.float32))
    assert np.array_equal(tr["rank_target"], np.array([[40, 12, 3, 0], [90, 95, 30, 4], [1, 0, 0, 0]], dtype=np.int32))
    assert tr["rank_target"].dtype == np.int32 and tr["lp_item"].dtype == np.float32
    assert tr["ioi"].tolist() == [3.0, 7.0, 0.0]
    assert tr["ior"].tolist() == [37, 86, 0]
    assert np.allclose(tr["avg_lp_item"], [-2.0, -6.5, -9.0])
    # the inputs are not modified, and a second pass over the cut arrays changes nothing
    assert lp_item[0, 3] == -4 and rank[2, 1] == 6
    again = path_trace_summary(tr["lp_item"], tr["lp_target"], tr["rank_target"], paths, targets)
    assert all(np.array_equal(again[k], tr[k]) for k in tr)


# ---------------------------------------------------------------- declared, exported, bound
def test_names_in_header_exports_and_ctypes_table():
    lib = _lib.load()
    txt = open(os.path.join(REPO, "include", "irs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("irs_path_trace_scratch_bytes", 2), ("irs_score_target_trace", 12), ("irs_bind_path_trace", 8)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["irs_path_trace_scratch_bytes"][0] is ctypes.c_size_t
    # the semantics are stated where the CPU statement was written from
    for phrase in ("rank_target", "lp_target", "lp_item", "Duplicates in the window count once", "no_repeat do NOT enter the rank"):
        assert phrase in txt, phrase


# ---------------------------------------------------------------- the scratch size and the binding's checks, without a device
def test_scratch_bytes_invalid_arguments():
    lib, h = _ctx()
    try:
        f = lib.irs_path_trace_scratch_bytes
        assert f(None, 4) == 0
        for rows in (0, -1, 65):  # max_rows = 64
            assert f(h, rows) == 0, rows
        assert f(h, 1) == 6 * 256 and f(h, 64) == 2 * 512 + 4 * 256 and f(h, 33) == 2 * 512 + 4 * 256
    finally:
        lib.irs_destroy(h)


def test_bind_argument_checks_and_workspace_unchanged():
    lib, h = _ctx()
    p = ctypes.c_void_p
    try:
        ws = lib.irs_workspace_bytes(h)
        f = lib.irs_bind_path_trace
        need = lib.irs_path_trace_scratch_bytes(h, 8)
        assert f(h, p(4096), p(4096), None, 8, 4, p(4096), need) == INVALID  # the three arrays go together
        assert f(h, p(4096), p(4096), p(4096), 0, 4, p(4096), need) == INVALID
        assert f(h, p(4096), p(4096), p(4096), 65, 4, p(4096), 1 << 20) == INVALID
        assert f(h, p(4096), p(4096), p(4096), 8, 0, p(4096), need) == INVALID
        assert f(h, p(4096), p(4096), p(4096), 8, 4, p(4096), need - 1) == INVALID and b"too small" in lib.irs_last_error(h)
        assert f(h, p(4096), p(4096), p(4096), 8, 4, None, need) == INVALID
        assert f(h, p(4096), p(4096), p(4096), 8, 4, p(4096 + 8), need) == INVALID and b"aligned" in lib.irs_last_error(h)
        assert f(h, p(4096), p(4096), p(4096), 8, 4, p(4096), need) == 0
        # while bound the beam steps refuse, before they look at anything else they would launch with
        q = p(4096)
        assert lib.irs_beam_step(h, q, q, q, q, q, q, q, q, 2, 2, 10, 0, 4, q, q, q, q, q, None) == UNSUPPORTED
        assert b"irs_bind_path_trace" in lib.irs_last_error(h)
        assert lib.irs_beam_step_until(h, q, q, q, q, q, q, q, q, q, 2, 2, 10, 0, 4, 0, q, q, q, q, q, q, q, None) == UNSUPPORTED
        assert f(h, None, None, None, 0, 0, None, 0) == 0  # unbind
        assert f(h, None, None, None, 0, 0, None, 0) == 0  # and again: nothing bound is fine
        assert lib.irs_workspace_bytes(h) == ws
        # the standalone sweep's checks (this context has no weights: a complete call ends at IRS_E_STATE)
        g = lib.irs_score_target_trace
        assert g(h, q, q, q, 8, q, need, q, q, q, q, None) == STATE
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        need = lib.irs_path_trace_scratch_bytes(h, 8)
        assert lib.irs_bind_path_trace(h, p(4096), p(4096), p(4096), 8, 4, p(4096), need) == UNSUPPORTED
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- Python layers
def test_keyword_is_off_by_default_and_the_front_end_refuses_without_a_device():
    import inspect

    from influentialrs_amd import synth
    from influentialrs_amd.engine import Engine
    from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
    for fn in (Engine.generate_paths, Engine.generate_paths_until):
        assert inspect.signature(fn).parameters["trace"].default is False, fn
    assert hasattr(Engine, "score_target_trace") and hasattr(Engine, "bind_path_trace")
    sig = inspect.signature(IRSNN.get_seq_in_batch, follow_wrapped=False).parameters
    assert sig["trace"].default is False and sig["trace"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(IRSNN.get_seq_in_batch).parameters)[-1] == "beam_stop"
    cfg = synth.make_config("tiny")
    net = InfluentialNet(cfg)
    irn = IRSNN(cfg, net, "cpu")
    B, L = 2, cfg.max_len
    seqs, users, targets = torch.ones((B, L), dtype=torch.int64), torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.int64)
    with pytest.raises(ValueError, match="trace is not built for beam search"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, beam_width=2, trace=True)
    net.shard_items(0, 2, drop_full=False)
    with pytest.raises(ValueError, match="trace is not built for an item-sharded catalog"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, trace=True)
    assert irn._trace is False, "the switch lasts for the call"
