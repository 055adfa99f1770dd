"""Beam trace, the parts that need no GPU: the numpy statement (tests/beam_trace_ref.py) at W = 1 against path_trace_ref along
the greedy oracle path, its carry on hand-made permutations, pick_beam's tie rules, the binding's argument checks, the refusal
of every other search entry point while bound (through the library, on contexts without a device, as
tests/test_search_options_host.py does), and the front end's ValueErrors."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_trace_ref as ref  # noqa: E402
import path_ref  # noqa: E402
import path_trace_ref  # noqa: E402

from influentialrs_amd import _lib, synth  # noqa: E402
from influentialrs_amd.model.influentialRS import (IRSNN, InfluentialNet, SearchOptions, beam_trace_summary, pick_beam,  # noqa: E402
                                                   search_option_kwargs)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, UNSUPPORTED = -1, -2, -4
DEAD, COPY = ref.DEAD, ref.COPY
P_ = ctypes.c_void_p(4096)  # a fake non-null address: every call here is refused before anything is dereferenced or launched


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


# ---------------------------------------------------------------- the statement at W = 1
def test_one_beam_is_the_greedy_trace_along_the_oracle_path(oracle, golden):
    g = golden("irn_tiny")
    cfg = synth.make_config("tiny")
    sd = synth.irn_state_dict(cfg, 1234)
    src = [0, 2, 6, 10]
    P = int(g["meta"][2])
    L = cfg.max_len
    seqs, users = g["seqs"][src], g["users"][src]
    hep0 = np.full(len(src), L - 2, dtype=np.int32)
    arrays, paths, _, fin, links = ref.search(oracle, sd, cfg, seqs, users, hep0, 1, P, stop_rule=1)
    assert np.array_equal(paths[:, 0], g["paths"][src])  # the reference's greedy path, zero behind the arrival
    assert fin[:, 0].sum() >= 2 and (fin[:, 0] == 0).any(), "users that arrive and one that does not"
    want = [np.zeros((len(src), P), dtype=np.float32), np.zeros((len(src), P), dtype=np.float32), np.zeros((len(src), P), dtype=np.int32)]
    for i, u in enumerate(src):
        win, hep = seqs[i].copy(), L - 2
        for s in range(P):
            item = int(g["paths"][u, s])
            if item == 0:
                break
            x, _ = oracle.decode(sd, cfg, win, users[i])
            logits = oracle.score_chain(x[hep], sd["project.weight"], sd["project.bias"])
            want[0][i, s], want[1][i, s], want[2][i, s] = path_trace_ref.step_values(logits, win[:hep + 1], win[-1], item)
            win, hep = path_ref.advance(win, hep, item)
    for a, w in zip(arrays, want):
        assert a.dtype == w.dtype and np.array_equal(a[:, 0].view(np.uint32), w.view(np.uint32))
    assert (arrays[2][:, 0, 0] >= 1).all() and (arrays[0][:, 0, 0] < 0).all()
    # a user that has arrived is done from the next step on: every beam copies itself
    assert all(int(l[i, 0]) == (COPY | 0) for i in range(len(src)) if fin[i, 0] for l, _ in links[-1:])


# ---------------------------------------------------------------- the carry, by hand
def _arrays(B, W, ld, fill=True):
    base = np.arange(B * W * ld, dtype=np.float32).reshape(B, W, ld) + 1
    if not fill:
        base = np.zeros_like(base)
    return (-base, -base * 2, (base * 3).astype(np.int32))


def _cols(B, W, marks):
    return [[(np.float32(-100 - 10 * b - t), np.float32(-200 - 10 * b - t), 300 + 10 * b + t) if (b, t) in marks else None
             for t in range(W)] for b in range(B)]


def test_carry_moves_a_finished_beam_kills_a_live_slot_and_leaves_a_done_user():
    B, W, ld, step = 3, 4, 6, 3
    arrays = _arrays(B, W, ld)
    for a in arrays:
        a[:, :, step:] = 0       # nothing is recorded at or behind the step ...
        a[0, 2, 2:] = 0          # ... and user 0's beam 2 finished at step 1: columns 0, 1
    link = np.array([[1, COPY | 2, 1, DEAD],                       # user 0: the finished beam 2 moves to slot 1; slot 3, live before, dies;
                     [3, 2, 1, 0],                                 #         beam 1 has two children.  user 1: a full reversal
                     [COPY | 0, COPY | 1, COPY | 2, COPY | 3]],    # user 2: done on entry
                    dtype=np.int32)
    marks = {(0, 0), (0, 2), (1, 0), (1, 1), (1, 2), (1, 3)}
    out = ref.carry(arrays, link, _cols(B, W, marks), step)
    for c, (a, o) in enumerate(zip(arrays, out)):
        assert np.array_equal(o[2], a[2])                          # the done user: untouched
        assert np.array_equal(o[0, 1], a[0, 2]) and not o[0, 1, 2:].any()  # the finished beam, whole, in its new slot
        assert not o[0, 3].any() and a[0, 3, :step].all()          # the dead slot was live
        for t in (0, 2):                                           # both children of beam 1
            assert np.array_equal(o[0, t, :step], a[0, 1, :step]) and not o[0, t, step + 1:].any()
        assert o[0, 0, step] == _cols(B, W, marks)[0][0][c] and o[0, 2, step] == _cols(B, W, marks)[0][2][c]
        for t in range(W):                                         # in place would have read slots already overwritten
            assert np.array_equal(o[1, t, :step], a[1, W - 1 - t, :step]) and o[1, t, step] == _cols(B, W, marks)[1][t][c]
        assert o.dtype == a.dtype
    # the inputs are not modified
    assert arrays[0][0, 3, 0] != 0


def test_links_of_a_step_by_hand():
    """Two users, W = 3, window items 90.. so that every candidate survives.  User 0: beam 0 finished (score -1.0), beam 1 live
    (score -0.5) whose first candidate scores -0.5 + (2.0 - 2.0) = -0.5 and takes slot 0, the finished beam moves to slot 1, beam
    1's second candidate (-0.5 + (1.0 - 2.0) = -1.5) takes slot 2; beam 2, live with -9, leaves no child.  User 1: one live beam
    with a single candidate: slots 1 and 2 die."""
    W, L, P, k = 3, 5, 4, 3
    seq = np.full((2, W, L), 90, dtype=np.int64)
    seq[:, :, L - 1] = 7
    hep = np.full((2, W), L - 2, dtype=np.int32)
    cum = np.array([[-1.0, -0.5, -9.0], [0.0, -np.inf, -np.inf]])
    paths = np.zeros((2, W, P), dtype=np.float32)
    paths[0, 0, :1] = 7
    paths[0, 1, :1], paths[0, 2, :1] = 11, 12
    fin = np.array([[1, 0, 0], [0, 0, 0]], dtype=np.int32)
    done = np.zeros(2, dtype=np.int32)
    val = np.tile(np.array([2.0, 1.0, 0.5], dtype=np.float32), (2 * W, 1))
    ids0 = np.tile(np.array([20, 21, 22], dtype=np.int64), (2 * W, 1))
    ids0[3, 1:] = -1  # user 1's beam 0: one candidate
    lmax, lsum = np.full(2 * W, 2.0, dtype=np.float32), np.ones(2 * W, dtype=np.float32)
    logits = np.full(40, -1.0, dtype=np.float32)
    logits[20:23], logits[6] = (2.0, 1.0, 0.5), 0.0  # the target, item 7, behind the three candidates and before everything else
    arrays = _arrays(2, W, P)
    for a in arrays:
        a[:, :, 1:] = 0
    out, state, done_o, status, link, link_val = ref.traced_step(arrays, (seq, hep, cum, paths, fin), done, val, ids0, lmax, lsum,
                                                                  lambda row: logits, 1, P, stop_rule=0)
    assert link.tolist() == [[1, COPY | 0, 1], [0, DEAD, DEAD]]
    assert link_val.tolist() == [[2.0, 0.0, 1.0], [2.0, 0.0, 0.0]]
    assert state[3][0].tolist() == [[11, 21, 0, 0], [7, 0, 0, 0], [11, 22, 0, 0]] and state[4][0].tolist() == [0, 1, 0]
    lp_i, lp_t, rk = out
    lse = path_trace_ref.lse64(logits)
    assert lp_i[0, 0, 1] == np.float32(2.0 - lse) and lp_i[0, 2, 1] == np.float32(1.0 - lse) and lp_i[0, 1, 1] == 0
    assert lp_t[0, 0, 1] == np.float32(0.0 - lse) and rk[0, 0, 1] == rk[0, 2, 1] == 4  # the three candidates rank before item 7
    assert np.array_equal(lp_i[0, 1], arrays[0][0, 0]) and np.array_equal(lp_i[0, 0, :1], arrays[0][0, 1, :1])
    assert not lp_i[1, 1:].any() and not rk[1, 1:].any() and lp_i[1, 0, 1] == np.float32(2.0 - lse)
    assert done_o.tolist() == [0, 0] and not status.any()


# ---------------------------------------------------------------- pick_beam
def test_pick_beam_every_tie_rule():
    P = 4
    t = 9
    paths = np.zeros((7, 3, P), dtype=np.float32)
    scores = np.full((7, 3), -1.0)
    lp = np.full((7, 3, P), -5.0, dtype=np.float32)
    n = np.full((7, 3), P, dtype=np.int64)
    paths[:] = [[1, 2, 3, 4]] * 3
    # 0: beam 2 holds the target earliest
    paths[0, 1, 3], paths[0, 2, 1] = t, t
    # 1: two beams hold it at the same step: the higher score wins
    paths[1, 0, 2], paths[1, 2, 2] = t, t
    scores[1] = [-3.0, -1.0, -2.0]
    # 2: the same step and the same score: the lower index wins
    paths[2, 1, 0], paths[2, 2, 0] = t, t
    # 3: nobody holds it: the largest lp_target in the last recorded column (n_steps - 1), not in column P - 1
    lp[3, 1, 1], n[3, 1] = -0.5, 2
    lp[3, 2, 3] = -1.0
    # 4: nobody holds it, equal lp: the higher score, then the lower index
    scores[4] = [-2.0, -1.0, -1.0]
    # 5: the beam that would win is dead
    paths[5, 2, 0] = t
    scores[5, 2] = -np.inf
    paths[5, 1, 3] = t
    # 6: nobody is live
    scores[6] = -np.inf
    targets = np.full(7, t)
    want = [2, 2, 1, 1, 1, 1, 0]
    assert pick_beam(paths, scores, lp, n, targets, "target").tolist() == want
    assert ref.pick_beam_ref(paths, scores, lp, n, targets).tolist() == want
    assert pick_beam(paths, scores, lp, n, targets).tolist() == [0] * 7  # "score", the default
    with pytest.raises(ValueError, match="beam_pick"):
        pick_beam(paths, scores, lp, n, targets, "best")
    rng = np.random.default_rng(5)
    for _ in range(50):  # random small cases with many ties, against the slow statement
        paths = rng.integers(1, 6, (4, 4, 3)).astype(np.float32)
        scores = -rng.integers(0, 3, (4, 4)).astype(np.float64)
        scores[rng.random((4, 4)) < 0.2] = -np.inf
        lp = -rng.integers(0, 3, (4, 4, 3)).astype(np.float32)
        n = rng.integers(1, 4, (4, 4))
        targets = rng.integers(1, 8, 4)
        assert pick_beam(paths, scores, lp, n, targets, "target").tolist() == ref.pick_beam_ref(paths, scores, lp, n, targets).tolist()


def test_summary_cuts_behind_each_beams_arrival():
    paths = np.array([[[5, 9, 7, 0], [4, 6, 8, 2], [0, 0, 0, 0]]], dtype=np.float32)
    scores = np.array([[-1.0, -2.0, -np.inf]])
    a = np.arange(1, 13, dtype=np.float32).reshape(1, 3, 4)
    tr = beam_trace_summary(-a, -2 * a, (3 * a).astype(np.int32), paths, scores, np.array([9]))
    assert tr["n_steps"].tolist() == [[2, 4, 0]]
    assert tr["lp_item"][0].tolist() == [[-1, -2, 0, 0], [-5, -6, -7, -8], [0, 0, 0, 0]]
    assert tr["rank_target"][0].tolist() == [[3, 6, 0, 0], [15, 18, 21, 24], [0, 0, 0, 0]] and tr["rank_target"].dtype == np.int32
    assert sorted(tr) == ["lp_item", "lp_target", "n_steps", "paths", "rank_target", "scores"]


# ---------------------------------------------------------------- declared, exported, bound
def test_names_in_header_exports_and_ctypes_table():
    lib = _lib.load()
    txt = open(os.path.join(REPO, "include", "irs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("irs_beam_trace_scratch_bytes", 3), ("irs_bind_beam_trace", 9), ("irs_beam_step_linked", 25),
                        ("irs_beam_trace_carry", 15)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["irs_beam_trace_scratch_bytes"][0] is ctypes.c_size_t
    assert re.search(r"#define IRS_BEAM_LINK_DEAD \(-1\)", txt) and re.search(r"#define IRS_BEAM_LINK_COPY 256", txt)
    assert (_lib.IRS_BEAM_LINK_DEAD, _lib.IRS_BEAM_LINK_COPY) == (DEAD, COPY)
    for phrase in ("NOT the term the step added to the beam's score", "copied whole", "off by default", "never silently ignored",
                   "reads 0 in every column"):
        assert phrase in txt, phrase


def test_scratch_bytes_and_bind_argument_checks():
    lib, h = _ctx()
    try:
        f = lib.irs_beam_trace_scratch_bytes
        assert f(None, 4, 2) == 0
        for users, W in ((0, 2), (4, 0), (4, 33), (33, 2), (2, 32 + 1), (-1, 2)):  # max_rows = max_seqs = 64
            assert f(h, users, W) == 0, (users, W)
        # the trace sweep's rows for users * W rows, one link word and one float per beam row, each array rounded up to 256
        assert f(h, 4, 2) == lib.irs_path_trace_scratch_bytes(h, 8) + 2 * 256
        assert f(h, 2, 32) == lib.irs_path_trace_scratch_bytes(h, 64) + 2 * 256
        assert f(h, 1, 1) == 8 * 256
        ws = lib.irs_workspace_bytes(h)
        b = lib.irs_bind_beam_trace
        need = f(h, 4, 2)
        assert b(h, P_, P_, None, 4, 2, 8, P_, need) == INVALID and b"go together" in lib.irs_last_error(h)
        assert b(h, P_, P_, P_, 4, 0, 8, P_, need) == INVALID and b"beam width" in lib.irs_last_error(h)
        assert b(h, P_, P_, P_, 4, 33, 8, P_, need) == INVALID
        assert b(h, P_, P_, P_, 0, 2, 8, P_, need) == INVALID
        assert b(h, P_, P_, P_, 33, 2, 8, P_, 1 << 20) == INVALID and b"max_seqs=64 / max_rows=64" in lib.irs_last_error(h)
        assert b(h, P_, P_, P_, 4, 2, 0, P_, need) == INVALID and b(h, P_, P_, P_, 4, 2, 65, P_, need) == INVALID
        assert b"ld must be in [1, 64]" in lib.irs_last_error(h)
        assert b(h, P_, P_, P_, 4, 2, 8, P_, need - 1) == INVALID and b"too small" in lib.irs_last_error(h)
        assert b(h, P_, P_, P_, 4, 2, 8, None, need) == INVALID
        assert b(h, P_, P_, P_, 4, 2, 8, ctypes.c_void_p(4096 + 8), need) == INVALID and b"aligned" in lib.irs_last_error(h)
        assert b(h, P_, P_, P_, 4, 2, 64, P_, need) == 0
        assert b(h, None, None, None, 0, 0, 0, None, 0) == 0 and b(h, None, None, None, 0, 0, 0, None, 0) == 0  # unbind, twice
        assert lib.irs_workspace_bytes(h) == ws
        # the two kernels alone: refused before the launch
        c = lib.irs_beam_trace_carry
        assert c(h, P_, P_, P_, P_, P_, None, 2, 2, 0, P_, P_, P_, 8, None) == INVALID
        for B, W, step, ld in ((0, 2, 0, 8), (2, 0, 0, 8), (2, 33, 0, 8), (2, 2, 8, 8), (2, 2, -1, 8), (2, 2, 0, 65), (2, 2, 0, 0)):
            assert c(h, P_, P_, P_, P_, P_, P_, B, W, step, P_, P_, P_, ld, None) == INVALID, (B, W, step, ld)
        s = lib.irs_beam_step_linked
        ok = dict(fin_in=None, fin_out=None, done=None, link=P_, W=33)

        def step_rc(**kw):
            a = dict(ok, **kw)
            return s(h, P_, P_, P_, P_, a["fin_in"], P_, P_, P_, P_, 2, a["W"], 10, 0, 3, a.get("rule", 0), P_, P_, P_, P_, a["fin_out"],
                     a["done"], P_, a["link"], P_)
        assert step_rc(link=None) == INVALID
        assert step_rc(fin_in=P_) == INVALID and b"go together" in lib.irs_last_error(h)
        assert step_rc(fin_in=P_, fin_out=P_, done=P_, rule=2) == INVALID and b"stop_rule" in lib.irs_last_error(h)
        # admitted: both forms end at the launcher's own width check (W = 33), as irs_beam_step does
        assert step_rc() == UNSUPPORTED and b"beam width 33" in lib.irs_last_error(h)
        assert step_rc(fin_in=P_, fin_out=P_, done=P_) == UNSUPPORTED and b"beam width 33" in lib.irs_last_error(h)
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        assert lib.irs_bind_beam_trace(h, P_, P_, P_, 4, 2, 8, P_, 1 << 20) == UNSUPPORTED
        assert b"irs_bind_beam_trace needs the whole catalog on one device" in lib.irs_last_error(h)
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- every other entry point refuses while bound
def _calls(lib, h):
    c = {}
    c["irs_generate_paths"] = lambda: lib.irs_generate_paths(h, P_, P_, P_, 4, 3, 10, 0, 0, 3, 0, 0, P_, P_, None)
    c["irs_generate_paths_until"] = lambda: lib.irs_generate_paths_until(h, P_, P_, P_, 4, 3, 10, 0, 0, 3, 0, 1, P_, P_, None, None)
    c["irs_path_step"] = lambda: lib.irs_path_step(h, P_, P_, 4, P_, P_, 4, 0, P_, 3, 0, 0, 0, P_, None)
    c["irs_beam_step"] = lambda: lib.irs_beam_step(h, P_, P_, P_, P_, P_, P_, P_, P_, 2, 33, 10, 0, 3, P_, P_, P_, P_, P_, None)
    c["irs_beam_step_until"] = lambda: lib.irs_beam_step_until(h, P_, P_, P_, P_, P_, P_, P_, P_, P_, 2, 33, 10, 0, 3, 0, P_, P_, P_, P_,
                                                               P_, P_, P_, None)
    c["irs_beam_search"] = lambda: lib.irs_beam_search(h, P_, P_, P_, 2, 2, 3, 10, 0, 0, P_, P_, None, P_, None)
    c["irs_beam_search_until"] = lambda: lib.irs_beam_search_until(h, P_, P_, P_, 2, 2, 3, 10, 0, 0, 1, P_, P_, P_, None, P_, None, None)
    return c


def test_every_other_entry_point_refuses_while_bound_and_works_again_after():
    lib, h = _ctx()
    try:
        assert lib.irs_bind_beam_trace(h, P_, P_, P_, 4, 2, 8, P_, lib.irs_beam_trace_scratch_bytes(h, 4, 2)) == 0
        for name, thunk in _calls(lib, h).items():
            rc, msg = thunk(), lib.irs_last_error(h).decode()
            if name in ("irs_beam_search", "irs_beam_search_until"):  # admitted: on a context without weights they end at readiness
                assert (rc, msg) == (STATE, "weights not finalized (irs_finalize_weights)"), name
            else:
                fn = name.split()[0]
                assert (rc, msg) == (UNSUPPORTED, f"{fn}: a beam trace is bound (irs_bind_beam_trace): irs_beam_search and "
                                                  "irs_beam_search_until only"), (name, rc, msg)
        # a bound path trace beside it: the beam trace's refusal comes first at the greedy loops, and the beam loops still admit
        assert lib.irs_bind_path_trace(h, P_, P_, P_, 8, 4, P_, lib.irs_path_trace_scratch_bytes(h, 8)) == 0
        assert _calls(lib, h)["irs_generate_paths"]() == UNSUPPORTED and b"irs_bind_beam_trace" in lib.irs_last_error(h)
        assert lib.irs_bind_path_trace(h, None, None, None, 0, 0, None, 0) == 0
        assert lib.irs_bind_beam_trace(h, None, None, None, 0, 0, 0, None, 0) == 0
        after = {n: (t(), lib.irs_last_error(h).decode()) for n, t in _calls(lib, h).items() if n != "irs_path_step"}
        for name, (rc, msg) in after.items():  # what test_search_options_host.py records for a context with nothing bound
            if "beam_step" in name:
                assert (rc, msg) == (UNSUPPORTED, "beam width 33 outside [1, 32]"), name
            else:
                assert (rc, msg) == (STATE, "weights not finalized (irs_finalize_weights)"), name
    finally:
        lib.irs_destroy(h)


def test_the_sharded_loops_cannot_meet_a_binding():
    """A context with world != 1 refuses the binding itself, so the sharded loops' refusal can never be needed; it exists
    (capi.hip: OPTS) so that the binding could not be ignored if that ever changed."""
    lib, h = _ctx(world=2)
    try:
        assert lib.irs_bind_beam_trace(h, P_, P_, P_, 2, 2, 4, P_, 1 << 20) == UNSUPPORTED
    finally:
        lib.irs_destroy(h)
    src = open(os.path.join(REPO, "influentialrs_amd", "csrc", "capi.hip")).read()
    assert "a bound beam trace (irs_bind_beam_trace) needs the whole catalog on one device" in src
    row = re.search(r"/\* AT_SHARDED_LOOP \*/ \{([^}]*)\}", src).group(1)
    assert "OPT_BTRACE" in row


# ---------------------------------------------------------------- Python layers
def test_keywords_are_off_by_default_and_the_front_end_refuses_without_a_device():
    from influentialrs_amd.engine import Engine
    for fn in (Engine.beam_search, Engine.beam_search_until):
        assert inspect.signature(fn).parameters["trace"].default is False, fn
    for name in ("bind_beam_trace", "unbind_beam_trace", "beam_step_linked", "beam_trace_carry", "beam_trace_scratch_bytes"):
        assert hasattr(Engine, name), name
    sig = inspect.signature(IRSNN.get_seq_in_batch, follow_wrapped=False).parameters
    assert sig["beam_trace"].default is False and sig["beam_trace"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["beam_pick"].default == "score" and sig["beam_pick"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(IRSNN.get_seq_in_batch).parameters)[-1] == "beam_stop"
    import dataclasses
    assert [f.name for f in dataclasses.fields(SearchOptions)][-2:] == ["beam_trace", "beam_pick"]
    assert SearchOptions().beam_trace is False and SearchOptions().beam_pick == "score"
    with pytest.raises(ValueError, match=r"beam_trace needs beam_width > 1: use trace=True"):
        search_option_kwargs(SearchOptions(beam_trace=True), 1, False, 1)
    with pytest.raises(ValueError, match="beam_trace is not built for an item-sharded catalog"):
        search_option_kwargs(SearchOptions(beam_trace=True), 4, False, 2)
    with pytest.raises(ValueError, match="beam_pick='best'"):
        search_option_kwargs(SearchOptions(beam_trace=True, beam_pick="best"), 4, False, 1)
    with pytest.raises(ValueError, match="use beam_trace=True"):
        search_option_kwargs(SearchOptions(beam_pick="target"), 4, False, 1)
    assert search_option_kwargs(SearchOptions(beam_trace=True, beam_pick="target"), 4, False, 1) == dict(exact_candidates=False, trace=False)
    cfg = synth.make_config("tiny")
    net = InfluentialNet(cfg)
    irn = IRSNN(cfg, net, "cpu")
    B, L = 2, cfg.max_len
    seqs, users, targets = torch.ones((B, L), dtype=torch.int64), torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.int64)
    with pytest.raises(ValueError, match="beam_trace needs beam_width > 1"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, beam_trace=True)
    with pytest.raises(ValueError, match="trace is not built for beam search"):  # as before this keyword existed
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, beam_width=2, trace=True)
    with pytest.raises(ValueError, match="trace is not built for beam search"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, beam_width=2, trace=True, beam_trace=True)
    net.shard_items(0, 2, drop_full=False)
    with pytest.raises(ValueError, match="beam_trace is not built for an item-sharded catalog"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, beam_width=2, beam_trace=True)
    assert irn._beam_trace is False and irn._beam_pick == "score", "the switches last for the call"
