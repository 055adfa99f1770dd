"""not-gpu: exact candidates when the window hides the top-k (irs_topk_ensure_survivors, irs_bind_survivor_scratch): the
restatement the GPU tests compare against, on hand-made rows; the scratch size; and every argument check of the new entry
points through the ABI on a context created without a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from influentialrs_amd import _lib, synth
from influentialrs_amd.engine import Engine
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
import survivors_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, UNSUPPORTED = -1, -2, -4
NINF = -np.inf


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


# ---------------------------------------------------------------- the restatement on hand-made rows
# catalog of 8 items; the exact ranking of every row is ids0 0, 1, .. 7 with scores 8, 7, .. 1; lists hold k = 3 entries
RANK = (np.arange(8, 0, -1).astype(np.float32), np.arange(8, dtype=np.int64))
K = 3


def _lists(M):
    val = np.tile(RANK[0][:K], (M, 1))
    ids = np.tile(RANK[1][:K], (M, 1))
    return val, ids


def _run(seq, hep, want, val=None, ids=None, **kw):
    seq = np.asarray(seq, dtype=np.int64)
    v0, i0 = _lists(seq.shape[0])
    val = v0 if val is None else val
    ids = i0 if ids is None else ids
    rps = kw.get("rows_per_status", 1)
    status = np.zeros(seq.shape[0] // rps, dtype=np.int32)
    return ref.ensure_survivors(seq, np.asarray(hep, dtype=np.int32), val, ids, status, want, lambda m: RANK, **kw)


def test_starved_row_gets_the_best_admissible_items_and_the_list_ends_behind_them():
    # the window holds items 1, 2, 3 (ids0 0, 1, 2): no survivor among the three candidates
    val, ids, st, starved = _run([[1, 2, 3, 0, 9]], [2], 1)
    assert starved == [0] and st[0] == ref.RESCUED
    assert ids[0].tolist() == [3, -1, 2] and val[0, 0] == 5 and val[0, 1] == NINF and val[0, 2] == 6
    # want = 2: two items, the terminator at entry 2
    val, ids, st, starved = _run([[1, 2, 3, 0, 9]], [2], 2)
    assert ids[0].tolist() == [3, 4, -1] and val[0].tolist() == [5, 4, NINF]
    # want = k: the whole list is rewritten, no room and no need for a terminator
    val, ids, st, starved = _run([[1, 2, 3, 0, 9]], [2], 3)
    assert ids[0].tolist() == [3, 4, 5] and val[0].tolist() == [5, 4, 3]


def test_rows_with_enough_survivors_are_not_written():
    v0, i0 = _lists(2)
    val, ids, st, starved = _run([[1, 2, 0, 0, 9], [5, 6, 7, 0, 9]], [1, 2], 1)
    assert starved == [] and not st.any()
    assert np.array_equal(val, v0) and np.array_equal(ids, i0)
    # one survivor is enough for want = 1 and too few for want = 2
    val, ids, st, starved = _run([[1, 2, 0, 0, 9]], [1], 2)
    assert starved == [0] and ids[0].tolist() == [2, 3, -1]


def test_a_list_that_ended_early_is_left_alone():
    val, ids = _lists(1)
    val[0, 2], ids[0, 2] = NINF, -1  # a catalog of two items: the list already is all of it
    out_val, out_ids, st, starved = _run([[1, 2, 0, 0, 9]], [1], 1, val=val, ids=ids)
    assert starved == [] and not st.any() and np.array_equal(out_ids, ids) and np.array_equal(out_val, val)


def test_a_catalog_inside_the_window_leaves_an_empty_list():
    seq = [[1, 2, 3, 4, 5, 6, 7, 8]]
    val, ids, st, starved = _run(seq, [7], 1)
    assert starved == [0] and st[0] == ref.RESCUED
    assert ids[0, 0] == -1 and val[0, 0] == NINF  # the path step then finds no survivor: IRS_ROW_NO_CANDIDATE
    assert ref.survivors(seq[0], val[0], ids[0], 1) == []


def test_positions_beyond_hep_do_not_count():
    # items 1, 2, 3 in the window; item 4 sits at hep + 1 and is admissible
    val, ids, st, starved = _run([[1, 2, 3, 4, 9]], [2], 1)
    assert ids[0, 0] == 3
    # ... and it is not once hep covers it
    val, ids, st, starved = _run([[1, 2, 3, 4, 9]], [3], 1)
    assert ids[0, 0] == 4
    # hep = -1: an empty window, nothing is starved
    assert _run([[1, 2, 3, 4, 9]], [-1], 3)[3] == []


def test_skipped_rows_and_the_status_word_of_a_user():
    seq = [[1, 2, 3, 0, 9]] * 4
    cum = np.array([0.0, NINF, 0.0, 0.0])
    fin = np.array([0, 0, 1, 0], dtype=np.int32)
    val, ids, st, starved = _run(seq, [2] * 4, 1, cum=cum, fin=fin, rows_per_status=2)
    assert starved == [0, 3] and st.tolist() == [ref.RESCUED, ref.RESCUED]
    v0, i0 = _lists(4)
    assert np.array_equal(ids[[1, 2]], i0[[1, 2]]) and np.array_equal(val[[1, 2]], v0[[1, 2]])
    val, ids, st, starved = _run(seq, [2] * 4, 1, done=np.array([1, 0], dtype=np.int32), rows_per_status=2)
    assert starved == [2, 3] and st.tolist() == [0, ref.RESCUED]


# ---------------------------------------------------------------- declared, exported, bound
def test_names_in_header_exports_and_ctypes_table():
    lib = _lib.load()
    txt = open(os.path.join(REPO, "include", "irs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"#define\s+IRS_ROW_RESCUED\s+8\b", code) and _lib.IRS_ROW_RESCUED == 8 == ref.RESCUED
    for name, nargs in (("irs_survivor_scratch_bytes", 3), ("irs_topk_ensure_survivors", 17), ("irs_bind_survivor_scratch", 3)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["irs_survivor_scratch_bytes"][0] is ctypes.c_size_t


# ---------------------------------------------------------------- the scratch size
def test_scratch_bytes_invalid_arguments_and_bound():
    lib, h = _ctx()
    try:
        f = lib.irs_survivor_scratch_bytes
        assert f(None, 4, 1) == 0
        for rows, want in ((0, 1), (-3, 1), (4, 0), (4, -1), (4, 33)):
            assert f(h, rows, want) == 0, (rows, want)
        # 256 + 4 rows rounded up to 16 + 8 rows strips want, strips = 4 at 1000 items (1000 / 128 = 7.8)
        assert f(h, 1, 1) == 256 + 16 + 8 * 4
        assert f(h, 64, 32) == 256 + 256 + 8 * 64 * 4 * 32
        assert f(h, 7, 3) % 16 == 0
    finally:
        lib.irs_destroy(h)
    for n_item, strips in ((100, 1), (255, 1), (256, 2), (300, 2), (1 << 20, 256), (10_000_000, 256)):
        lib, h = _ctx(n_item=n_item)
        try:
            assert lib.irs_survivor_scratch_bytes(h, 8, 2) == 256 + 32 + 8 * 8 * strips * 2, n_item
            # the documented bound: never of order rows x n_item
            for rows, want in ((1, 1), (4096, 1), (4096, 8), (131072, 32), (1 << 20, 32)):
                n = lib.irs_survivor_scratch_bytes(h, rows, want)
                assert 0 < n <= 272 + 4 * rows + 8 * max(1 << 21, rows * want), (n_item, rows, want, n)
        finally:
            lib.irs_destroy(h)


# ---------------------------------------------------------------- argument checks, before any launch
def _ensure_args(**kw):
    """A complete argument list of irs_topk_ensure_survivors with fake non-null addresses (nothing is dereferenced: every
    call here is refused before a launch), then the overrides."""
    p = ctypes.c_void_p
    a = dict(xrows=p(4096), seq=p(4096), hep=p(4096), M=8, rps=1, k=100, want=1, cum=None, fin=None, done=None, val=p(4096),
             ids0=p(4096), status=p(4096), scratch=p(4096), scratch_bytes=1 << 24, stream=None)
    a.update(kw)
    return [a[n] for n in ("xrows", "seq", "hep", "M", "rps", "k", "want", "cum", "fin", "done", "val", "ids0", "status",
                           "scratch", "scratch_bytes", "stream")]


def test_ensure_survivors_argument_checks():
    lib, h = _ctx()
    try:
        f = lib.irs_topk_ensure_survivors
        assert f(None, *_ensure_args()) == INVALID
        for name in ("xrows", "seq", "hep", "val", "ids0", "status", "scratch"):
            assert f(h, *_ensure_args(**{name: None})) == INVALID, name
        assert b"null" in lib.irs_last_error(h)
        for bad in (dict(M=0), dict(M=-1), dict(want=0), dict(want=33), dict(k=8, want=9), dict(k=0), dict(k=101),
                    dict(rps=0), dict(rps=-2), dict(rps=3), dict(M=8, rps=16)):
            assert f(h, *_ensure_args(**bad)) == INVALID, bad
        need = lib.irs_survivor_scratch_bytes(h, 8, 1)
        assert f(h, *_ensure_args(scratch_bytes=need - 1)) == INVALID and b"too small" in lib.irs_last_error(h)
        assert f(h, *_ensure_args(scratch_bytes=0)) == INVALID
        assert f(h, *_ensure_args(scratch=ctypes.c_void_p(4096 + 8))) == INVALID and b"aligned" in lib.irs_last_error(h)
        # everything valid: nothing is bound on this context
        assert f(h, *_ensure_args(scratch_bytes=need)) == STATE
        # the optional pointers are optional
        assert f(h, *_ensure_args(cum=ctypes.c_void_p(4096), fin=ctypes.c_void_p(4096), done=ctypes.c_void_p(4096))) == STATE
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        assert lib.irs_topk_ensure_survivors(h, *_ensure_args()) == UNSUPPORTED
        assert b"whole catalog" in lib.irs_last_error(h)
        assert lib.irs_topk_ensure_survivors(h, *_ensure_args(M=0)) == INVALID  # the argument checks come first
    finally:
        lib.irs_destroy(h)


def test_bind_checks_and_the_sharded_loops_refuse_a_bound_scratch():
    lib, h = _ctx()
    try:
        f = lib.irs_bind_survivor_scratch
        assert f(None, ctypes.c_void_p(4096), 64) == INVALID
        assert f(h, None, 64) == INVALID and f(h, ctypes.c_void_p(4096), 0) == INVALID
        assert f(h, ctypes.c_void_p(4096 + 4), 64) == INVALID and b"aligned" in lib.irs_last_error(h)
        assert f(h, ctypes.c_void_p(4096), 64) == 0
        assert f(h, None, 0) == 0 and f(h, None, 0) == 0  # unbinding twice is fine
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    comm = ctypes.c_void_p()

    def never(*a):  # pragma: no cover
        raise AssertionError("a collective ran")

    cbs = (_lib.ALLGATHER_FN(never), _lib.ALLTOALL_FN(never), _lib.ALLREDUCE_F32_FN(never))
    assert lib.irs_comm_init_callbacks(ctypes.byref(comm), 0, 2, None, ctypes.cast(cbs[0], ctypes.c_void_p),
                                       ctypes.cast(cbs[1], ctypes.c_void_p), ctypes.cast(cbs[2], ctypes.c_void_p)) == 0
    try:
        p = ctypes.c_void_p(4096)
        paths_args = (comm, p, p, p, 4, 3, 100, 0, 0, 0, 0, 0, p, p, None)
        beam_args = (comm, p, p, p, 2, 2, 3, 100, 0, 0, 0, p, p, None, p, None)
        # unbound: the loops get as far as the unbound weights
        assert lib.irs_generate_paths_sharded(h, *paths_args) == STATE
        assert lib.irs_beam_search_sharded(h, *beam_args) == STATE
        assert lib.irs_bind_survivor_scratch(h, p, 1 << 20) == 0
        assert lib.irs_generate_paths_sharded(h, *paths_args) == UNSUPPORTED and b"whole catalog" in lib.irs_last_error(h)
        assert lib.irs_beam_search_sharded(h, *beam_args) == UNSUPPORTED
        assert lib.irs_bind_survivor_scratch(h, None, 0) == 0
        assert lib.irs_generate_paths_sharded(h, *paths_args) == STATE
    finally:
        lib.irs_comm_destroy(comm)
        lib.irs_destroy(h)


# ---------------------------------------------------------------- Python layers
def test_keyword_is_off_by_default_everywhere():
    for fn in (Engine.generate_paths, Engine.generate_paths_until, Engine.beam_search, Engine.beam_search_until):
        assert inspect.signature(fn).parameters["exact_candidates"].default is False, fn
    assert hasattr(Engine, "ensure_survivors")
    # the front end takes the keyword in a wrapper: off by default, keyword only, the declared parameters as they were
    sig = inspect.signature(IRSNN.get_seq_in_batch, follow_wrapped=False).parameters
    assert sig["exact_candidates"].default is False and sig["exact_candidates"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(IRSNN.get_seq_in_batch).parameters)[-1] == "beam_stop"


def test_front_end_refuses_an_item_sharded_module_without_a_device():
    cfg = synth.make_config("tiny")
    net = InfluentialNet(cfg)
    net.shard_items(0, 2, drop_full=False)
    irn = IRSNN(cfg, net, "cpu")
    B, L = 2, cfg.max_len
    seqs, users, targets = torch.ones((B, L), dtype=torch.int64), torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.int64)
    with pytest.raises(ValueError, match="exact_candidates is not built for an item-sharded catalog"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, exact_candidates=True)
    with pytest.raises(ValueError, match="exact_candidates"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, beam_width=4, exact_candidates=True)
    assert irn._exact_candidates is False, "the switch lasts for the call"


def test_harness_passes_the_keyword_only_when_the_config_sets_it():
    from influentialrs_amd import harness
    cfg = synth.make_config("tiny")
    for k, v in dict(gap_len=0, batch_size=2, top_k=5, use_h=False, max_path_len=3, sample=False, sample_k=3).items():
        setattr(cfg, k, v)
    rows = [(np.array([1, 2, 3]), 0, 9, 4), (np.array([2, 5]), 1, 8, 6)]
    seen = []

    class Handler:
        def eval(self):
            pass

        def get_pif_in_batch(self, seq, u):
            return np.zeros((seq.shape[0], 1), dtype=np.float32)

        def get_accuracy_metrics_in_batch(self, raw, seq, u, t, l, top_k, gap_len, use_h):
            return 0, np.ones(seq.shape[0])

        def get_seq_in_batch(self, seq, u, t, max_path_len, gap_len, sample, sample_k, **kw):
            seen.append(kw)
            B = seq.shape[0]
            return np.zeros((B, max_path_len), dtype=np.float32), t.numpy(), [np.array([1])] * B, 0

    harness.test_model(cfg, rows, Handler(), "cpu", verbose=False)
    cfg.exact_candidates = True
    harness.test_model(cfg, rows, Handler(), "cpu", verbose=False)
    cfg.stop_at_target = True
    harness.test_model(cfg, rows, Handler(), "cpu", verbose=False)
    assert seen == [{}, {"exact_candidates": True}, {"stop_at_target": True, "exact_candidates": True}]
