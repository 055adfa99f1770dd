"""not-gpu: bound exclusions (irs_bind_exclusions): the restatement the GPU tests compare against, on hand-made rows; the
scratch size; every refusal of the binding through the ABI on a context created without a device; the Python layers."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import beam_until_ref
import exclusion_ref as ref
import path_ref
from influentialrs_amd import _lib, synth
from influentialrs_amd.engine import Engine
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet, exclusion_ids0

INVALID, STATE, UNSUPPORTED = -1, -2, -4
NINF = -np.inf
N_ITEM = 8
# every row's list: ids0 0 .. 5 with scores 8 .. 3
VAL = np.arange(8, 2, -1).astype(np.float32)
IDS = np.arange(6, dtype=np.int64)


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


# ---------------------------------------------------------------- the restatement
def test_membership_is_window_or_list_or_path():
    excl = np.array([4, -1, 4, 9, 2], dtype=np.int64)  # a hole, a duplicate, an id >= n_item
    assert ref.hidden(excl, N_ITEM) == {5, 3}
    assert ref.hidden(None, N_ITEM) == set()
    path = np.array([6, 0, 7, 1], dtype=np.float32)
    assert ref.hidden(excl, N_ITEM, path, 3, no_repeat=False) == {5, 3}, "the path counts under no_repeat only"
    assert ref.hidden(excl, N_ITEM, path, 3, no_repeat=True) == {5, 3, 6, 7}, "entries [0, step), zeros are no items"
    assert ref.hidden(None, N_ITEM, path, 4, no_repeat=True) == {6, 7, 1}
    window = [2, 8]
    assert [ref.is_member(i, window, excl, N_ITEM, path, 3, True) for i in range(1, 9)] == [False, True, True, False, True, True, True,
                                                                                           True]


def test_sorted_row_is_what_the_prepare_launch_writes():
    big = np.iinfo(np.int64).max
    row, n = ref.sorted_row(np.array([5, -1, 2, 5, 99, 0], dtype=np.int64), N_ITEM)
    assert n == 4 and row.tolist() == [0, 2, 5, 5, big, big, big, big]
    row, n = ref.sorted_row(np.array([-1, -1, -1], dtype=np.int64), N_ITEM)
    assert n == 0 and row.tolist() == [big] * 4
    row, n = ref.sorted_row(np.array([3], dtype=np.int64), N_ITEM)
    assert n == 1 and row.tolist() == [3]
    row, n = ref.sorted_row(np.zeros(0, dtype=np.int64), N_ITEM)
    assert n == 0 and len(row) == 0


def test_strike_keeps_the_order_and_the_end():
    v, i = ref.strike(VAL, IDS, {1, 4})
    assert i.tolist() == [1, 2, 4, 5, -1, -1] and v[:4].tolist() == [7, 6, 4, 3] and np.isneginf(v[4:]).all()
    ids = IDS.copy()
    ids[3] = -1  # the list ends early: entries behind the end do not come back
    v, i = ref.strike(VAL, ids, {2})
    assert i.tolist() == [0, 2, -1, -1, -1, -1]


def _state(B=2, L=6, P=4):
    seq = np.zeros((B, L), dtype=np.int64)
    seq[:, 0] = 1  # the window holds item 1 (id0 0)
    seq[:, L - 1] = 8
    return seq, np.zeros(B, dtype=np.int32), np.zeros((B, P), dtype=np.float32), np.zeros(B, dtype=np.int32)


def test_path_step_drops_window_list_and_path():
    seq, hep, paths, status = _state()
    val, ids = np.tile(VAL, (2, 1)), np.tile(IDS, (2, 1))
    excl = np.array([[1, -1], [-1, -1]], dtype=np.int64)
    s, h, p, st = ref.path_step(seq, hep, val, ids, 0, paths, status, excl, N_ITEM)
    assert p[:, 0].tolist() == [3, 2] and h.tolist() == [1, 1] and s[0, 1] == 3 and s[1, 1] == 2 and not st.any()
    # step 1 without no_repeat: row 1 is offered nothing new by the list; the window holds its step-0 choice anyway
    s2, h2, p2, _ = ref.path_step(s, h, val, ids, 1, p, st, excl, N_ITEM)
    assert p2[:, 1].tolist() == [4, 3]
    # an item that slid out of the window comes back unless no_repeat holds it: a window of one slot before the target
    seq = np.array([[2, 8]], dtype=np.int64)
    hep0, paths0, status0 = np.zeros(1, dtype=np.int32), np.array([[2, 0, 0]], dtype=np.float32), np.zeros(1, dtype=np.int32)
    seq[0, 0] = 3  # the path's item 2 has left the window
    ids1, val1 = np.array([[1, 2, 3]], dtype=np.int64), np.array([[9, 8, 7]], dtype=np.float32)
    again = ref.path_step(seq, hep0, val1, ids1, 1, paths0, status0, None, N_ITEM, no_repeat=False)
    fresh = ref.path_step(seq, hep0, val1, ids1, 1, paths0, status0, None, N_ITEM, no_repeat=True)
    assert again[2][0, 1] == 2 and fresh[2][0, 1] == 4


def test_path_step_without_a_survivor_leaves_the_row_alone():
    seq, hep, paths, status = _state(B=1)
    excl = np.array([[1, 2, 3, 4, 5]], dtype=np.int64)  # with the window's id0 0: the whole list
    s, h, p, st = ref.path_step(seq, hep, VAL[None], IDS[None], 2, paths, status, excl, N_ITEM)
    assert st[0] == path_ref.NO_CANDIDATE and p[0, 2] == 0 and np.array_equal(s, seq) and np.array_equal(h, hep)


def test_sampled_path_step_draws_among_the_first_admissible():
    seq, hep, paths, status = _state(B=1)
    excl = np.array([[2, 3]], dtype=np.int64)
    (items, prob), = ref.path_step(seq, hep, VAL[None], IDS[None], 0, paths, status, excl, N_ITEM, sample=True, sample_k=3)
    assert items.tolist() == [2, 5, 6] and abs(prob.sum() - 1) < 1e-12 and prob[0] > prob[1] > prob[2]


def _beam_state(W=2, L=6, P=3):
    seq = np.zeros((1, W, L), dtype=np.int64)
    seq[..., 0] = 1
    seq[..., L - 1] = 8
    hep = np.zeros((1, W), dtype=np.int32)
    cum = np.array([[0.0, -1.0]])
    paths = np.zeros((1, W, P), dtype=np.float32)
    return seq, hep, cum, paths


def test_beam_step_shares_the_list_and_reads_the_parents_path():
    W = 2
    seq, hep, cum, paths = _beam_state(W)
    paths[0, 0, 0], paths[0, 1, 0] = 2, 3  # step 0's choices; the window (one item) does not show them
    val, ids = np.tile(VAL, (W, 1)), np.tile(IDS, (W, 1))
    lmax, lsum = np.zeros(W), np.ones(W)
    excl = np.array([[3]], dtype=np.int64)  # item 4, for both beams
    (s, h, c, p), st = ref.beam_step((seq, hep, cum, paths), val, ids, lmax, lsum, 1, 3, excl, N_ITEM, no_repeat=True)
    # beam 0 (cum 0) sees 3, 5 (not 1: window, 2: own path, 4: list): 6, 4; beam 1 (cum -1) sees 2, 5 (not 3: own path): 6, 3
    assert p[0, :, :2].tolist() == [[2, 3], [3, 2]] and c[0].tolist() == [6.0, 6.0], "the tie goes to the lower parent"
    (s, h, c, p), st = ref.beam_step((seq, hep, cum, paths), val, ids, lmax, lsum, 1, 3, excl, N_ITEM, no_repeat=False)
    assert p[0, :, :2].tolist() == [[2, 2], [2, 3]] and c[0].tolist() == [7.0, 6.0], "beam 0 may repeat its own item 2"
    plain, _ = path_ref.beam_step((seq, hep, cum, paths), val, ids, lmax, lsum, 1, 3)
    unbound, _ = ref.beam_step((seq, hep, cum, paths), val, ids, lmax, lsum, 1, 3, None, N_ITEM)
    assert all(np.array_equal(a, b) for a, b in zip(plain, unbound))


def test_beam_step_until_never_reads_a_finished_beams_list():
    W = 2
    seq, hep, cum, paths = _beam_state(W)
    fin = np.array([[0, 1]], dtype=np.int32)
    val, ids = np.tile(VAL, (W, 1)), np.tile(IDS, (W, 1))
    ids[1] = 10 ** 12  # garbage
    excl = np.array([[1]], dtype=np.int64)
    done = np.zeros(1, dtype=np.int32)
    (s, h, c, p, f), d, st = ref.beam_step_until((seq, hep, cum, paths, fin), done, val, ids, np.zeros(W), np.ones(W), 0, 3,
                                                 beam_until_ref.STOP_ALL, excl, N_ITEM, no_repeat=True)
    assert c[0].tolist() == [6.0, 5.0] and p[0, :, 0].tolist() == [3, 4] and f[0].tolist() == [0, 0] and d[0] == 0
    cum[0, 1] = 7.0  # the finished beam outranks them: it stays, whole
    (s, h, c, p, f), d, st = ref.beam_step_until((seq, hep, cum, paths, fin), done, val, ids, np.zeros(W), np.ones(W), 0, 3,
                                                 beam_until_ref.STOP_BEST, excl, N_ITEM)
    assert c[0].tolist() == [7.0, 6.0] and f[0].tolist() == [1, 0] and d[0] == 1


def test_ensure_survivors_counts_the_list_and_ranks_outside_it():
    rank = (np.arange(8, 0, -1).astype(np.float32), np.arange(8, dtype=np.int64))
    seq = np.array([[1, 0, 0, 9], [1, 0, 0, 9], [1, 0, 0, 9]], dtype=np.int64)
    hep = np.zeros(3, dtype=np.int32)
    val, ids = np.tile(rank[0][:3], (3, 1)), np.tile(rank[1][:3], (3, 1))
    excl = np.array([[1, 2, 4], [1, -1, -1], [1, 2, 4]], dtype=np.int64)
    paths = np.array([[4, 0], [0, 0], [0, 0]], dtype=np.float32)
    v, i, st, starved = ref.ensure_survivors(seq, hep, val, ids, np.zeros(3, dtype=np.int32), 1, lambda m: rank, excl, N_ITEM,
                                             paths=paths, step=1, no_repeat=True)
    assert starved == [0, 2]
    assert i[0].tolist() == [5, -1, 2] and v[0, 0] == 3, "items 1 (window), 2, 3, 5 (list) and 4 (path) are gone: item 6"
    assert i[2].tolist() == [3, -1, 2] and i[1].tolist() == [0, 1, 2] and st.tolist() == [8, 0, 8]
    # two rows per user: both read user 0's list, and the standalone form has no path
    v, i, st, starved = ref.ensure_survivors(seq[:2], hep[:2], val[:2], ids[:2], np.zeros(1, dtype=np.int32), 2, lambda m: rank, excl,
                                             N_ITEM, rows_per_status=2)
    assert starved == [0, 1] and i[0].tolist() == [3, 5, -1] and i[1].tolist() == [3, 5, -1] and st.tolist() == [8]


# ---------------------------------------------------------------- the scratch size
def test_scratch_bytes_values_and_zeros():
    lib, h = _ctx()
    try:
        f = lib.irs_exclusion_scratch_bytes
        assert f(None, 4, 8) == 0
        for users, n in ((0, 8), (-1, 8), (4, -1), (4, 4097)):
            assert f(h, users, n) == 0 == ref.scratch_bytes(users, n), (users, n)
        assert f(h, 1, 0) == 16 and f(h, 5, 0) == 32
        assert f(h, 1, 1) == 16 + 8 and f(h, 3, 63) == 16 + 8 * 3 * 64 and f(h, 3, 64) == 16 + 8 * 3 * 64
        assert f(h, 3, 65) == 16 + 8 * 3 * 128 and f(h, 4096, 4096) == 4 * 4096 + 8 * 4096 * 4096
        for users, n in ((1, 0), (7, 3), (64, 100), (4096, 2276), (9, 4096)):
            assert f(h, users, n) == ref.scratch_bytes(users, n) and f(h, users, n) % 16 == 0
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- refusals, before any launch
def test_bind_refusals_without_a_device():
    p = ctypes.c_void_p
    lib, h = _ctx()
    try:
        f = lib.irs_bind_exclusions
        big = 1 << 26
        assert f(None, p(4096), 4, 8, 0, p(4096), big, None) == INVALID
        assert f(h, None, 0, 0, 0, None, 0, None) == 0, "unbinding what was never bound is fine"
        assert f(h, p(4096), 4, 4097, 0, p(4096), 1 << 30, None) == UNSUPPORTED and b"4096" in lib.irs_last_error(h)
        assert f(h, p(4096), 4, -1, 0, p(4096), big, None) == INVALID
        assert f(h, p(4096), 0, 8, 0, p(4096), big, None) == INVALID and b"users" in lib.irs_last_error(h)
        assert f(h, p(4096), -2, 8, 1, p(4096), big, None) == INVALID
        assert f(h, None, 4, 8, 0, p(4096), big, None) == INVALID, "n_excl >= 1 without a list"
        assert f(h, p(4096), 4, 0, 1, p(4096), big, None) == INVALID, "a list without n_excl >= 1"
        assert f(h, None, 4, 0, 0, p(4096), big, None) == INVALID, "neither a list nor no_repeat"
        need = lib.irs_exclusion_scratch_bytes(h, 4, 8)
        assert f(h, p(4096), 4, 8, 0, p(4096), need - 1, None) == INVALID and b"too small" in lib.irs_last_error(h)
        assert f(h, p(4096), 4, 8, 0, None, need, None) == INVALID
        assert f(h, p(4096), 4, 8, 0, p(4096), 0, None) == INVALID
        assert f(h, p(4096), 4, 8, 0, p(4096 + 8), big, None) == INVALID and b"aligned" in lib.irs_last_error(h)
        assert f(h, None, 4, 0, 1, p(4096 + 4), big, None) == INVALID
        # nothing of the above bound anything: an entry point gets as far as the unbound weights
        assert lib.irs_generate_paths(h, p(4096), p(4096), p(4096), 64, 3, 100, 0, 0, 0, 0, 0, p(4096), p(4096), None) == STATE
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        assert lib.irs_bind_exclusions(h, p(4096), 4, 8, 0, p(4096), 1 << 26, None) == UNSUPPORTED
        assert b"whole catalog" in lib.irs_last_error(h)
        assert lib.irs_bind_exclusions(h, None, 4, 0, 1, p(4096), 1 << 26, None) == UNSUPPORTED
        assert lib.irs_bind_exclusions(h, None, 0, 0, 0, None, 0, None) == 0
    finally:
        lib.irs_destroy(h)


def test_the_two_symbols_are_in_the_ctypes_table():
    sig = _lib.SIGNATURES
    assert sig["irs_exclusion_scratch_bytes"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32])
    res, args = sig["irs_bind_exclusions"]
    assert res is ctypes.c_int32 and len(args) == 8 and args[6] is ctypes.c_size_t
    lib = _lib.load()
    assert hasattr(lib, "irs_bind_exclusions") and hasattr(lib, "irs_exclusion_scratch_bytes")


# ---------------------------------------------------------------- Python layers
def test_keywords_are_off_by_default_everywhere():
    for fn in (Engine.generate_paths, Engine.generate_paths_until, Engine.beam_search, Engine.beam_search_until):
        par = inspect.signature(fn).parameters
        assert par["exclude"].default is None and par["no_repeat"].default is False, fn
    assert hasattr(Engine, "exclusion_scratch_bytes") and hasattr(Engine, "bind_exclusions") and hasattr(Engine, "unbind_exclusions")
    sig = inspect.signature(IRSNN.get_seq_in_batch, follow_wrapped=False).parameters
    for name, default in (("exclude", None), ("no_repeat", False)):
        assert sig[name].default is default and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(IRSNN.get_seq_in_batch).parameters)[-1] == "beam_stop"


def test_front_end_lists_take_both_forms_and_no_repeat_adds_the_window():
    seqs = torch.tensor([[0, 3, 4, 0, 9], [5, 6, 7, 0, 2]], dtype=torch.int64)
    ragged = [np.array([8, 1]), torch.tensor([2])]
    a = exclusion_ids0(ragged, False, seqs, 2, "cpu")
    assert a.dtype == torch.int64 and a.tolist() == [[7, 0], [1, -1]]
    padded = torch.tensor([[8, 1], [2, 0]])
    assert exclusion_ids0(padded, False, seqs, 2, "cpu").tolist() == [[7, 0], [1, -1]]
    b = exclusion_ids0(ragged, True, seqs, 2, "cpu")
    assert b.tolist() == [[7, 0, -1, 2, 3], [1, -1, 4, 5, 6]], "the window seqs[:, :hep + 1], pads as unused slots; not the target"
    assert exclusion_ids0(None, True, seqs, 1, "cpu").tolist() == [[-1, 2], [4, 5]]
    assert exclusion_ids0(None, False, seqs, 2, "cpu") is None
    with pytest.raises(ValueError, match="exclude"):
        exclusion_ids0([np.array([1])], False, seqs, 2, "cpu")
    with pytest.raises(ValueError, match="exclude"):
        exclusion_ids0(torch.zeros((3, 2), dtype=torch.int64), False, seqs, 2, "cpu")


def test_front_end_refuses_an_item_sharded_module_without_a_device():
    cfg = synth.make_config("tiny")
    net = InfluentialNet(cfg)
    net.shard_items(0, 2, drop_full=False)
    irn = IRSNN(cfg, net, "cpu")
    B, L = 2, cfg.max_len
    seqs, users, targets = torch.ones((B, L), dtype=torch.int64), torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.int64)
    with pytest.raises(ValueError, match="exclude / no_repeat is not built for an item-sharded catalog"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, exclude=[np.array([1]), np.array([2])])
    with pytest.raises(ValueError, match="no_repeat is not built"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, beam_width=4, no_repeat=True)
    assert irn._exclude is None and irn._no_repeat is False, "the switches last for the call"


def test_harness_passes_the_keywords_only_when_the_config_sets_them():
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
            self.raw = raw
            return 0, np.ones(seq.shape[0])

        def get_seq_in_batch(self, seq, u, t, max_path_len, gap_len, sample, sample_k, **kw):
            seen.append((kw, self.raw))
            B = seq.shape[0]
            return np.zeros((B, max_path_len), dtype=np.float32), t.numpy(), [np.array([1])] * B, 0

    harness.test_model(cfg, rows, Handler(), "cpu", verbose=False)
    cfg.no_repeat = True
    harness.test_model(cfg, rows, Handler(), "cpu", verbose=False)
    cfg.exclude_history = True
    harness.test_model(cfg, rows, Handler(), "cpu", verbose=False)
    assert seen[0][0] == {} and seen[1][0] == {"no_repeat": True}
    kw, raw = seen[2]
    assert sorted(kw) == ["exclude", "no_repeat"] and kw["exclude"] is raw, "the batch's raw histories, as the metric filters them"
