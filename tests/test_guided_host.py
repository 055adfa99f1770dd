"""not-gpu: the guided choice (irs_bind_guide): the numpy statement (tests/guided_ref.py) against what the reference's own
distance function chooses (tests/golden/guided_choice.npz, make_guided_golden.py), the new symbols in header, library and
ctypes table, the scratch size, every refusal of the binding and of the bound entry points on a context created without a
device, and the Python layers."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import guided_ref as ref
import path_ref
from influentialrs_amd import _lib, synth
from influentialrs_amd.engine import Engine
from influentialrs_amd.model import Rec2Inf
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
from influentialrs_amd.model.rec2inf import rec2inf_windows
from influentialrs_amd.model.uRS import SampleNet

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "guided_choice.npz")
INVALID, STATE, UNSUPPORTED = -1, -2, -4
BINARY, FLOAT = _lib.IRS_GUIDE_BINARY, _lib.IRS_GUIDE_FLOAT
GROUPS = (("bin18", ref.BINARY), ("f1", ref.FLOAT), ("f3", ref.FLOAT), ("f64", ref.FLOAT))


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


# ---------------------------------------------------------------- the statement against the reference's distance function
@pytest.mark.parametrize("name,kind", GROUPS)
def test_statement_reproduces_the_reference_choice(name, kind):
    """`chosen_stable` is the reference's line with a stable argsort (the first of the nearest: what its pinned numpy returns up
    to 16 candidates, and what the header defines); the statement must reproduce it on EVERY row, ties included.  `chosen` is
    the line verbatim under the generating numpy, whose default argsort returns any of several equal distances: it may differ
    from the stable choice only inside an exact tie of the minimum.  (As generated: 9 of 96 binary rows and 11 of 96 F = 1
    rows differ that way, none of the F = 3 / F = 64 rows.)"""
    z = np.load(GOLDEN)
    table = z[f"{name}_table"]
    n_rows, tied = len(z[f"{name}_count"]), 0
    assert n_rows >= 64 and set(z[f"{name}_count"].tolist()) == set(range(1, 33))
    for r in range(n_rows):
        n, t = int(z[f"{name}_count"][r]), int(z[f"{name}_target"][r])
        items = [int(x) for x in z[f"{name}_cands"][r, :n]]
        got = ref.choose(table, kind, t, items)
        assert got == int(z[f"{name}_chosen_stable"][r]), (name, r, items, t)
        dist = (lambda c: float(ref.dist_float(table, t, c))) if kind == ref.FLOAT else (lambda c: ref.dist_binary(table, t, c))
        d = [dist(c) for c in items]
        assert d[got] == min(d) and got == d.index(min(d))
        verbatim = int(z[f"{name}_chosen"][r])
        assert d[verbatim] == d[got], "the unstable argsort may only move inside an exact tie"
        tied += d.count(min(d)) > 1
    if name in ("bin18", "f1"):
        assert tied >= 30, "the golden is meant to be full of exact ties"


def test_float_chain_is_the_float32_fma_chain():
    # 3 * 3 + 2^24 is not a float32: the chain rounds once per step, to even here
    tab = np.array([[0, 0], [3, 4096], [0, 0]], dtype=np.float32)
    assert ref.dist_float(tab, 2, 1) == np.float32(16777216.0 + 8.0), "9 + 2^24 rounds to 2^24 + 8"
    assert ref.fma32(np.float32(3), np.float32(3), np.float32(16777216.0)) == np.float32(16777224.0)
    # a product whose low bits only an fma keeps: (1 + 2^-12)^2 - 1 = 2^-11 + 2^-24
    a = np.float32(1 + 2.0 ** -12)
    assert ref.fma32(a, a, np.float32(-1)) == np.float32(2.0 ** -11 + 2.0 ** -24)
    assert np.isnan(ref.dist_float(np.array([[0], [np.nan], [1]], dtype=np.float32), 1, 2))


def test_nan_sorts_last_and_ties_keep_the_better_rank():
    tab = np.array([[0], [0], [np.nan], [2], [-2], [5]], dtype=np.float32)  # items 1 .. 5; target 1 = 0.0
    assert ref.choose(tab, ref.FLOAT, 1, [2, 3, 4]) == 1, "a NaN first survivor is replaced by the first real distance"
    assert ref.choose(tab, ref.FLOAT, 1, [5, 3, 4, 2]) == 1, "3 and 4 tie at distance 4: the better rank"
    assert ref.choose(tab, ref.FLOAT, 2, [3, 4, 5]) == 0, "all NaN (the target's own row): the first survivor"
    assert ref.choose(tab, ref.FLOAT, 0, [5, 3]) == 0 and ref.choose(tab, ref.FLOAT, 6, [5, 3]) == 0, "no target: greedy"
    assert ref.choose(tab, ref.FLOAT, 1, [5, 9, 3]) == 2, "an id outside the table is the farthest"
    bits = np.array([[0, 0, 0], [1, 1, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.uint8)
    assert ref.choose(bits, ref.BINARY, 1, [2, 3, 4]) == 2 and ref.choose(bits, ref.BINARY, 1, [2, 3]) == 0
    assert ref.choose(bits, ref.BINARY, 1, [7, 3]) == 1


def test_pack_bits_layout():
    t = np.zeros((2, 33), dtype=np.uint8)
    t[1, [0, 31, 32]] = (1, 7, 200)  # nonzero = 1
    p = ref.pack_bits(t)
    assert p.shape == (2, 2) and p[0].tolist() == [0, 0] and p[1].tolist() == [0x80000001, 1]


def _state(B, L, P=4):
    seq = np.zeros((B, L), dtype=np.int64)
    seq[:, 0] = 1
    seq[:, L - 1] = 4
    return seq, np.zeros(B, dtype=np.int32), np.zeros((B, P), dtype=np.float32), np.zeros(B, dtype=np.int32)


def test_k_c_one_or_an_all_equal_table_is_the_greedy_step():
    g = np.random.default_rng(3)
    B, L, k, n_item = 6, 7, 9, 40
    seq, hep, paths, status = _state(B, L)
    ids0 = np.stack([g.permutation(n_item)[:k] for _ in range(B)]).astype(np.int64)
    ids0[2, 3:] = -1
    ids0[4, :] = 0  # only item 1, which the window holds: no candidate
    ids0[4, 1:] = -1
    val = -np.sort(-g.standard_normal((B, k)).astype(np.float32), axis=1)
    plain = path_ref.path_step(seq, hep, val, ids0, 1, paths, status)
    table = g.integers(0, 2, size=(n_item + 1, 18)).astype(np.uint8)
    for got in (ref.path_step(seq, hep, val, ids0, 1, paths, status, table, ref.BINARY, 1),
                ref.path_step(seq, hep, val, ids0, 1, paths, status, np.ones((n_item + 1, 3), dtype=np.float32), ref.FLOAT, 5),
                ref.path_step(seq, hep, val, ids0, 1, paths, status, np.zeros((n_item + 1, 40), dtype=np.uint8), ref.BINARY, 9)):
        assert all(np.array_equal(a, b) for a, b in zip(plain, got))
    assert plain[3][4] == path_ref.NO_CANDIDATE
    # and a table that matters moves at least one row off the greedy choice, to the nearest of its first five survivors
    guided = ref.path_step(seq, hep, val, ids0, 1, paths, status, table, ref.BINARY, 5)
    assert (guided[2][:, 1] != plain[2][:, 1]).any()
    for r in range(B):
        surv = [s[0] for s in path_ref.survivors(seq[r, :1], val[r], ids0[r], 5)]
        if surv:
            d = [ref.dist_binary(table, 4, c) for c in surv]
            assert guided[2][r, 1] == surv[d.index(min(d))]


def test_guided_step_composes_with_exclusions():
    seq, hep, paths, status = _state(1, 6)
    ids0 = np.array([[1, 2, 4, 5, 6]], dtype=np.int64)  # items 2, 3, 5, 6, 7
    val = np.array([[5, 4, 3, 2, 1]], dtype=np.float32)
    table = np.zeros((9, 1), dtype=np.float32)
    table[:, 0] = [0, 0, 9, 1, 0, 8, 7, 0.5, 0]  # the target 4 sits at 0: item 7 is nearest, then 3
    assert ref.path_step(seq, hep, val, ids0, 0, paths, status, table, ref.FLOAT, 3)[2][0, 0] == 3, "7 is not among the first 3"
    excl = np.array([[1]], dtype=np.int64)  # item 2 goes: the first three admissible are 3, 5, 6
    assert ref.path_step(seq, hep, val, ids0, 0, paths, status, table, ref.FLOAT, 3, excl, 8)[2][0, 0] == 3
    excl = np.array([[2]], dtype=np.int64)  # item 3 goes: 2, 5, 6 -> 6
    assert ref.path_step(seq, hep, val, ids0, 0, paths, status, table, ref.FLOAT, 3, excl, 8)[2][0, 0] == 6
    paths[0, 0] = 3
    assert ref.path_step(seq, hep, val, ids0, 1, paths, status, table, ref.FLOAT, 4, None, 8, no_repeat=True)[2][0, 1] == 7


# ---------------------------------------------------------------- symbols, scratch size
def test_new_symbols_in_header_library_and_table():
    txt = open(os.path.join(REPO, "include", "irs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("irs_guide_scratch_bytes", "irs_bind_guide"):
        assert re.search(r"\b%s\s*\(" % name, code), name
    for name, value in (("IRS_GUIDE_BINARY", BINARY), ("IRS_GUIDE_FLOAT", FLOAT), ("IRS_MAX_GUIDE_KC", 32),
                        ("IRS_MAX_GUIDE_BITS", 1024), ("IRS_MAX_GUIDE_FLOATS", 512)):
        assert re.search(r"#define %s %d\b" % (name, value), code), name
    sig = _lib.SIGNATURES
    assert sig["irs_guide_scratch_bytes"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32])
    res, args = sig["irs_bind_guide"]
    assert res is ctypes.c_int32 and len(args) == 8 and args[6] is ctypes.c_size_t
    lib = _lib.load()
    assert hasattr(lib, "irs_bind_guide") and hasattr(lib, "irs_guide_scratch_bytes") and lib.irs_abi_version() == 1
    assert (_lib.IRS_MAX_GUIDE_KC, _lib.IRS_MAX_GUIDE_BITS, _lib.IRS_MAX_GUIDE_FLOATS) == (ref.MAX_KC, ref.MAX_BITS, ref.MAX_FLOATS)
    from influentialrs_amd import build
    assert "guide.hip" in build.SOURCES


def test_scratch_bytes_values_and_zeros():
    lib, h = _ctx()
    try:
        f = lib.irs_guide_scratch_bytes
        assert f(None, BINARY, 18) == 0
        for kind, F in ((BINARY, 0), (BINARY, -3), (BINARY, 1025), (0, 18), (3, 18), (FLOAT, 64), (FLOAT, 1), (FLOAT, 513)):
            assert f(h, kind, F) == 0 == ref.scratch_bytes(1000, kind if kind != 0 and kind != 3 else -1, F), (kind, F)
        assert f(h, BINARY, 1) == f(h, BINARY, 32) == 4096 and 1001 * 4 <= 4096 < 1001 * 4 + 256
        assert f(h, BINARY, 33) == 1001 * 8 + (256 - 1001 * 8 % 256) and f(h, BINARY, 1024) == (1001 * 32 * 4 + 255) // 256 * 256
        for F in (1, 18, 32, 33, 64, 65, 1000, 1024):
            assert f(h, BINARY, F) == ref.scratch_bytes(1000, ref.BINARY, F) and f(h, BINARY, F) % 256 == 0
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- refusals, before any launch
def test_bind_refusals_without_a_device():
    p = ctypes.c_void_p
    lib, h = _ctx()
    try:
        f = lib.irs_bind_guide
        big = 1 << 26
        assert f(None, FLOAT, p(4096), 8, 5, None, 0, None) == INVALID
        assert f(h, 0, None, 0, 0, None, 0, None) == 0, "unbinding what was never bound is fine"
        assert f(h, 0, p(4096), 8, 5, None, 0, None) == INVALID and b"kind" in lib.irs_last_error(h)
        assert f(h, 3, p(4096), 8, 5, p(4096), big, None) == INVALID
        for kind in (BINARY, FLOAT):
            assert f(h, kind, p(4096), 0, 5, p(4096), big, None) == INVALID and b"F" in lib.irs_last_error(h)
            assert f(h, kind, p(4096), -1, 5, p(4096), big, None) == INVALID
            assert f(h, kind, p(4096), 8, 0, p(4096), big, None) == INVALID and b"k_c" in lib.irs_last_error(h)
            assert f(h, kind, p(4096), 8, -2, p(4096), big, None) == INVALID
            assert f(h, kind, p(4096), 8, 33, p(4096), big, None) == UNSUPPORTED and b"32" in lib.irs_last_error(h)
        assert f(h, BINARY, p(4096), 1025, 5, p(4096), big, None) == UNSUPPORTED and b"1024" in lib.irs_last_error(h)
        assert f(h, FLOAT, p(4096), 513, 5, None, 0, None) == UNSUPPORTED and b"512" in lib.irs_last_error(h)
        need = lib.irs_guide_scratch_bytes(h, BINARY, 18)
        assert f(h, BINARY, p(4096), 18, 5, p(4096), need - 1, None) == INVALID and b"too small" in lib.irs_last_error(h)
        assert f(h, BINARY, p(4096), 18, 5, None, need, None) == INVALID
        assert f(h, BINARY, p(4096), 18, 5, p(4096), 0, None) == INVALID
        assert f(h, BINARY, p(4096), 18, 5, p(4096 + 8), big, None) == INVALID and b"aligned" in lib.irs_last_error(h)
        assert f(h, FLOAT, p(4096 + 2), 8, 5, None, 0, None) == INVALID and b"aligned" in lib.irs_last_error(h)
        # nothing of the above bound anything: a sampled loop call gets as far as the unbound weights
        assert lib.irs_generate_paths(h, p(4096), p(4096), p(4096), 64, 3, 100, 0, 1, 3, 0, 0, p(4096), p(4096), None) == STATE
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(max_k=20)
    try:
        assert lib.irs_bind_guide(h, FLOAT, p(4096), 8, 21, None, 0, None) == INVALID and b"max_k" in lib.irs_last_error(h)
        assert lib.irs_bind_guide(h, FLOAT, p(4096), 8, 20, None, 0, None) == 0
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        assert lib.irs_bind_guide(h, FLOAT, p(4096), 8, 5, None, 0, None) == UNSUPPORTED
        assert b"whole catalog" in lib.irs_last_error(h)
        assert lib.irs_bind_guide(h, BINARY, p(4096), 18, 5, p(4096), 1 << 26, None) == UNSUPPORTED
        assert lib.irs_bind_guide(h, 0, None, 0, 0, None, 0, None) == 0
    finally:
        lib.irs_destroy(h)


def test_bound_entry_points_refuse_without_a_device():
    """A float guide is kept by pointer and binds without a launch, so the checks of the bound entry points can be reached on a
    context that has no device: each names the binding, and none of them gets as far as the unbound weights."""
    p = ctypes.c_void_p
    a = p(4096)
    lib, h = _ctx()
    try:
        assert lib.irs_bind_guide(h, FLOAT, a, 8, 5, None, 0, None) == 0

        def err():
            return lib.irs_last_error(h)
        assert lib.irs_path_step(h, a, a, 4, a, a, 10, 0, a, 3, 1, 3, 0, a, None) == UNSUPPORTED and b"irs_bind_guide" in err()
        assert lib.irs_path_step(h, a, a, 4, a, a, 4, 0, a, 3, 0, 0, 0, a, None) == INVALID and b"k_c=5" in err()
        assert lib.irs_generate_paths(h, a, a, a, 8, 3, 100, 0, 1, 3, 0, 0, a, a, None) == UNSUPPORTED and b"sample" in err()
        assert lib.irs_generate_paths(h, a, a, a, 8, 3, 4, 0, 0, 0, 0, 1, a, a, None) == INVALID and b"k=4" in err()
        assert lib.irs_generate_paths_until(h, a, a, a, 8, 3, 100, 0, 1, 3, 0, 1, a, a, None, None) == UNSUPPORTED
        assert lib.irs_generate_paths_until(h, a, a, a, 8, 3, 4, 0, 0, 0, 0, 1, a, a, None, None) == INVALID
        assert lib.irs_beam_step(h, a, a, a, a, a, a, a, a, 2, 2, 10, 0, 3, a, a, a, a, a, None) == UNSUPPORTED and b"greedy" in err()
        assert lib.irs_beam_step_until(h, a, a, a, a, a, a, a, a, a, 2, 2, 10, 0, 3, 0, a, a, a, a, a, a, a, None) == UNSUPPORTED
        assert lib.irs_beam_search(h, a, a, a, 2, 2, 3, 100, 0, 0, a, a, None, a, None) == UNSUPPORTED and b"irs_bind_guide" in err()
        assert lib.irs_beam_search_until(h, a, a, a, 2, 2, 3, 100, 0, 0, 1, a, a, None, None, a, None, None) == UNSUPPORTED
        # accepted arguments get as far as the unbound weights, and an unbind restores the unguided checks
        assert lib.irs_generate_paths(h, a, a, a, 8, 3, 100, 0, 0, 0, 0, 0, a, a, None) == STATE
        assert lib.irs_bind_guide(h, 0, None, 0, 0, None, 0, None) == 0
        assert lib.irs_generate_paths(h, a, a, a, 8, 3, 4, 0, 1, 3, 0, 0, a, a, None) == STATE
        assert lib.irs_beam_search(h, a, a, a, 2, 2, 3, 100, 0, 0, a, a, None, a, None) == STATE
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- Python layers
def test_keywords_are_off_by_default_and_keyword_only():
    for fn in (Engine.generate_paths, Engine.generate_paths_until):
        par = inspect.signature(fn).parameters
        assert par["guide"].default is None and par["guide_k"].default == 5, fn
    for fn in (Engine.beam_search, Engine.beam_search_until, Engine.generate_paths_sharded):
        assert "guide" not in inspect.signature(fn).parameters, fn
    for name in ("guide_scratch_bytes", "bind_guide", "unbind_guide", "_search_options"):
        assert hasattr(Engine, name), name
    sig = inspect.signature(IRSNN.get_seq_in_batch, follow_wrapped=False).parameters
    for name, default in (("guide", None), ("guide_k", 5)):
        assert sig[name].default == default and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(IRSNN.get_seq_in_batch).parameters)[-1] == "beam_stop"
    par = inspect.signature(Rec2Inf.get_seq_in_batch).parameters
    assert list(par) == ["self", "seqs", "targets", "guide", "guide_k", "max_path_len", "stop_at_target", "exclude", "no_repeat",
                         "exact_candidates", "trace"]
    assert (par["guide_k"].default, par["max_path_len"].default, par["stop_at_target"].default) == (5, 20, True)


def test_irn_front_end_refuses_without_a_device():
    cfg = synth.make_config("tiny")
    irn = IRSNN(cfg, InfluentialNet(cfg), "cpu")
    B, L = 2, cfg.max_len
    seqs, users, targets = torch.ones((B, L), dtype=torch.int64), torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.int64)
    table = torch.zeros((cfg.n_item + 1, 4))
    with pytest.raises(ValueError, match="guide is not built for beam search.*beam_width=1"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, beam_width=4, guide=table)
    with pytest.raises(ValueError, match="guide is not built for the sampled search.*sample=False"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, sample=True, guide=table)
    with pytest.raises(ValueError, match="guide_k=33"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, guide=table, guide_k=33)
    assert irn._guide is None and irn._guide_k == 5, "the switches last for the call"
    net = InfluentialNet(cfg)
    net.shard_items(0, 2, drop_full=False)
    irn = IRSNN(cfg, net, "cpu")
    with pytest.raises(ValueError, match="guide is not built for an item-sharded catalog"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, guide=table)


def test_rec2inf_front_end_without_a_device():
    cfg = synth.make_config("eval_tiny")
    r2i = Rec2Inf(cfg, SampleNet(cfg), "cpu")
    table = torch.zeros((cfg.n_item + 1, 4))
    hist, targets = [np.array([3, 4, 5]), np.array([], dtype=np.int64)], torch.tensor([9, 8])
    with pytest.raises(ValueError, match="empty history"):
        r2i.get_seq_in_batch(hist, targets, table)
    with pytest.raises(ValueError, match="needs a guide"):
        r2i.get_seq_in_batch(hist[:1], targets[:1], None)
    with pytest.raises(ValueError, match="guide_k=0"):
        r2i.get_seq_in_batch(hist[:1], targets[:1], table, guide_k=0)
    net = SampleNet(cfg)
    net.shard_items(0, 2, drop_full=False)
    with pytest.raises(ValueError, match="item-sharded"):
        Rec2Inf(cfg, net, "cpu").get_seq_in_batch(hist[:1], targets[:1], table)
    # the window layout: the last L - 1 items left-aligned, zeros, the target in slot L - 1, hep = n - 1
    L = 6
    win, hep, histories = rec2inf_windows([np.array([3, 4]), np.arange(1, 10), torch.tensor([7])], torch.tensor([9, 20, 1]), L, "cpu")
    assert win.tolist() == [[3, 4, 0, 0, 0, 9], [5, 6, 7, 8, 9, 20], [7, 0, 0, 0, 0, 1]] and hep.tolist() == [1, 4, 0]
    assert hep.dtype == torch.int32 and win.dtype == torch.int64 and [len(h) for h in histories] == [2, 9, 1]
    win2, hep2, _ = rec2inf_windows(torch.tensor([[3, 4, 0], [0, 2, 0]]), [9, 8], L, "cpu")
    assert win2.tolist() == [[3, 4, 0, 0, 0, 9], [2, 0, 0, 0, 0, 8]] and hep2.tolist() == [1, 0]
    with pytest.raises(ValueError, match="histories for"):
        rec2inf_windows([np.array([1])], [1, 2], L, "cpu")
