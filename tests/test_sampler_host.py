"""not-gpu: the bound sampler (irs_bind_sampler): the integer RNG, the properties of the numpy statement (tests/sampler_ref.py),
the derived tolerance TOL confirmed on a float32 emulation of the stated expressions, every refusal of the binding and of the bound
entry points on a context created without a device, and the ValueErrors of the front end."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import path_ref
import sampler_ref as ref
from influentialrs_amd import _lib, synth
from influentialrs_amd.engine import Engine, Sampler
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet, SearchOptions, search_option_kwargs
from influentialrs_amd.model.rec2inf import Rec2Inf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE, UNSUPPORTED = -1, -2, -4
NINF = np.float32(-np.inf)


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


# ---------------------------------------------------------------- the RNG
def test_draws_are_24_bit_uniform_and_keyed_by_row_and_step():
    """u over rows 0 .. 255 x steps 0 .. 63 (16384 draws) per seed: every u is k * 2^-24 with 0 <= k < 2^24, so u is exact in
    float32 and in [0, 1).  Chi-square over 64 equal bins, 63 degrees of freedom; the bound is the 99.9 % point, 103.4.
    Recorded: seed 1: 60.8, seed 12345: 81.5, seed 2^63 + 7: 74.7."""
    for seed in (1, 12345, (1 << 63) + 7):
        bits = np.array([[ref.draw_bits(seed, r, s) for s in range(64)] for r in range(256)], dtype=np.int64)
        assert bits.min() >= 0 and bits.max() < (1 << 24)
        u = np.array([[ref.draw(seed, r, s) for s in range(64)] for r in range(256)])
        assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
        assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, bits.astype(np.float64)), "u is the 24 bits, exactly"
        counts = np.bincount((bits >> 18).reshape(-1), minlength=64)
        expected = bits.size / 64
        chi2 = float(((counts - expected) ** 2 / expected).sum())
        print(f"seed {seed}: chi-square {chi2:.1f}")
        assert chi2 < 103.4, (seed, chi2)
        assert len(np.unique(bits)) > 0.99 * bits.size, "rows and steps draw apart"
    # the stock sampled step's expression with the caller's row: the same integer for the same (seed, row, step)
    z = (5 + 0x9E3779B97F4A7C15 * (3 * 1315423911 + 2 + 1)) & ref.MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & ref.MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & ref.MASK
    assert ref.draw_bits(5, 3, 2) == ((z ^ (z >> 31)) >> 40) & 0xFFFFFF


# ---------------------------------------------------------------- the statement
def _case(g, M, L, k, n_item=600):
    ids0 = np.stack([g.permutation(n_item)[:k] for _ in range(M)]).astype(np.int64)
    val = -np.sort(-(g.standard_normal((M, k)) * 2).astype(np.float32), axis=1)
    seq = g.integers(1, n_item + 1, size=(M, L)).astype(np.int64)
    hep = g.integers(0, L - 1, size=M).astype(np.int32)
    return seq, hep, val, ids0


def test_reference_properties():
    g = np.random.default_rng(3)
    M, L, k = 40, 10, 50
    seq, hep, val, ids0 = _case(g, M, L, k)
    status = np.zeros(M, dtype=np.int32)
    greedy = path_ref.path_step(seq, hep, val, ids0, 0, np.zeros((M, 4), dtype=np.float32), status)

    def chosen(top_k, T, p, seed=9, step=0):
        v, i, rec = ref.choose(seq, hep, val, ids0, top_k, T, p, step, seed)
        assert (i[rec["written"], 1] == -1).all() and (v[rec["written"], 1] == NINF).all()
        assert np.array_equal(i[:, 2:], ids0[:, 2:]), "only entries 0 and 1 are written"
        return i[:, 0] + 1, rec
    # T -> 0 picks candidate 0; top_k = 1 is greedy; a small top_p gives support 1
    for items, rec in (chosen(8, 1e-4, 1.0), chosen(1, 1.0, 1.0), chosen(8, 1.0, 1e-6)):
        assert np.array_equal(items.astype(np.float32), greedy[2][:, 0]) and (rec["index"] == 0).all()
    assert (chosen(8, 1.0, 1e-6)[1]["support"] == 1).all() and (chosen(1, 1.0, 1.0)[1]["lq"] == 0).all()
    # top_p = 1, T = 1, top_k <= 8: the weights of the stock sampled step (softmax of the survivors' scores)
    for top_k in (3, 8):
        dists = path_ref.path_step(seq, hep, val, ids0, 0, np.zeros((M, 4), dtype=np.float32), status, sample=True, sample_k=top_k)
        _, _, rec = ref.choose(seq, hep, val, ids0, top_k, 1.0, 1.0, 0, 9)
        for r in range(M):
            kept = rec["kept"][r]
            assert [int(ids0[r, c]) + 1 for _, c in kept] == dists[r][0].tolist()
            w = ref.weights64(np.array([v for v, _ in kept], dtype=np.float32), 1.0)
            assert np.allclose(w / w.sum(), dists[r][1], rtol=1e-12, atol=0)
            assert rec["support"][r] == len(kept) and np.isclose(rec["lq"][r], np.log(dists[r][1][rec["index"][r]]), rtol=1e-9, atol=1e-12)
    # the draw decides: seeds and steps move the choice, the record says which candidate and how probable it was
    a, ra = chosen(8, 2.0, 0.9, seed=1)
    b, _ = chosen(8, 2.0, 0.9, seed=2)
    c, _ = chosen(8, 2.0, 0.9, seed=1, step=1)
    assert (a != b).any() and (a != c).any() and (ra["index"] > 0).any() and (ra["lq"] < 0).all()
    assert (ra["support"] >= 1).all() and (ra["support"] <= 8).all() and (ra["index"] < ra["support"]).all()
    # a row key: the draw of row r under row_ids is the draw of the row it names
    ids = g.permutation(M).astype(np.int32)
    _, _, rk = ref.choose(seq, hep, val, ids0, 8, 2.0, 0.9, 0, 1, row_ids=ids)
    assert np.array_equal(rk["u"], np.array([ref.draw(1, int(ids[r]), 0) for r in range(M)]))
    # -inf in the tail weighs nothing; a first value that is not finite takes candidate 0
    v2 = val.copy()
    v2[:, 5:] = NINF
    _, _, r2 = ref.choose(np.zeros_like(seq), np.full(M, -1, dtype=np.int32), v2, ids0, 8, 1.0, 1.0, 0, 4)
    assert (r2["index"] < 5).all() and (r2["support"] <= 5).all()
    v2[:, 0] = NINF
    _, i3, r3 = ref.choose(np.zeros_like(seq), np.full(M, -1, dtype=np.int32), v2, ids0, 8, 1.0, 1.0, 0, 4)
    assert (r3["index"] == 0).all() and (r3["lq"] == 0).all() and (r3["support"] == 1).all() and np.array_equal(i3[:, 0], ids0[:, 0])
    # rows that are not written: finished, offered (the offer's list), without a candidate
    fin = (np.arange(M) % 4 == 1).astype(np.int32)
    st = np.where(np.arange(M) % 4 == 2, ref.OFFERED, 0).astype(np.int32)
    i4, v4 = ids0.copy(), val.copy()
    off = st != 0
    i4[off, 0], i4[off, 1] = seq[off, -1] - 1, -1
    hid = np.arange(M) % 4 == 3
    s4, h4 = seq.copy(), hep.copy()
    i4[hid, 1] = -1
    s4[hid, 0], h4[hid] = i4[hid, 0] + 1, 0
    v5, i5, r5 = ref.choose(s4, h4, v4, i4, 8, 1.0, 1.0, 2, 4, status=st, fin=fin)
    for rows in (fin != 0, off, hid):
        assert not r5["written"][rows].any() and np.array_equal(i5[rows], i4[rows]) and np.array_equal(v5[rows].view(np.uint32), v4[rows].view(np.uint32))
    assert (r5["support"][off] == 1).all() and (r5["u"][off] == 0).all() and (r5["support"][hid] == 0).all()
    assert not r5["recorded"][fin != 0].any() and r5["recorded"][fin == 0].all()


# ---------------------------------------------------------------- the tolerance
@pytest.mark.parametrize("order", ["serial", "pairwise"])
def test_tol_holds_on_the_float32_emulation(order):
    """TOL (sampler_ref.TOL = 5e-5, derived there) bounds the gap between a float32 cumulative bound S_m / S_m* and the float64
    one.  Confirmed here on the float32 emulation of the stated expressions, n in {1, 2, 64, 65, 256}, temperatures 0.05, 1 and 4,
    top_p 0.1, 0.9 and 1, values whose arguments reach 20 in magnitude, 40 rows each.  Largest gap seen: serial 1.34e-6, pairwise
    3.36e-7 (both far below the derived 3.6e-5: rounding errors of a sum do not line up)."""
    g = np.random.default_rng(11)
    worst = 0.0
    for n in (1, 2, 64, 65, 256):
        for T in (0.05, 1.0, 4.0):
            inv_t = np.float32(1.0) / np.float32(T)
            for p in (0.1, 0.9, 1.0):
                for _ in range(40):
                    v = -np.sort(-(g.random(n) * min(20.0 * T, 12.0)).astype(np.float32))
                    if n > 2 and g.random() < 0.3:
                        v[1] = v[0]  # a tie at the head
                    u = np.float32(g.integers(0, 1 << 24) * 2.0 ** -24)
                    e = ref.emulate32(v, inv_t, p, u, order)
                    c = ref.choose64(v, inv_t, p, u)
                    S64 = np.cumsum(ref.weights64(v, inv_t))
                    m = e["support"]  # both normalised by their own S at the emulation's support
                    gap = np.abs(e["S"][:m].astype(np.float64) / float(e["S"][m - 1]) - S64[:m] / S64[m - 1]).max()
                    gap = max(gap, np.abs(e["S"].astype(np.float64) / float(e["S"][-1]) - c["frac"]).max())
                    worst = max(worst, float(gap))
                    if c["near_u"] > ref.TOL and c["near_p"] > ref.TOL:
                        assert e["index"] == c["index"] and e["support"] == c["support"], (n, T, p)
                        if np.isfinite(c["lq"]) and c["lq"] > -20:
                            assert abs(float(e["lq"]) - c["lq"]) <= 2 * ref.TOL * max(1.0, abs(c["lq"])), (n, T, p, e["lq"], c["lq"])
    print(f"{order}: largest gap {worst:.3g}, TOL {ref.TOL:.3g}")
    assert worst <= ref.TOL


# ---------------------------------------------------------------- header, library, table, build
def test_new_symbols_in_header_library_table_and_build():
    txt = open(os.path.join(REPO, "include", "irs_hip.h")).read()
    assert re.search(r"#define IRS_MAX_SAMPLER_K 256\b", txt) and _lib.IRS_MAX_SAMPLER_K == ref.MAX_SAMPLER_K == 256
    lib = _lib.load()
    for name in ("irs_bind_sampler", "irs_sampler_choose"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(r"\bint %s\(" % name, txt), name
    assert lib.irs_abi_version() == 1
    from influentialrs_amd import build
    assert "sampler.hip" in build.SOURCES


# ---------------------------------------------------------------- refusals, before any launch
def test_bind_refusals_without_a_device():
    p = ctypes.c_void_p
    a = p(4096)
    lib, h = _ctx()
    try:
        f = lib.irs_bind_sampler

        def err():
            return lib.irs_last_error(h)
        assert f(None, 3, 1.0, 1.0, None, None, None, 0, 0) == INVALID
        assert f(h, 0, 1.0, 1.0, None, None, None, 0, 0) == 0, "unbinding what was never bound is fine"
        for T in (0.0, -1.0, float("inf"), float("nan")):
            assert f(h, 3, T, 1.0, None, None, None, 0, 0) == INVALID and b"irs_bind_sampler" in err() and b"temperature" in err(), T
        for tp in (0.0, -0.5, 1.0001, float("nan")):
            assert f(h, 3, 1.0, tp, None, None, None, 0, 0) == INVALID and b"top_p" in err(), tp
        for top_k in (-1, 101, 257):
            assert f(h, top_k, 1.0, 1.0, None, None, None, 0, 0) == UNSUPPORTED and b"top_k" in err(), top_k
        assert f(h, 3, 1.0, 1.0, a, None, None, 0, 4) == INVALID and f(h, 3, 1.0, 1.0, None, None, a, 8, 0) == INVALID
        # nothing of the above bound anything: a sampled loop call gets as far as the unbound weights
        assert lib.irs_generate_paths(h, a, a, a, 8, 3, 100, 0, 1, 3, 0, 0, a, a, None) == STATE
        # one choice rule at a time, both ways round, guide and lookahead
        assert f(h, 100, 0.5, 0.9, None, a, None, 8, 4) == 0
        assert lib.irs_bind_guide(h, _lib.IRS_GUIDE_FLOAT, a, 8, 5, None, 0, None) == UNSUPPORTED and b"irs_bind_sampler" in err()
        need = lib.irs_lookahead_scratch_bytes(h, 8, 3)
        assert lib.irs_bind_lookahead(h, 3, a, need, None, None, 8, 4) == UNSUPPORTED and b"irs_bind_sampler" in err()
        assert f(h, 0, 0.0, 0.0, None, None, None, 0, 0) == 0, "an unbind looks at top_k alone"
        assert lib.irs_bind_guide(h, _lib.IRS_GUIDE_FLOAT, a, 8, 5, None, 0, None) == 0
        assert f(h, 3, 1.0, 1.0, None, None, None, 0, 0) == UNSUPPORTED and b"irs_bind_guide" in err() and b"irs_bind_sampler" in err()
        assert lib.irs_bind_guide(h, 0, None, 0, 0, None, 0, None) == 0
        assert lib.irs_bind_lookahead(h, 3, a, need, None, None, 8, 4) == 0
        assert f(h, 3, 1.0, 1.0, None, None, None, 0, 0) == UNSUPPORTED and b"irs_bind_lookahead" in err()
        assert lib.irs_bind_lookahead(h, 0, None, 0, None, None, 0, 0) == 0
        assert f(h, 3, 1.0, 1.0, None, None, None, 0, 0) == 0 and f(h, 0, 1.0, 1.0, None, None, None, 0, 0) == 0
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        assert lib.irs_bind_sampler(h, 3, 1.0, 1.0, None, None, None, 0, 0) == UNSUPPORTED
        assert b"irs_bind_sampler" in lib.irs_last_error(h) and b"whole catalog" in lib.irs_last_error(h)
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(max_k=300)
    try:
        assert lib.irs_bind_sampler(h, 257, 1.0, 1.0, None, None, None, 0, 0) == UNSUPPORTED and b"256" in lib.irs_last_error(h)
        assert lib.irs_bind_sampler(h, 256, 1.0, 1.0, None, None, None, 0, 0) == 0
    finally:
        lib.irs_destroy(h)


def test_bound_entry_points_refuse_without_a_device():
    """The binding launches nothing, so the checks of the bound entry points can be reached on a context that has no device: each
    names the binding, and none of them gets as far as the unbound weights."""
    p = ctypes.c_void_p
    a, big = p(4096), 1 << 30
    lib, h = _ctx()
    try:
        assert lib.irs_bind_sampler(h, 5, 0.7, 0.9, a, a, a, 16, 4) == 0

        def err():
            return lib.irs_last_error(h)
        gp, gu = lib.irs_generate_paths, lib.irs_generate_paths_until
        assert gp(h, a, a, a, 8, 3, 100, 0, 1, 3, 0, 0, a, a, None) == INVALID and b"two samplers" in err() and b"irs_generate_paths" in err()
        assert gu(h, a, a, a, 8, 3, 100, 0, 1, 3, 0, 1, a, a, None, None) == INVALID and b"two samplers" in err() and b"irs_generate_paths_until" in err()
        assert gp(h, a, a, a, 8, 3, 4, 0, 0, 0, 0, 1, a, a, None) == INVALID and b"k=4 < top_k=5" in err()
        assert gp(h, a, a, a, 17, 3, 100, 0, 0, 0, 0, 0, a, a, None) == INVALID and b"[16, 4]" in err()
        assert gp(h, a, a, a, 8, 5, 100, 0, 0, 0, 0, 0, a, a, None) == INVALID and b"[16, 4]" in err()
        assert lib.irs_beam_step(h, a, a, a, a, a, a, a, a, 2, 2, 10, 0, 3, a, a, a, a, a, None) == UNSUPPORTED and b"irs_bind_sampler" in err()
        assert lib.irs_beam_step_until(h, a, a, a, a, a, a, a, a, a, 2, 2, 10, 0, 3, 0, a, a, a, a, a, a, a, None) == UNSUPPORTED
        assert b"irs_bind_sampler" in err()
        assert lib.irs_beam_search(h, a, a, a, 2, 2, 3, 100, 0, 0, a, a, None, a, None) == UNSUPPORTED and b"greedy loops only" in err()
        assert lib.irs_beam_search_until(h, a, a, a, 2, 2, 3, 100, 0, 0, 1, a, a, None, None, a, None, None) == UNSUPPORTED
        assert b"irs_bind_sampler" in err()
        # accepted arguments get as far as the unbound weights; irs_path_step alone is unchanged (it launches: not called here)
        assert gp(h, a, a, a, 8, 3, 100, 0, 0, 0, 77, 0, a, a, None) == STATE
        # top_k > 32 with a bound survivor scratch
        assert lib.irs_bind_sampler(h, 33, 1.0, 1.0, None, None, None, 0, 0) == 0
        assert lib.irs_bind_survivor_scratch(h, a, big) == 0
        assert gp(h, a, a, a, 8, 9, 100, 0, 0, 0, 0, 0, a, a, None) == UNSUPPORTED and b"32" in err() and b"irs_bind_survivor_scratch" in err()
        assert lib.irs_bind_sampler(h, 32, 1.0, 1.0, None, None, None, 0, 0) == 0
        assert gp(h, a, a, a, 8, 9, 100, 0, 0, 0, 0, 0, a, a, None) == STATE, "without a record the path length is free"
        assert lib.irs_bind_survivor_scratch(h, None, 0) == 0
        # the kernel alone
        sc = lib.irs_sampler_choose
        ok = (a, a, 4, a, a, 40, 0, 5, None, a, None, None, 0)
        for at in (0, 1, 3, 4, 9):
            bad = list(ok)
            bad[at] = None
            assert sc(h, *bad) == INVALID and b"irs_sampler_choose" in err(), at
        assert sc(h, a, a, 0, a, a, 40, 0, 5, None, a, None, None, 0) == INVALID
        assert sc(h, a, a, 4, a, a, 31, 0, 5, None, a, None, None, 0) == INVALID and b"top_k=32" in err()
        assert sc(h, a, a, 4, a, a, 101, 0, 5, None, a, None, None, 0) == INVALID
        assert sc(h, a, a, 4, a, a, 40, -1, 5, None, a, None, None, 0) == INVALID and b"step" in err()
        assert sc(h, a, a, 4, a, a, 40, 5, 5, None, a, None, a, 4) == INVALID and b"step" in err()
        # and an unbind restores the unbound checks
        assert lib.irs_bind_sampler(h, 0, 1.0, 1.0, None, None, None, 0, 0) == 0
        assert sc(h, *ok) == STATE and b"no sampler is bound" in err()
        assert gp(h, a, a, a, 8, 3, 4, 0, 1, 3, 0, 0, a, a, None) == STATE
        assert lib.irs_beam_search(h, a, a, a, 2, 2, 3, 100, 0, 0, a, a, None, a, None) == STATE
    finally:
        lib.irs_destroy(h)


# ---------------------------------------------------------------- Python layers
def test_keywords_are_off_by_default_and_keyword_only():
    for fn in (Engine.generate_paths, Engine.generate_paths_until):
        assert inspect.signature(fn).parameters["sampler"].default is None, fn
    for fn in (Engine.beam_search, Engine.beam_search_until, Engine.generate_paths_sharded):
        assert "sampler" not in inspect.signature(fn).parameters, fn
    for name in ("bind_sampler", "unbind_sampler", "sampler_choose"):
        assert hasattr(Engine, name), name
    s = Sampler(5)
    assert (s.top_k, s.temperature, s.top_p, s.record) == (5, 1.0, 1.0, False)
    with pytest.raises(Exception):
        s.top_k = 6  # frozen
    sig = inspect.signature(IRSNN.get_seq_in_batch, follow_wrapped=False).parameters
    for name, default in (("temperature", None), ("top_p", None), ("draw_k", None), ("draw_record", False)):
        assert sig[name].default is default and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
    declared = list(inspect.signature(IRSNN.get_seq_in_batch).parameters)
    assert declared == ["self", "seqs", "users", "targets", "max_path_len", "gap_len", "sample", "sample_k", "beam_width", "stop_at_target",
                        "beam_stop"], "the positional signature is unchanged"
    # any of the three binds the sampler, the others at their defaults
    for kw, want in ((dict(temperature=0.5), Sampler(3, 0.5, 1.0)), (dict(top_p=0.8), Sampler(3, 1.0, 0.8)),
                     (dict(draw_k=40), Sampler(40, 1.0, 1.0)), (dict(draw_k=7, temperature=2, draw_record=True), Sampler(7, 2.0, 1.0, True))):
        assert search_option_kwargs(SearchOptions(**kw), 1, False, 1)["sampler"] == want, kw
    assert "sampler" not in search_option_kwargs(SearchOptions(), 1, False, 1)


def test_front_ends_refuse_without_a_device():
    cfg = synth.make_config("tiny")
    irn = IRSNN(cfg, InfluentialNet(cfg), "cpu")
    B, L = 2, cfg.max_len
    seqs, users, targets = torch.ones((B, L), dtype=torch.int64), torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.int64)
    table = torch.zeros((cfg.n_item + 1, 4))

    def call(**kw):
        return irn.get_seq_in_batch(seqs, users, targets, 5, 0, **kw)
    for kw in (dict(temperature=0.7), dict(top_p=0.9), dict(draw_k=5)):
        with pytest.raises(ValueError, match="two samplers.*sample=False"):
            call(sample=True, **kw)
        with pytest.raises(ValueError, match="temperature / top_p / draw_k and guide"):
            call(guide=table, **kw)
        with pytest.raises(ValueError, match="temperature / top_p / draw_k and lookahead"):
            call(lookahead=3, **kw)
        with pytest.raises(ValueError, match="is not built for beam search.*beam_width=1"):
            call(beam_width=4, **kw)
    for bad in (0, -1.0, float("inf"), float("nan"), True):
        with pytest.raises(ValueError, match="temperature=.*finite and above 0"):
            call(temperature=bad)
    for bad in (0, -0.1, 1.5, float("nan"), True):
        with pytest.raises(ValueError, match=r"top_p=.*in \(0, 1\]"):
            call(top_p=bad)
    for bad in (0, 101, 2.0, "3", True):
        with pytest.raises(ValueError, match="draw_k=.*an int from 1 to 100"):
            call(draw_k=bad)
    with pytest.raises(ValueError, match="draw_k=33 with exact_candidates=True"):
        call(draw_k=33, exact_candidates=True)
    with pytest.raises(ValueError, match="draw_record=True needs the sampler"):
        call(draw_record=True)
    assert irn._temperature is None and irn._top_p is None and irn._draw_k is None and irn._draw_record is False, "the switches last for the call"
    net = InfluentialNet(cfg)
    net.shard_items(0, 2, drop_full=False)
    sharded = IRSNN(cfg, net, "cpu")
    with pytest.raises(ValueError, match="temperature / top_p / draw_k is not built for an item-sharded catalog"):
        sharded.get_seq_in_batch(seqs, users, targets, 5, 0, temperature=0.5)
    # Rec2Inf always binds a guide: the sampler's keywords are refused in the same words
    sig = inspect.signature(Rec2Inf.get_seq_in_batch.__wrapped__.__wrapped__, follow_wrapped=False).parameters
    for name in ("temperature", "top_p", "draw_k"):
        assert sig[name].default is None and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
    r2i = Rec2Inf.__new__(Rec2Inf)
    torch.nn.Module.__init__(r2i)
    for kw in (dict(temperature=0.7), dict(top_p=0.9), dict(draw_k=5)):
        with pytest.raises(ValueError, match="temperature / top_p / draw_k and guide"):
            r2i.get_seq_in_batch([[1, 2]], [3], table, **kw)
