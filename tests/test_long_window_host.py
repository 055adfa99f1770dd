"""not-gpu: long windows (max_len above 256) at the C ABI and in the CPU statements the GPU tests compare against.

irs_create keeps its contract ([2, 256]); irs_create_ex with IRS_CREATE_LONG_WINDOWS admits [2, IRS_MAX_LEN_LONG = 1024]; flags == 0
is irs_create; an unknown flag bit is an argument error with a message.  The workspace of a long context is no smaller than that of
the same dims at 256 tokens.  tests/path_ref.py and oracle_np.decode -- the references of test_gpu_long_window_*.py -- run at
L = 320 (nothing in them is sized by the old limit)."""
import ctypes
import os
import re

import numpy as np

import path_ref
from influentialrs_amd import _lib, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(n_item=1000, n_user=10, d=64, max_len=50, n_heads=4, ffn_dim=256, n_layers=6, u_dim=10, mask_mode=0, max_rows=8,
            max_k=100, max_seqs=0)


def _create(max_len, flags=None, **over):
    """-> (return code, handle); flags None: irs_create."""
    lib = _lib.load()
    h = ctypes.c_void_p()
    dims = _lib.IrsDims(**dict(BASE, max_len=max_len, **over))
    if flags is None:
        rc = lib.irs_create(ctypes.byref(h), ctypes.byref(dims), None)
    else:
        rc = lib.irs_create_ex(ctypes.byref(h), ctypes.byref(dims), None, flags)
    return rc, h


def test_header_and_ctypes_agree_on_the_flag_and_the_bound():
    txt = open(os.path.join(REPO, "include", "irs_hip.h")).read()
    assert int(re.search(r"#define IRS_CREATE_LONG_WINDOWS (\d+)u", txt).group(1)) == _lib.IRS_CREATE_LONG_WINDOWS == 1
    assert int(re.search(r"#define IRS_MAX_LEN_LONG (\d+)", txt).group(1)) == _lib.IRS_MAX_LEN_LONG == 1024
    assert _lib.load().irs_abi_version() == 1


def test_irs_create_keeps_its_limit_and_flags_zero_is_irs_create():
    lib = _lib.load()
    for flags in (None, 0):
        for L in (257, 300):
            rc, _ = _create(L, flags)
            assert rc == -1, (flags, L)
            assert b"[2, 256]" in lib.irs_last_error(None)
        for L in (2, 256):
            rc, h = _create(L, flags)
            assert rc == 0, (flags, L, lib.irs_last_error(None))
            lib.irs_destroy(h)
        assert _create(1, flags)[0] == -1


def test_long_windows_flag_opens_257_to_1024():
    lib = _lib.load()
    for L in (2, 256, 257, 300, 1024):
        rc, h = _create(L, _lib.IRS_CREATE_LONG_WINDOWS)
        assert rc == 0, (L, lib.irs_last_error(None))
        assert lib.irs_workspace_bytes(h) > 0 and lib.irs_derived_bytes(h) > 0
        lib.irs_destroy(h)
    rc, _ = _create(1025, _lib.IRS_CREATE_LONG_WINDOWS)
    assert rc == -1 and b"[2, 1024]" in lib.irs_last_error(None)
    # every other check is unchanged under the flag
    for bad in (dict(d=63), dict(n_heads=3), dict(max_k=0), dict(n_item=0)):
        assert _create(300, _lib.IRS_CREATE_LONG_WINDOWS, **bad)[0] == -1, bad


def test_unknown_flag_bit_is_refused_with_a_message():
    lib = _lib.load()
    for flags in (2, 3, 0x80000000):
        rc, _ = _create(50, flags)
        assert rc == -1, flags
        assert b"flag" in lib.irs_last_error(None)


def test_workspace_of_a_long_context_is_no_smaller():
    lib = _lib.load()
    for over in (dict(), dict(d=128, ffn_dim=256, n_heads=4, max_rows=64), dict(d=256, max_rows=40, max_seqs=16)):
        rc, h256 = _create(256, None, **over)
        assert rc == 0
        rc, h320 = _create(320, _lib.IRS_CREATE_LONG_WINDOWS, **over)
        assert rc == 0
        rc, h256x = _create(256, _lib.IRS_CREATE_LONG_WINDOWS, **over)
        assert rc == 0
        try:
            assert lib.irs_workspace_bytes(h320) >= lib.irs_workspace_bytes(h256), over
            assert lib.irs_workspace_bytes(h256x) == lib.irs_workspace_bytes(h256), over  # the flag alone changes nothing
            assert lib.irs_derived_bytes(h256x) == lib.irs_derived_bytes(h256), over
        finally:
            for h in (h256, h320, h256x):
                lib.irs_destroy(h)


def test_path_ref_runs_at_320():
    """A window whose leading candidates sit in slots 256 and above: the first survivor is the candidate behind them."""
    L, k = 320, 100
    g = np.random.default_rng(5)
    ids0 = g.permutation(5000)[:k].astype(np.int64)[None]
    val = np.sort(g.random(k).astype(np.float32))[::-1][None].copy()
    seq = g.integers(6001, 9000, size=(1, L)).astype(np.int64)
    seq[0, 256:256 + 40] = ids0[0, :40] + 1
    for hep, grown in ((L - 3, True), (L - 2, False)):
        got = path_ref.path_step(seq, np.array([hep], np.int32), val, ids0, 0, np.zeros((1, 4), np.float32), np.zeros(1, np.int32))
        g_seq, g_hep, g_paths, g_st = got
        assert g_paths[0, 0] == ids0[0, 40] + 1 and g_st[0] == 0
        assert g_hep[0] == (hep + 1 if grown else hep) and g_seq[0, L - 2] == ids0[0, 40] + 1
    state = (seq[None], np.array([[L - 2]], np.int32), np.zeros((1, 1)), np.zeros((1, 1, 4), np.float32))
    (s_o, h_o, c_o, p_o), st = path_ref.beam_step(state, val, ids0, None, None, 0, 4)
    assert p_o[0, 0, 0] == ids0[0, 40] + 1 and st[0] == 0
    items = np.arange(1, 401, dtype=np.int64)
    b_seq, label, raw, raw_n = path_ref.build_eval_batch(items, np.array([0, 400]), L, 350, 20, np.array([7]))
    assert b_seq[0, L - 1] == 7 and label[0] == 400 and raw_n[0] == 350 and (b_seq[0, L - 21:L - 1] == 0).all()
    assert np.array_equal(b_seq[0, :L - 21], items[399 - (L - 21):399])


def test_oracle_decodes_at_320(oracle):
    cfg = synth.make_config("tiny", max_len=320)
    sd = synth.irn_state_dict(cfg, 2027)
    g = np.random.default_rng(9)
    seq = np.zeros(320, dtype=np.int64)
    seq[320 - 290:] = g.integers(1, cfg.n_item + 1, size=290)
    o32 = oracle.decode(sd, cfg, seq, 3)[0]
    o64 = oracle.decode(sd, cfg, seq, 3, dtype=np.float64)[0]
    assert o32.shape == (320, cfg.emb_dim) and np.isfinite(o64).all()
    assert np.abs(o32 - o64).max() < 2e-5
