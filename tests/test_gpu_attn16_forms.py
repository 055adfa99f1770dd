"""k_attn16<16, FAST, PLANES>: the four instantiations of the packed head-dim-32 attention (float32 V rows or float16 V planes,
packed rows-only or whole-window decode) and the few-sequences launch of the float32 form, on one batch built for the
statements the forms share.

The route matrix (test_gpu_decoder_routes.py) draws its window lengths at random and holds no IRN window without a target item
(seq[b][L - 1] == 0) on the two-kernel path; one mask statement serves every form.  Here: c2 at max_len = 48 (three 16-key
tiles, two 32-key mask words), 700 windows (33600 rows: above the 16-token layer kernels, the fragment-major fused route) whose
packed lengths cycle through 1, 2, 15, 16, 17, 31, 32, 33, 47, 48; every fifth window has target id 0; every seventh is consumed
on a pad -- inside the history where it is long enough (in the last key tile: only ever a diagonal tile; in an earlier one:
below the diagonal of the later query blocks), else in front of it; the first and last user ids occur.

Two engines: the default (V planes) and IRS_ATTN_GEMM=f32, both with the sequence-resident decoder off.  Rows against
oracle_np on the same state dict at test_gpu_decoder_path.py's X_TOL / X_TOL_X6 (on the first SAMPLE windows -- every length x pad
phase x target phase -- and the last ones: the oracle takes 17 ms per window), the two engines against each other at X_TOL_X6
over the whole batch, and no NaN row except where the oracle's row is NaN.

The oracle and windows without a target item (checked below, no GPU needed): like the reference it masks the window's last
COLUMN, so every pad row IN FRONT of the history sees no key at all, is NaN after the first layer and -- 0 x NaN -- takes the
whole window with it after the second.  Only a window whose history fills every column in front of the empty target column
(length 48 here: 47 items) has finite oracle rows; the packed kernels hold no such pad rows and stay finite, which is why the NaN
rule is one-sided and why the shorter no-target windows are held by the comparison of the two engines alone."""
import os

import numpy as np
import pytest
import torch

from influentialrs_amd import synth
from test_gpu_decoder_path import X_TOL, X_TOL_X6

B = 700
LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48]
SAMPLE = 100  # 50 = the period of (length, target phase); 7 = the pad phase: every pad phase of every length, each target phase twice
SEED = 20261021


def _config():
    return synth.make_config("c2", max_len=48, n_layers=2)


def _no_target(b):
    return b % 5 == (b // len(LENGTHS)) % 5  # every fifth window, walking through the lengths


def _batch(cfg):
    """seqs [B, L], users [B], pos [B], pad_tile [B] (key tile of an in-history pad, else -1)."""
    L = cfg.max_len
    g = np.random.default_rng(SEED)
    seqs = np.zeros((B, L), dtype=np.int64)
    pos = np.zeros(B, dtype=np.int32)
    pad_tile = np.full(B, -1)
    for b in range(B):
        n = LENGTHS[b % len(LENGTHS)]
        c0 = L - n  # pre-padded, the target last
        seqs[b, c0:] = g.integers(1, cfg.n_item + 1, size=n)
        pos[b] = L - 2 if n > 1 else L - 1
        if _no_target(b):
            seqs[b, L - 1] = 0
        if b % 7 == 3:  # consumed on a pad: the one pad a packed sequence may hold
            if n >= 3:
                q = (3 + 5 * (b // 7)) % (n - 1)  # packed index inside the history, in front of the target column
                seqs[b, c0 + q] = 0
                pos[b] = c0 + q
                pad_tile[b] = q >> 4
            else:
                pos[b] = c0 - 1  # in front of the history
    users = g.integers(0, cfg.n_user, size=B).astype(np.int64)
    users[0], users[-1] = 0, cfg.n_user - 1
    return seqs, users, pos, pad_tile


def test_batch_holds_the_cases_and_oracle_decodes_no_target_windows(oracle):
    cfg = _config()
    L = cfg.max_len
    assert L == 48 and B * L > 32768
    seqs, users, pos, pad_tile = _batch(cfg)
    n = np.array([LENGTHS[b % len(LENGTHS)] for b in range(B)])
    nt = np.array([_no_target(b) for b in range(B)])
    assert nt.sum() == B // 5 and set(n[nt]) == set(LENGTHS) and np.all(seqs[nt, L - 1] == 0) and np.all(seqs[~nt, L - 1] != 0)
    assert set(n[:SAMPLE][nt[:SAMPLE]]) == set(LENGTHS)
    padded = np.arange(B) % 7 == 3
    assert np.all(seqs[padded, pos[padded]] == 0) and set(n[padded]) == set(LENGTHS)
    last_tile = (n - 1) >> 4
    for sel in (slice(None), slice(0, SAMPLE)):  # pads in a tile that is only ever diagonal, and below later blocks' diagonals
        assert np.any((pad_tile[sel] >= 0) & (pad_tile[sel] == last_tile[sel]))
        assert np.any((pad_tile[sel] >= 0) & (pad_tile[sel] < last_tile[sel]))
    assert np.any(padded & (pad_tile < 0))  # and in front of the history
    assert users[0] == 0 and users[-1] == cfg.n_user - 1

    sd = synth.irn_state_dict(cfg, 2027)
    full = next(b for b in range(B) if nt[b] and n[b] == L and not padded[b])  # 47 items, the target column empty
    x = oracle.decode(sd, cfg, seqs[full], int(users[full]))[0]
    assert np.isfinite(x).all()
    # without a target item the last history item is a causal key like any other: rows in front of it do not see it
    other = seqs[full].copy()
    other[L - 2] = other[L - 2] % cfg.n_item + 1
    y = oracle.decode(sd, cfg, other, int(users[full]))[0]
    assert np.array_equal(x[:L - 2], y[:L - 2]) and not np.array_equal(x[L - 2], y[L - 2])
    # with one, every row sees it
    tgt = next(b for b in range(B) if not nt[b] and n[b] == L and not padded[b])
    other = seqs[tgt].copy()
    other[L - 1] = other[L - 1] % cfg.n_item + 1
    assert not np.array_equal(oracle.decode(sd, cfg, seqs[tgt], int(users[tgt]))[0][0], oracle.decode(sd, cfg, other, int(users[tgt]))[0][0])
    # pad rows in front of a no-target history see nothing: NaN, and the whole window after the second layer
    short = next(b for b in range(B) if nt[b] and n[b] == 17 and not padded[b])
    assert np.isnan(oracle.decode(sd, cfg, seqs[short], int(users[short]))[0]).all()


@pytest.fixture(scope="module")
def case(oracle):
    """The batch, the two engines and the oracle's rows of the sampled windows (computed once, never written to)."""
    from gpu_util import make_engine
    cfg = _config()
    sd = synth.irn_state_dict(cfg, 2027)
    seqs, users, pos, _ = _batch(cfg)
    engines = {}
    old = os.environ.pop("IRS_ATTN_GEMM", None)
    try:
        for attn in ("planes", "f32"):
            if attn == "f32":
                os.environ["IRS_ATTN_GEMM"] = "f32"
            engines[attn] = make_engine(cfg, sd, max_rows=B, max_seqs=B)
            engines[attn].decoder_seq = 0
    finally:
        os.environ.pop("IRS_ATTN_GEMM", None)
        if old is not None:
            os.environ["IRS_ATTN_GEMM"] = old
    sample = sorted(set(range(SAMPLE)) | set(range(B - 4, B)))
    ref = np.stack([oracle.decode(sd, cfg, seqs[b], int(users[b]))[0] for b in sample])
    ref.setflags(write=False)
    dev = dict(seq=torch.from_numpy(seqs).cuda(), usr=torch.from_numpy(users).cuda(), pos=torch.from_numpy(pos).cuda())
    return dict(cfg=cfg, pos=pos, has_target=seqs[:, cfg.max_len - 1] != 0, engines=engines, sample=np.array(sample), ref=ref, dev=dev)


def _decode(case, attn, rows_only, nb=B):
    eng, d = case["engines"][attn], case["dev"]
    x, xr, _ = eng.decode(d["seq"][:nb].contiguous(), d["usr"][:nb].contiguous(), want_x=not rows_only, pos=d["pos"][:nb].contiguous())
    torch.cuda.synchronize()
    return (xr if rows_only else x).cpu().numpy(), eng.decoder_route_last


def _against_oracle(case, got, route, rows_only, nb=B):
    """got: [nb, d] rows at pos, or [nb, L, d] windows."""
    sample = case["sample"][case["sample"] < nb]
    ref = case["ref"][:len(sample)] if nb < B else case["ref"]
    if rows_only:
        ref = ref[np.arange(len(sample)), case["pos"][sample]]
    g = got[sample]
    assert not np.any(np.isnan(g) & ~np.isnan(ref)), "a NaN row where the oracle's row is a number"
    fin = np.isfinite(g) & np.isfinite(ref)
    assert fin.mean() > 0.5
    bar = X_TOL_X6 if (route["x6"] and route["layer"] == "FRAG_FUSED") else X_TOL  # split-precision layer kernel or float32 rows
    err = float(np.abs(g - ref)[fin].max())
    print(f"{route['layer']} rows_only={rows_only} windows={nb}: max |err| {err:.3g} against the oracle (bar {bar:.3g}), "
          f"{int(fin.all(axis=-1).sum())} finite rows")
    assert err < bar, err


@pytest.mark.gpu
@pytest.mark.parametrize("rows_only", [True, False], ids=["rows_only", "full"])
def test_both_forms_against_oracle_and_each_other(case, rows_only):
    """rows_only: the FAST forms behind the plan (packed sequences); full: the general forms on whole windows."""
    got = {}
    for attn in ("planes", "f32"):
        got[attn], route = _decode(case, attn, rows_only)
        assert route["layer"] == "FRAG_FUSED" and not route["seq"] and route["kv_planes"] == (attn == "planes"), route
        assert route["rows_only"] == rows_only
        _against_oracle(case, got[attn], route, rows_only)
    a, b = got["planes"], got["f32"]
    has_target = case["has_target"]
    assert not np.isnan(a[has_target]).any() and not np.isnan(b[has_target]).any(), "every row of a window with a target sees it"
    if rows_only:
        assert np.array_equal(np.isnan(a), np.isnan(b)), "the two forms differ in their NaN rows"
    else:
        # A window without a target holds rows that see no key (the pads in front of its history): NaN, as in the reference,
        # whose whole window is NaN after the next layer (0 x NaN).  The kernels skip key tiles that are masked throughout, the
        # plane form by PAIRS of tiles and the float32 form tile by tile, so how far the NaN spreads differs between the forms.
        diff = np.isnan(a).any(axis=(1, 2)) != np.isnan(b).any(axis=(1, 2))
        print(f"whole-window decode: {int(diff.sum())} of {int((~has_target).sum())} windows without a target hold NaN rows in one form only")
    fin = np.isfinite(a) & np.isfinite(b)
    err = float(np.abs(a - b)[fin].max())
    print(f"float16-plane form against float32 form, rows_only={rows_only}: max {err:.3g} (bar {X_TOL_X6:.3g})")
    assert err < X_TOL_X6, err


@pytest.mark.gpu
@pytest.mark.parametrize("rows_only", [True, False], ids=["rows_only", "full"])
@pytest.mark.parametrize("attn", ["planes", "f32"])
def test_z_split_grid_on_four_windows(case, attn, rows_only):
    """heads x windows = 16 <= 64: launch_attn's latency branch, which deals one query block per wave over gridDim.z workgroups
    (the float32 form on either engine: the small routes write no planes).  At max_len = 48 a workgroup's four waves hold all
    three blocks, so gridDim.z is 1 here; grids with z > 1 need max_len > 64 and are the route matrix's (c2_b1 .. at 200)."""
    got, route = _decode(case, attn, rows_only, nb=4)
    assert not route["kv_planes"] and not route["seq"] and not route["att_fused"], route
    _against_oracle(case, got, route, rows_only, nb=4)
