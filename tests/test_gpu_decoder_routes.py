"""-m gpu: every decoder kernel route of tests/decoder_route_cases.py against a float64 reference.

Each case decodes one seeded batch with edge contents (a target-only window, a full window, a repeated item, item ids 1 and n_item,
users 0 and n_user - 1, consumed positions at 0, at L - 1 and on a pad, the sequences of the last partial tile), asserts that
irs_decoder_route_last reports the case's route, and compares the rows with oracle.decode(..., dtype=np.float64) on a seeded sample
that always holds the edge sequences (r_u with the float64 user factor over the whole batch):

- the NaN pattern is identical;
- max |err| is within the bar of the arithmetic, the bars test_gpu_decoder_path.py keeps against the float32 oracle (X_TOL float32
  kernels, X_TOL_X6 split-precision kernels; at d > 128 x2 / x1.5, whole float32 windows x3: see _max_bar);
- mean |err| is under a systematic-error bar, and the least-squares scale sum(got * ref) / sum(ref * ref) is within a bar of 1: a
  bias that stays under the max bar (a LayerNorm eps off by 10x in one family, a truncating accumulator, a wrong row in a partial
  tile that lands near its neighbour) moves these.

Rows-only cases whose full decode fits decode the full window too: the consumed rows must equal the full decode's pos rows within
the same max bar over the WHOLE batch.  Measured errors go to decoder_route_errors.json beside the parity record of
parity_record.py (with the float32 oracle's own error on the same sequences, for comparison)."""
import json
import os

import numpy as np
import pytest
import torch

import decoder_route_cases as C
from gpu_util import make_engine
from parity_record import OUT as PARITY_OUT
from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_GEMM_F32, IRS_GEMM_H3, IRS_GEMM_X6
from test_gpu_decoder_path import X_TOL, X_TOL_X6

pytestmark = pytest.mark.gpu

OUT = os.path.join(os.path.dirname(PARITY_OUT), "decoder_route_errors.json")
GEMM = {"h3": IRS_GEMM_H3, "x6": IRS_GEMM_X6, "f32": IRS_GEMM_F32}
SEQ = {0: 0, 1: 1, "auto": None}
N_SAMPLE = 16
# systematic-error bars against float64, per arithmetic (mean |err| over the sampled rows; |scale - 1|), calibrated on one MI355X
# run of this module over all cases: 3x the worst measured value.  Measured worst (case): mean f32 1.31e-6 (c2_b1_att_fused, one
# row; 1.24e-6 c4d_full_b164), split 7.2e-7 (c4d_b164); |scale - 1| f32 6.0e-8 (c2_b1_att_fused), split 2.8e-8 (c2_b600_x6).
# (The float32 oracle on the same rows: mean up to 8.5e-7.)
MEAN_BAR = {"f32": 3.9e-6, "split": 2.2e-6}
SCALE_BAR = {"f32": 1.8e-7, "split": 8.4e-8}
_ENG = {}


def _arith(c):
    return "split" if C.split_precision(c) else "f32"


def _max_bar(c, cfg):
    """The bars of test_gpu_decoder_path.py: split-precision rows X_TOL_X6 (x1.5 at d > 128, test_split_bf16_layer_kernel_d256),
    float32 rows X_TOL (x2 at d > 128, test_throughput_shape_decode_matches_small_batches_and_oracle; whole windows at d > 128 x3,
    test_decoder_random_shapes_against_oracle: over 200 positions of 16 sequences the float32 oracle itself is 3.3e-5 from float64
    at c4d, the kernels 4.3e-5)."""
    if C.split_precision(c):
        return X_TOL_X6 * (1.5 if cfg.emb_dim > 128 else 1.0)
    if cfg.emb_dim > 128:
        return X_TOL * (2.0 if c.rows_only else 3.0)
    return X_TOL


def _engine(c):
    key = c.engine_key()
    if key not in _ENG:
        _ENG.clear()  # one engine resident at a time (the c2 group is sized for 8193 sequences)
        cfg = c.config()
        sd = synth.irn_state_dict(cfg, 2027, evaluator=c.evaluator)
        n = C.max_seqs(key)
        old = os.environ.pop("IRS_ATTN_GEMM", None)
        try:
            if c.attn != "h3":
                os.environ["IRS_ATTN_GEMM"] = c.attn
            eng = make_engine(cfg, sd, evaluator=c.evaluator, max_rows=n, max_seqs=n)
        finally:
            os.environ.pop("IRS_ATTN_GEMM", None)
            if old is not None:
                os.environ["IRS_ATTN_GEMM"] = old
        _ENG[key] = (cfg, sd, eng)
    return _ENG[key]


def _batch(c, cfg, seed):
    """Seeded windows plus the edge contents; returns seqs [B, L], users [B] (None for the evaluator), pos [B], edge indices."""
    B, L, n_item = c.B, cfg.max_len, cfg.n_item
    g = np.random.default_rng(seed)
    seqs = np.zeros((B, L), dtype=np.int64)
    pos = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = int(np.clip(g.lognormal(np.log(max(2.0, 0.4 * L)), 0.8), 1, L))  # tokens in the window
        items = g.integers(1, n_item + 1, size=n)
        if c.evaluator:
            seqs[b, :n] = items                    # post-padded, no target
            pos[b] = n - 1
        else:
            seqs[b, L - n:] = items                # pre-padded, the target last
            pos[b] = L - 2 if n > 1 else L - 1
    # edge contents, on the first sequences (a one-sequence batch keeps an ordinary window)
    edges = []

    def edge(b, window, p):
        if b < B:
            seqs[b] = window
            pos[b] = p
            edges.append(b)

    def win(tokens):
        w = np.zeros(L, dtype=np.int64)
        tokens = np.asarray(tokens, dtype=np.int64)[:L]
        if c.evaluator:
            w[:len(tokens)] = tokens
        else:
            w[L - len(tokens):] = tokens
        return w

    first, last_item = (0, L - 1) if c.evaluator else (L - 1, L - 1)
    edge(1, win([int(g.integers(1, n_item + 1))]), first)                      # length 1 (IRN: the target alone)
    edge(2, win(g.integers(1, n_item + 1, size=L)), L - 1)                     # full window, no pad
    edge(3, win([int(g.integers(1, n_item + 1))] * L), L // 2)                 # one item repeated across the window
    edge(4, win([1, n_item] * (L // 2) + [1] * (L % 2)), 0)                    # item ids 1 and n_item, consumed at 0
    n5 = max(1, L // 3)
    w5 = win(g.integers(1, n_item + 1, size=n5))
    # consumed position on a pad: IRN -- in front of the history (the row sees the target); evaluator -- behind the items
    edge(5, w5, (L - n5 - 1 if L - n5 - 1 >= 0 else 0) if not c.evaluator else min(n5, L - 1))
    if not c.evaluator:
        edge(6, win([int(g.integers(1, n_item + 1))]), 0)                      # target alone, consumed at a pad (position 0)
    else:
        edge(6, win(g.integers(1, n_item + 1, size=max(1, L // 2))), L - 1)    # evaluator: consumed at L - 1, a pad
    users = None
    if not c.evaluator:
        users = g.integers(0, cfg.n_user, size=B).astype(np.int64)
        users[0] = 0
        users[-1] = cfg.n_user - 1
    pos[np.arange(B) % 97 == 50] = last_item                                    # a few more at L - 1
    return seqs, users, pos, edges


def _sample(B, edges, seed):
    tail = [b for b in (B - 3, B - 2, B - 1) if b >= 0]                        # the last partial tile
    must = sorted(set([0] + edges + tail))
    rest = np.setdiff1d(np.arange(B), must)
    g = np.random.default_rng(seed + 1)
    extra = g.choice(rest, size=min(len(rest), max(0, N_SAMPLE - len(must))), replace=False) if len(rest) else []
    return sorted(set(must) | set(int(b) for b in extra))


def _record(key, data):
    try:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        cur = {}
        if os.path.exists(OUT):
            with open(OUT) as fh:
                cur = json.load(fh)
        cur[key] = data
        with open(OUT, "w") as fh:
            json.dump(cur, fh, indent=1, sort_keys=True)
    except OSError:
        pass  # a read-only tree must not fail the test


def _ordered():
    """The cases grouped by engine (one engine per group), table order otherwise."""
    keys = []
    for c in C.CASES:
        if c.engine_key() not in keys:
            keys.append(c.engine_key())
    return sorted(C.CASES, key=lambda c: keys.index(c.engine_key()))


@pytest.mark.parametrize("c", _ordered(), ids=lambda c: c.id)
def test_decoder_route_against_float64(oracle, c):
    cfg, sd, eng = _engine(c)
    L, B = cfg.max_len, c.B
    seqs, users, pos, edges = _batch(c, cfg, seed=1000 + B)
    seq = torch.from_numpy(seqs).cuda()
    usr = None if users is None else torch.from_numpy(users).cuda()
    p = torch.from_numpy(pos).cuda()
    eng.decoder_gemm = GEMM[c.gemm]
    eng.decoder_seq = SEQ[c.seq]
    try:
        x, xr, ru = eng.decode(seq, usr, want_x=not c.rows_only, pos=p, want_r_u=not c.evaluator)
        route = eng.decoder_route_last
        x = None if x is None else x.cpu().numpy()
        xr = xr.cpu().numpy()
        ru = None if ru is None else ru.cpu().numpy()
        full = None
        if c.rows_only and c.full_check:
            _, xr_full, _ = eng.decode(seq, usr, want_x=True, pos=p)
            full = xr_full.cpu().numpy()
    finally:
        eng.decoder_gemm = IRS_GEMM_H3
        eng.decoder_seq = None
    assert route == c.route, {k: (route[k], c.route[k]) for k in route if route[k] != c.route[k]}

    if ru is not None:  # the user factor over the whole batch, float64
        U = sd["user_embedder.weight"].astype(np.float64)[users]
        ref_ru = U @ sd["user_mask_layer.weight"][0].astype(np.float64) + np.float64(sd["user_mask_layer.bias"][0])
        assert np.abs(ru - ref_ru).max() < 1e-6

    sample = _sample(B, edges, seed=1000 + B)
    got, ref, ref32, where = [], [], [], []
    for b in sample:
        u = None if users is None else int(users[b])
        o64 = oracle.decode(sd, cfg, seqs[b], u, evaluator=c.evaluator, dtype=np.float64)[0]
        o32 = oracle.decode(sd, cfg, seqs[b], u, evaluator=c.evaluator)[0]
        if x is not None:  # a full decode: every position of the window
            assert np.array_equal(xr[b], x[b, pos[b]]), b
            rows = list(range(L))
            got.append(x[b])
        else:
            rows = [int(pos[b])]
            got.append(xr[b][None])
        ref.append(o64[rows])
        ref32.append(o32[rows])
        where += [(b, i) for i in rows]
    got, ref, ref32 = np.concatenate(got), np.concatenate(ref), np.concatenate(ref32)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs from the float64 reference"
    fin = np.isfinite(ref) & np.isfinite(got)
    assert fin.any()
    err_all = np.where(fin, np.abs(got - ref), 0.0)
    worst_b, worst_p = where[int(np.argmax(err_all.max(axis=1)))]
    err = err_all[fin]
    err32 = np.abs(ref32 - ref)[fin & np.isfinite(ref32)]
    g64, r64 = got[fin].astype(np.float64), ref[fin]
    scale = float((g64 * r64).sum() / (r64 * r64).sum())
    m = dict(max=float(err.max()), mean=float(err.mean()), scale_minus_1=scale - 1.0, oracle32_max=float(err32.max()),
             oracle32_mean=float(err32.mean()), arith=_arith(c), values=int(fin.sum()), sample=len(sample),
             worst=[int(worst_b), int(worst_p), int(seqs[worst_b, worst_p])])
    if full is not None:
        both = np.isfinite(xr) & np.isfinite(full)
        assert np.array_equal(np.isnan(xr), np.isnan(full)), "rows-only and full decode differ in their NaN rows"
        m["rows_only_vs_full_max"] = float(np.abs(xr - full)[both].max()) if both.any() else 0.0
    _record(c.id, m)
    bar = _max_bar(c, cfg)
    assert m["max"] < bar, (c.id, m)
    assert m["mean"] < MEAN_BAR[_arith(c)], (c.id, m)
    assert abs(m["scale_minus_1"]) < SCALE_BAR[_arith(c)], (c.id, m)
    if full is not None:
        assert m["rows_only_vs_full_max"] < bar, (c.id, m)
