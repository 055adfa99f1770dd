"""-m gpu: decodes behind long windows (256 < max_len <= 1024) against a float64 reference, by the method of
tests/test_gpu_decoder_routes.py over the table of tests/long_window_cases.py.

Each case decodes that module's seeded batch with its edge contents, asserts the route, compares a sample of at most 12 sequences
with oracle.decode(..., dtype=np.float64) -- identical NaN pattern, max / mean / scale bars -- runs the rows-only decode against the
full decode over the whole batch, and repeats the same call once: bit-identical.

A second batch per engine (CONTENT_CASES) holds the windows the table of tests/decoder_route_cases.py cannot: only the last three
slots filled (every earlier key chunk fully masked), exactly 256 and exactly 257 tokens, full windows, IRN windows without a target
item (one consumed on a leading pad: a NaN row), consumed positions 0, 255, 256 and L - 1.

Error bars.  The bars of test_gpu_decoder_routes.py (_max_bar, MEAN_BAR, SCALE_BAR: float32 arithmetic) were calibrated at
L <= 256, and the float32 ORACLE is itself 1.3e-5 to 1.5e-5 from float64 at c2, two layers, L = 320 / 1024 -- close to X_TOL = 2e-5.
So per case: where the float32 oracle's own maximum error on the sampled rows exceeds a third of the existing max bar, the max bar
is 3 x that error (the project's calibration margin: the kernels sum in another order than numpy), and the mean and scale bars grow
by the same ratio.  Both errors per case go to long_window_errors.json beside the parity record."""
import json
import os

import numpy as np
import pytest
import torch

import long_window_cases as LW
from gpu_util import make_engine
from parity_record import OUT as PARITY_OUT
from influentialrs_amd import synth
from test_gpu_decoder_routes import MEAN_BAR, SCALE_BAR, _arith, _batch, _max_bar

pytestmark = pytest.mark.gpu

OUT = os.path.join(os.path.dirname(PARITY_OUT), "long_window_errors.json")
N_SAMPLE = 12
_ENG = {}


def _engine(c):
    key = c.engine_key()
    if key not in _ENG:
        _ENG.clear()  # one engine resident at a time
        cfg = c.config()
        sd = synth.irn_state_dict(cfg, 2027, evaluator=c.evaluator)
        n = LW.max_seqs(key)
        _ENG[key] = (cfg, sd, make_engine(cfg, sd, evaluator=c.evaluator, max_rows=n, max_seqs=n))
    return _ENG[key]


def _sample(B, must, seed):
    must = sorted(set([0] + list(must) + [b for b in (B - 3, B - 2, B - 1) if b >= 0]))[:N_SAMPLE]
    rest = np.setdiff1d(np.arange(B), must)
    g = np.random.default_rng(seed + 1)
    extra = g.choice(rest, size=min(len(rest), N_SAMPLE - len(must)), replace=False) if len(rest) else []
    return sorted(set(must) | set(int(b) for b in extra))


def _content_batch(cfg, evaluator, seed):
    """The windows of the module docstring: seqs [N_CONTENT, L], users, pos, and the rows that must come out NaN."""
    L, n_item = cfg.max_len, cfg.n_item
    g = np.random.default_rng(seed)

    def win(n, target=True):
        """n tokens: IRN -- pre-padded, the last one the target (without: n history items in front of an empty last slot);
        evaluator -- post-padded"""
        w = np.zeros(L, dtype=np.int64)
        items = g.integers(1, n_item + 1, size=n)
        if evaluator:
            w[:n] = items
        elif target:
            w[L - n:] = items
        else:
            w[L - 1 - n:L - 1] = items
        return w

    rows = [
        (win(3), L - 2 if not evaluator else 2),       # only the last three slots (IRN): every earlier key chunk is masked
        (win(256), 0),                                 # exactly 256 tokens, consumed at 0 (IRN: a pad in front of them)
        (win(257), 255),                               # exactly 257 tokens
        (win(L), 256),                                 # a full window, consumed in its second 256-key chunk
        (win(L), L - 1),                               # a full window, consumed at L - 1
        (win(L // 2, target=False), 3),                # IRN without a target, consumed on a leading pad: no visible key
        (win(L - 1, target=False), L - 2),             # IRN without a target, no pad in front: the last key is a causal key
        (win(max(4, L // 3)), 255),
        (win(257), 256),
        (win(L - 7), 0),
    ]
    assert len(rows) == LW.N_CONTENT
    seqs = np.stack([r[0] for r in rows])
    pos = np.array([r[1] for r in rows], dtype=np.int32)
    users = None if evaluator else g.integers(0, cfg.n_user, size=len(rows)).astype(np.int64)
    return seqs, users, pos, ([] if evaluator else [5])


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


def _check(oracle, c, tag, seqs, users, pos, must, nan_rows, seed):
    cfg, sd, eng = _engine(c)
    B = seqs.shape[0]
    seq = torch.from_numpy(seqs).cuda()
    usr = None if users is None else torch.from_numpy(users).cuda()
    p = torch.from_numpy(pos).cuda()
    _, xr_t, ru = eng.decode(seq, usr, want_x=False, pos=p, want_r_u=not c.evaluator)
    route = eng.decoder_route_last
    _, xr_again, _ = eng.decode(seq, usr, want_x=False, pos=p)
    _, xr_full, _ = eng.decode(seq, usr, want_x=True, pos=p)
    xr, again, full = xr_t.cpu().numpy(), xr_again.cpu().numpy(), xr_full.cpu().numpy()
    assert route == c.route, {k: (route[k], c.route[k]) for k in route if route[k] != c.route[k]}
    assert np.array_equal(xr.view(np.uint32), again.view(np.uint32)), "the same call twice differs in its bits"

    if ru is not None:  # the user factor over the whole batch, float64
        U = sd["user_embedder.weight"].astype(np.float64)[users]
        ref_ru = U @ sd["user_mask_layer.weight"][0].astype(np.float64) + np.float64(sd["user_mask_layer.bias"][0])
        assert np.abs(ru.cpu().numpy() - ref_ru).max() < 1e-6

    sample = _sample(B, must, seed)
    assert len(sample) <= N_SAMPLE
    ref, ref32 = [], []
    for b in sample:
        u = None if users is None else int(users[b])
        ref.append(oracle.decode(sd, cfg, seqs[b], u, evaluator=c.evaluator, dtype=np.float64)[0][int(pos[b])])
        ref32.append(oracle.decode(sd, cfg, seqs[b], u, evaluator=c.evaluator)[0][int(pos[b])])
    got, ref, ref32 = xr[sample], np.stack(ref), np.stack(ref32)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs from the float64 reference"
    for b in nan_rows:
        assert np.isnan(ref[sample.index(b)]).all(), "the window without a visible key is a NaN row of the reference"
    fin = np.isfinite(ref) & np.isfinite(got)
    assert fin.any()
    err = np.abs(got - ref)[fin]
    err32 = np.abs(ref32 - ref)[fin & np.isfinite(ref32)]
    g64, r64 = got[fin].astype(np.float64), ref[fin]
    scale = float((g64 * r64).sum() / (r64 * r64).sum())
    both = np.isfinite(xr) & np.isfinite(full)
    assert np.array_equal(np.isnan(xr), np.isnan(full)), "rows-only and full decode differ in their NaN rows"
    base_bar = _max_bar(c, cfg)
    o32 = float(err32.max())
    ratio = 3.0 * o32 / base_bar if o32 > base_bar / 3.0 else 1.0
    bar, mean_bar, scale_bar = base_bar * ratio, MEAN_BAR[_arith(c)] * ratio, SCALE_BAR[_arith(c)] * ratio
    m = dict(max=float(err.max()), mean=float(err.mean()), scale_minus_1=scale - 1.0, oracle32_max=o32,
             oracle32_mean=float(err32.mean()), arith=_arith(c), values=int(fin.sum()), sample=len(sample),
             rows_only_vs_full_max=float(np.abs(xr - full)[both].max()) if both.any() else 0.0,
             max_bar=bar, mean_bar=mean_bar, scale_bar=scale_bar, L=int(cfg.max_len), B=int(B))
    print(c.id + tag, json.dumps(m, sort_keys=True))
    _record(c.id + tag, m)
    assert m["max"] < bar, (c.id, m)
    assert m["mean"] < mean_bar, (c.id, m)
    assert abs(m["scale_minus_1"]) < scale_bar, (c.id, m)
    assert m["rows_only_vs_full_max"] < bar, (c.id, m)


def _ordered():
    """The cases grouped by engine (one engine per group), each group's batch of special windows behind its CONTENT case."""
    keys = []
    for c in LW.CASES:
        if c.engine_key() not in keys:
            keys.append(c.engine_key())
    out = []
    for c in sorted(LW.CASES, key=lambda c: keys.index(c.engine_key())):
        out.append((c, False))
        if c.id in LW.CONTENT_CASES:
            out.append((c, True))
    return out


@pytest.mark.parametrize("c,content", _ordered(), ids=lambda v: v.id if hasattr(v, "id") else ("windows" if v else "batch"))
def test_long_window_decode_against_float64(oracle, c, content):
    cfg = _engine(c)[0]
    assert cfg.max_len > 256 and cfg.n_layers == 2
    if content:
        assert c.B <= 64  # (the special batch takes the case's own route: the single-workgroup plan)
        seqs, users, pos, nan_rows = _content_batch(cfg, c.evaluator, seed=77 + cfg.max_len)
        _check(oracle, c, ":windows", seqs, users, pos, range(LW.N_CONTENT), nan_rows, seed=77)
    else:
        seqs, users, pos, edges = _batch(c, cfg, seed=1000 + c.B)
        _check(oracle, c, "", seqs, users, pos, edges, [], seed=1000 + c.B)
