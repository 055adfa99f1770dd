"""The float16-plane range bound restated in numpy float64 (test infrastructure, no GPU).

irs_finalize_weights takes eight statistics of the bound weights (irs_launch_h3_range, influentialrs_amd/csrc/decoder.hip) and
folds them into one bound on every float16-plane operand (irs_h3_operand_bound); at LIMIT = 32752 or more the engine runs the
split-bf16 kernels instead.  Here:

  stats            the eight statistics from a state dict
  terms            the five terms of the bound by name, and their maximum
  operand_maxima   a float64 forward of the decoder that returns the largest magnitude each operand class really reaches
  scaled / solve   one tensor family of a model multiplied until the bound sits in a window around LIMIT

tests/test_h3_range_host.py checks the restatement against itself (deciding terms, soundness), tests/test_gpu_h3_range.py the
engine against the restatement."""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np

from oracle import oracle_np

LIMIT = 32752.0          # irs_finalize_weights: h3_ok = bound < 32752 (half the float16 range)
WSCALE = 256.0           # the float16 weight planes hold 2^8 x the weights (x6_wscale(2))
FAMILIES = ("E", "pe", "ln_gamma", "ln_beta", "cross_bias", "ffn1", "v_rows", "out_w")
TERMS = ("embed", "ln", "v", "hidden", "wplane")


def seq_shape(cfg) -> bool:
    """irs_seq_shape (irs_internal.h): the dims of the sequence-resident layer kernel, whose attention splits q and k rows too."""
    return cfg.emb_dim == 128 and cfg.ffn_dim == 256 and cfg.n_heads == 4 and cfg.max_len <= 256 and cfg.n_layers > 1


def _emb(evaluator: bool) -> str:
    return "word_embedder.weight" if evaluator else "item_embedder.weight"


def _amax(*arrays) -> float:
    m = 0.0
    for a in arrays:
        a = np.abs(np.asarray(a, dtype=np.float64))
        m = max(m, float(np.inf if np.isnan(a).any() else a.max()))   # a NaN weight fails the bound
    return m


def _rownorm_max(W) -> float:
    q = np.sqrt((np.asarray(W, dtype=np.float64) ** 2).sum(axis=1))
    return float(np.inf if np.isnan(q).any() else q.max())


def stats(sd, cfg, evaluator: bool = False) -> np.ndarray:
    """st[0..7]: max|E|, max|pe|, max LayerNorm |gamma|, max LayerNorm |beta|, max|c_l|, max row norm of W1, max row norm of the V
    rows of W_in (all 3d rows on the sequence-resident dims), max of every other |weight| and |bias| that becomes or feeds an
    operand (self-attention W_in, b_in, W_o; W1, b1, W2)."""
    d = cfg.emb_dim
    st = np.zeros(8, dtype=np.float64)
    st[0] = _amax(sd[_emb(evaluator)])
    st[1] = _amax(sd["pos_embedder.pe"].reshape(-1, d)[:cfg.max_len])
    for l in range(cfg.n_layers):
        p = f"decoder.layers.{l}."
        st[2] = max(st[2], _amax(*(sd[p + n + ".weight"] for n in ("norm1", "norm2", "norm3"))))
        st[3] = max(st[3], _amax(*(sd[p + n + ".bias"] for n in ("norm1", "norm2", "norm3"))))
        st[4] = max(st[4], _amax(oracle_np.cross_attn_const(sd, p, d, np.float64)))
        st[5] = max(st[5], _rownorm_max(sd[p + "linear1.weight"]))
        Win = sd[p + "self_attn.in_proj_weight"]
        st[6] = max(st[6], _rownorm_max(Win if seq_shape(cfg) else Win[2 * d:]))
        st[7] = max(st[7], _amax(sd[p + "self_attn.out_proj.weight"], sd[p + "linear1.weight"], sd[p + "linear2.weight"], Win,
                                 sd[p + "linear1.bias"], sd[p + "self_attn.in_proj_bias"]))
    return st


def terms(st, d: int) -> Dict[str, float]:
    """The terms of irs_h3_operand_bound by name, and `bound`, their maximum."""
    rd = math.sqrt(d)
    embed = st[0] * rd + st[1]                     # an embedded token
    ln = rd * st[2] + st[3] + st[4]                # a LayerNorm output (+ c_l)
    xin = rd * max(embed, ln)                      # norm of a layer's input row
    v = xin * st[6] + st[7]                        # a V row, the attention output (sequence-resident dims: a q or k row too)
    hidden = rd * ln * st[5] + st[7]               # a hidden activation
    t = dict(embed=float(embed), ln=float(ln), v=float(v), hidden=float(hidden), wplane=float(st[7] * WSCALE))
    t["bound"] = max(t[k] for k in TERMS)
    return t


def deciding(t: Dict[str, float]) -> str:
    return max(TERMS, key=lambda k: t[k])


def bound(sd, cfg, evaluator: bool = False) -> Tuple[float, str, Dict[str, float]]:
    t = terms(stats(sd, cfg, evaluator), cfg.emb_dim)
    return t["bound"], deciding(t), t


def operand_maxima(sd, cfg, seqs, users, evaluator: bool = False):
    """A float64 forward of the post-norm decoder layer (mask and c_l as oracle_np.decoder_layer) over the windows `seqs`.
    Returns (maxima, rows): the largest magnitude reached by each operand class of the float16-plane kernels, and the final rows
    [B, L, d] (equal to oracle_np.decode(..., dtype=np.float64))."""
    f8 = np.float64
    d, H = cfg.emb_dim, cfg.n_heads
    hd = d // H
    names = ("embed", "layer_in", "ln1", "ln1_c", "ln2", "q", "k", "v", "attn_out", "hidden", "wplane")
    mx = {k: 0.0 for k in names}

    def see(k, a):
        a = np.abs(a)
        if np.isfinite(a).any():
            mx[k] = max(mx[k], float(np.nanmax(a)))

    out = []
    for b, seq in enumerate(np.asarray(seqs, dtype=np.int64)):
        L = seq.shape[0]
        x = oracle_np.embed_pe(sd[_emb(evaluator)], sd["pos_embedder.pe"], seq, f8)
        see("embed", x)
        if evaluator:
            mask = oracle_np.causal_mask(L, seq, f8)
        else:
            mask = oracle_np.irn_mask(L, oracle_np.pif(sd, int(users[b]), f8), seq, f8)
        with np.errstate(invalid="ignore"):
            for l in range(cfg.n_layers):
                p = f"decoder.layers.{l}."
                g = lambda k: sd[p + k].astype(f8)
                see("layer_in", x)
                qkv = x @ g("self_attn.in_proj_weight").T + g("self_attn.in_proj_bias")
                q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
                see("q", q), see("k", k), see("v", v)
                o = np.empty_like(x)
                for h in range(H):
                    sl = slice(h * hd, (h + 1) * hd)
                    s = (q[:, sl] * f8(1.0 / math.sqrt(hd))) @ k[:, sl].T + mask
                    pr = np.exp(s - s.max(axis=1, keepdims=True))
                    o[:, sl] = (pr / pr.sum(axis=1, keepdims=True)) @ v[:, sl]
                see("attn_out", o)
                y = oracle_np.layer_norm(x + (o @ g("self_attn.out_proj.weight").T + g("self_attn.out_proj.bias")),
                                         g("norm1.weight"), g("norm1.bias"))
                see("ln1", y)
                y = y + oracle_np.cross_attn_const(sd, p, d, f8)
                see("ln1_c", y)
                y = oracle_np.layer_norm(y, g("norm2.weight"), g("norm2.bias"))
                see("ln2", y)
                hdn = np.maximum(y @ g("linear1.weight").T + g("linear1.bias"), 0)
                see("hidden", hdn)
                x = oracle_np.layer_norm(y + (hdn @ g("linear2.weight").T + g("linear2.bias")), g("norm3.weight"), g("norm3.bias"))
        see("layer_in", x)  # (a layer's output is the next one's input; the last one's leaves the decoder in float32)
        out.append(x)
    mx["wplane"] = float(stats(sd, cfg, evaluator)[7] * WSCALE)
    return mx, np.stack(out)


def scaled(sd, cfg, which: str, s: float):
    """A copy of `sd` with one tensor family multiplied by s (float32 tensors).  ffn1 and v_rows are function-preserving pairs:
    relu is positively homogeneous, and the attention output is linear in V."""
    assert which in FAMILIES, which
    d, s = cfg.emb_dim, np.float32(s)
    out = dict(sd)

    def mul(key, f, rows=slice(None)):
        a = np.array(out[key], dtype=np.float32, copy=True)
        a[rows] = a[rows] * np.float32(f)
        out[key] = a

    if which == "E":
        mul("word_embedder.weight" if "word_embedder.weight" in sd else "item_embedder.weight", s)
    elif which == "pe":
        mul("pos_embedder.pe", s)
    elif which in ("ln_gamma", "ln_beta"):
        for n in ("norm1", "norm2", "norm3"):
            mul(f"decoder.layers.0.{n}." + ("weight" if which == "ln_gamma" else "bias"), s)
    else:
        for l in range(cfg.n_layers):
            p = f"decoder.layers.{l}."
            if which == "cross_bias":
                mul(p + "multihead_attn.out_proj.bias", s)
            elif which == "ffn1":
                mul(p + "linear1.weight", s), mul(p + "linear1.bias", s), mul(p + "linear2.weight", 1.0 / s)
            elif which == "v_rows":
                mul(p + "self_attn.in_proj_weight", s, slice(2 * d, 3 * d)), mul(p + "self_attn.in_proj_bias", s, slice(2 * d, 3 * d))
                mul(p + "self_attn.out_proj.weight", 1.0 / s)
            else:
                mul(p + "self_attn.out_proj.weight", s)
    return out


def solve(sd, cfg, which: str, lo: float, hi: float, evaluator: bool = False) -> Tuple[float, str]:
    """Bisects on log s until the restated bound of scaled(sd, cfg, which, s) lies in [lo, hi] x LIMIT.  Returns s and the name
    of the deciding term there."""
    assert 0 < lo < hi

    def at(s):
        b, name, _ = bound(scaled(sd, cfg, which, s), cfg, evaluator)
        return b / LIMIT, name

    r, name = at(1.0)
    if lo <= r <= hi:
        return 1.0, name
    # bracket from s = 1 in the direction that moves the bound towards the window (every family is monotone on that side)
    step = 2.0 if r < lo else 0.5
    a = z = 1.0
    for _ in range(80):
        z = a * step
        rz, name = at(z)
        if lo <= rz <= hi:
            return float(np.float32(z)), name
        if (rz > hi) == (r < lo):
            break
        a = z
    else:
        raise AssertionError(f"scaling {which} never moves the bound across [{lo}, {hi}] x {LIMIT}")
    a, z = min(a, z), max(a, z)
    for _ in range(200):
        s = math.sqrt(a * z)
        r, name = at(s)
        if lo <= r <= hi:
            return float(np.float32(s)), name
        if r < lo:
            a = s
        else:
            z = s
    raise AssertionError(f"no scale of {which} puts the bound in [{lo}, {hi}] x {LIMIT}")
