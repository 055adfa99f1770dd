"""Test-side restatements of the native training trunk (include/irs_hip.h, irs_train_*):

* the dropout generator (Philox4x32-10, per-element layout of the header) in numpy;
* the stock train-mode trunk in any dtype (InfluentialNet / SampleNet._decoding_autograd with the masks and the zero memory
  built in that dtype, so that a float64 copy of the module runs);
* a functional float64 restatement of the same trunk that takes the dropout masks as arguments."""
import math

import numpy as np
import torch
import torch.nn.functional as F

SITES = {"emb": 0, "self": 1, "drop1": 2, "cross": 3, "drop2": 4, "ffn": 5, "drop3": 6}
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint32 counter arrays and a scalar key: the four output words (uint64 arrays holding uint32)."""
    c = [np.asarray(v, dtype=np.uint64) & _U32 for v in (c0, c1, c2, c3)]
    c = [np.broadcast_to(v, np.broadcast(*c).shape).copy() for v in c]
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(_W0)) & _U32
            k1 = (k1 + np.uint64(_W1)) & _U32
        p0 = c[0] * np.uint64(_M0)
        p1 = c[2] * np.uint64(_M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & _U32
        hi1, lo1 = p1 >> np.uint64(32), p1 & _U32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return c


def keep_words(seed: int, site: int, layer: int, e: np.ndarray) -> np.ndarray:
    """The uint32 word that decides element e (uint64 array) of (site, layer)."""
    e = np.asarray(e, dtype=np.uint64)
    q = e >> np.uint64(2)
    w = philox4x32_10(q & _U32, q >> np.uint64(32), np.uint64(layer), np.uint64(site), seed & 0xFFFFFFFF, seed >> 32)
    sel = (e & np.uint64(3)).astype(np.int64)
    return np.choose(sel, w)


def drop_mult(seed: int, p: float, site: int, layer: int, shape) -> np.ndarray:
    """float64 multiplier (0 or 1 / (1 - p)) of every element of a site, in the header's flat layout (row-major `shape`)."""
    n = int(np.prod(shape))
    if p == 0.0:
        return np.ones(shape)
    thr = np.uint64(math.ceil(float(np.float32(p)) * 16777216.0))
    keep = (keep_words(seed, site, layer, np.arange(n, dtype=np.uint64)) >> np.uint64(8)) >= thr
    return (keep / (1.0 - float(np.float32(p)))).reshape(shape)


def trunk_masks(seed: int, p: float, B: int, L: int, d: int, H: int, F_: int, Lm: int, n_layers: int):
    m = {"emb": drop_mult(seed, p, 0, 0, (B, L, d))}
    for l in range(n_layers):
        m[("self", l)] = drop_mult(seed, p, 1, l, (B, H, L, L))
        m[("drop1", l)] = drop_mult(seed, p, 2, l, (B, L, d))
        m[("cross", l)] = drop_mult(seed, p, 3, l, (B, H, L, Lm))
        m[("drop2", l)] = drop_mult(seed, p, 4, l, (B, L, d))
        m[("ffn", l)] = drop_mult(seed, p, 5, l, (B, L, F_))
        m[("drop3", l)] = drop_mult(seed, p, 6, l, (B, L, d))
    return m


def _emb(net):
    return net.item_embedder if hasattr(net, "item_embedder") else net.word_embedder


def _mask(net, seq, user, dtype):
    """[B, L, L] additive mask incl. key padding (IRN: r_u allowed, last column 1.0; SampleNet: causal 0 / -inf)."""
    B, L = seq.shape
    tril = torch.ones(L, L, device=seq.device).tril().bool()
    if user is not None:
        r = net.user_mask_layer(net.user_embedder(user)).detach().to(dtype).view(B, 1, 1)
        m = torch.where(tril, r.expand(B, L, L), torch.full((B, L, L), float("-inf"), dtype=dtype, device=seq.device))
        m[:, :, -1] = 1.0
    else:
        m = torch.zeros((B, L, L), dtype=dtype, device=seq.device).masked_fill(~tril, float("-inf"))
    return m + torch.zeros((B, 1, L), dtype=dtype, device=seq.device).masked_fill(seq.eq(0).view(B, 1, L), float("-inf"))


def stock_trunk(net, seq, user, dtype):
    """The train-mode nn.TransformerDecoder trunk of _decoding_autograd, built in `dtype` (float64 for the yard-stick)."""
    B, L = seq.shape
    d = net.embed_dim
    x = _emb(net)(seq) * math.sqrt(d) + net.pos_embedder(seq).to(dtype)
    x = F.dropout(x, net.dropout, net.training).transpose(0, 1)
    enc = torch.zeros(net.max_len, B, d, dtype=dtype, device=seq.device)
    mask = torch.repeat_interleave(_mask(net, seq, user, dtype), net.n_heads, dim=0)
    return net.decoder(tgt=x, memory=enc, tgt_mask=mask).transpose(0, 1)


def _ln(x, mod):
    return F.layer_norm(x, (x.shape[-1],), mod.weight, mod.bias, mod.eps)


def functional_trunk(net, seq, user, masks, dtype=torch.float64):
    """The trunk written out with explicit dropout multipliers (from trunk_masks), in `dtype`, on net's parameters."""
    B, L = seq.shape
    d, H = net.embed_dim, net.n_heads
    hd = d // H
    dev = seq.device
    t = lambda a: torch.as_tensor(a, dtype=dtype, device=dev)  # noqa: E731
    pe = net.pos_embedder(seq).to(dtype)
    x = (_emb(net)(seq) * math.sqrt(d) + pe) * t(masks["emb"])
    amask = _mask(net, seq, user, dtype).view(B, 1, L, L)
    for l, lay in enumerate(net.decoder.layers):
        sa = lay.self_attn
        qkv = F.linear(x, sa.in_proj_weight, sa.in_proj_bias).view(B, L, 3, H, hd)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))  # [B, H, L, hd]
        P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd) + amask, dim=-1) * t(masks[("self", l)])
        a = F.linear((P @ v).transpose(1, 2).reshape(B, L, d), sa.out_proj.weight, sa.out_proj.bias)
        y1 = _ln(x + a * t(masks[("drop1", l)]), lay.norm1)
        ca = lay.multihead_attn
        Wq, Wk, Wv = ca.in_proj_weight.split(d)
        bq, bk, bv = ca.in_proj_bias.split(d)
        Lm = net.max_len
        mem = torch.zeros(B, Lm, d, dtype=dtype, device=dev)
        qc = F.linear(y1, Wq, bq).view(B, L, H, hd).transpose(1, 2)
        kc = F.linear(mem, Wk, bk).view(B, Lm, H, hd).transpose(1, 2)
        vc = F.linear(mem, Wv, bv).view(B, Lm, H, hd).transpose(1, 2)
        Pc = torch.softmax(qc @ kc.transpose(-1, -2) / math.sqrt(hd), dim=-1) * t(masks[("cross", l)])
        c = F.linear((Pc @ vc).transpose(1, 2).reshape(B, L, d), ca.out_proj.weight, ca.out_proj.bias)
        y2 = _ln(y1 + c * t(masks[("drop2", l)]), lay.norm2)
        h = torch.relu(F.linear(y2, lay.linear1.weight, lay.linear1.bias)) * t(masks[("ffn", l)])
        f = F.linear(h, lay.linear2.weight, lay.linear2.bias)
        x = _ln(y2 + f * t(masks[("drop3", l)]), lay.norm3)
    return x
