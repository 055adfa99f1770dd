"""The CPU statement of the bound sampler (include/irs_hip.h, "sampler": irs_bind_sampler / irs_sampler_choose), in plain numpy and
Python loops.  Written from the header: the walk is the path step's (window + the user's list + the path under no_repeat, the list
ends at its first negative id), the integer RNG is exact, the distribution is stated in float64.  `emulate32` restates the
float32 expressions in a chosen summation order, for the host test that confirms the derived tolerance TOL."""
import math

import numpy as np

import exclusion_ref

MAX_SAMPLER_K = 256
OFFERED = 16  # IRS_ROW_OFFERED
NINF = np.float32(-np.inf)
MASK = (1 << 64) - 1
# The largest permitted gap between a float32 cumulative bound S_m / S_m* and the float64 one.  Derived, not measured: arguments
# that matter are at most 20 in magnitude; the subtraction and the product round once each, at most 2 * 20 * 2^-24 = 2.4e-6 absolute
# in the argument; expf is within 2 ulp (2.4e-7 relative): every w_i carries a relative error of at most about 2.6e-6.  A sum of
# n <= 256 terms adds at most n * 2^-24 = 1.5e-5 relative.  A ratio doubles it: at most 3.6e-5.
TOL = 5e-5


def draw_bits(seed, row_id, step):
    """z >> 40 of the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * (row_id * 1315423911 + step + 1): 24 bits."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * ((int(row_id) * 1315423911 + int(step) + 1) & MASK)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z = z ^ (z >> 31)
    return z >> 40


def draw(seed, row_id, step):
    """u = (z >> 40) * 2^-24, exact in float32."""
    return np.float32(draw_bits(seed, row_id, step) * 2.0 ** -24)


def walk(window, val_row, ids0_row, top_k, gone=()):
    """The first top_k admissible entries of a ranked list as [(value, position)]: not in `window` (1-based items), not in `gone`
    (1-based items: the user's list and, under no_repeat, the path so far).  The list ends at its first negative id."""
    present = {int(v) for v in window} | {int(g) for g in gone}
    out = []
    for c in range(len(ids0_row)):
        if len(out) >= top_k or ids0_row[c] < 0:
            break
        if int(ids0_row[c]) + 1 not in present:
            out.append((val_row[c], c))
    return out


def weights64(v, inv_t):
    """w_i = exp((v_i - v_0) * inv_T) in float64 on the float32 values, inv_T the float32 the host formed; -inf gives 0."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isneginf(v), 0.0, np.exp((v - v[0]) * float(np.float32(inv_t))))


def choose64(v, inv_t, top_p, u):
    """The float64 statement on one row's kept values: dict(index, support, lq, cum -- S_m / S_m* for m = 1 .. m* --, frac --
    S_m / S_n for m = 1 .. n --, near -- the distance of u to the nearest cumulative bound it could cross and of top_p to the
    nearest frac it could cross)."""
    if not np.isfinite(v[0]):
        return dict(index=0, support=1, lq=0.0, cum=np.ones(1), frac=np.ones(1), near_u=1.0, near_p=1.0)
    w = weights64(v, inv_t)
    S = np.cumsum(w)
    frac = S / S[-1]
    tp = float(np.float32(top_p))
    support = int(np.argmax(S >= tp * S[-1])) + 1
    cum = S[:support] / S[support - 1]
    t = float(u)
    above = np.where(cum > t)[0]
    index = int(above[0]) if len(above) else support - 1
    inner = cum[:-1]  # (the last bound is 1 > u: never crossed)
    near_u = float(np.abs(inner - t).min()) if len(inner) else 1.0
    near_p = float(np.abs(frac[:-1] - tp).min()) if len(frac) > 1 else 1.0  # (S_n itself always reaches top_p * S_n)
    with np.errstate(divide="ignore"):
        lq = float(np.log(w[index] / S[support - 1]))
    return dict(index=index, support=support, lq=lq, cum=cum, frac=frac, near_u=near_u, near_p=near_p)


def _sum32(w, order):
    """Prefix sums of float32 terms in float32: "serial", or "pairwise" (blocks of four summed serially, the blocks' totals by a
    Hillis-Steele scan: the kernel's order)."""
    w = np.asarray(w, dtype=np.float32)
    n = len(w)
    out = np.zeros(n, dtype=np.float32)
    if order == "serial":
        acc = np.float32(0)
        for i in range(n):
            acc = np.float32(acc + w[i])
            out[i] = acc
        return out
    lanes = (n + 3) // 4
    own = np.zeros((lanes, 4), dtype=np.float32)
    tot = np.zeros(lanes, dtype=np.float32)
    for l in range(lanes):
        acc = np.float32(0)
        for j in range(4):
            acc = np.float32(acc + (w[4 * l + j] if 4 * l + j < n else np.float32(0)))
            own[l, j] = acc
        tot[l] = acc
    incl = tot.copy()
    d = 1
    while d < 64:
        nxt = incl.copy()
        for l in range(d, lanes):
            nxt[l] = np.float32(incl[l] + incl[l - d])
        incl = nxt
        d <<= 1
    for i in range(n):
        l, j = divmod(i, 4)
        out[i] = own[l, j] if l == 0 else np.float32(incl[l - 1] + own[l, j])
    return out


def emulate32(v, inv_t, top_p, u, order="pairwise"):
    """The stated float32 expressions on one row: dict(index, support, lq, S -- the float32 prefix sums)."""
    v = np.asarray(v, dtype=np.float32)
    if not np.isfinite(v[0]):
        return dict(index=0, support=1, lq=np.float32(0), S=np.ones(1, dtype=np.float32))
    inv_t, top_p, u = np.float32(inv_t), np.float32(top_p), np.float32(u)
    with np.errstate(invalid="ignore", over="ignore"):
        arg = ((v - v[0]).astype(np.float32) * inv_t).astype(np.float32)
        w = np.where(np.isneginf(v), np.float32(0), np.exp(arg.astype(np.float64)).astype(np.float32)).astype(np.float32)
    S = _sum32(w, order)
    n = len(v)
    thr = np.float32(top_p * S[n - 1])
    support = int(np.argmax(S >= thr)) + 1 if (S >= thr).any() else n
    t = np.float32(u * S[support - 1])
    above = np.where(S[:support] > t)[0]
    index = int(above[0]) if len(above) else support - 1
    with np.errstate(divide="ignore"):
        lq = np.float32(math.log(float(np.float32(w[index] / S[support - 1])))) if w[index] > 0 else NINF
    return dict(index=index, support=support, lq=lq, S=S)


def choose(seq, hep, val, ids0, top_k, temperature, top_p, step, seed, row_ids=None, status=None, fin=None, excl=None, n_item=None,
           paths=None, no_repeat=False):
    """irs_sampler_choose on copies: returns (val, ids0, rec) with rec = dict(u float32 [M], lq float64 [M], support int32 [M],
    written bool [M], index int [M] -- the chosen slot among the kept candidates, -1: none --, n [M], near_u / near_p float [M],
    kept -- per row the [(value, position)] walked).  Row r reads list and path of user row_ids[r] (None: r)."""
    seq, hep = np.asarray(seq), np.asarray(hep)
    val, ids0 = np.array(val, dtype=np.float32), np.array(ids0, dtype=np.int64)
    M, k = ids0.shape
    L = seq.shape[1]
    inv_t = np.float32(1.0) / np.float32(temperature)
    rec = dict(u=np.zeros(M, dtype=np.float32), lq=np.zeros(M), support=np.zeros(M, dtype=np.int32), written=np.zeros(M, dtype=bool),
               index=np.full(M, -1), n=np.zeros(M, dtype=np.int64), near_u=np.ones(M), near_p=np.ones(M), kept=[[] for _ in range(M)],
               recorded=np.zeros(M, dtype=bool))
    for r in range(M):
        if fin is not None and fin[r]:
            continue
        rec["recorded"][r] = True
        rid = r if row_ids is None else int(row_ids[r])
        if status is not None and (int(status[r]) & OFFERED) and ids0[r, 0] == seq[r, L - 1] - 1 and (k == 1 or ids0[r, 1] < 0):
            rec["support"][r] = 1
            continue
        gone = ()
        if excl is not None or no_repeat:
            gone = exclusion_ref.hidden(None if excl is None else excl[rid], n_item, None if paths is None else paths[rid], step, no_repeat)
        kept = walk(seq[r, :max(int(hep[r]) + 1, 0)], val[r], ids0[r], min(top_k, MAX_SAMPLER_K), gone)
        rec["kept"][r], rec["n"][r] = kept, len(kept)
        if not kept:
            continue
        u = draw(seed, rid, step)
        c = choose64(np.array([kv[0] for kv in kept], dtype=np.float32), inv_t, top_p, u)
        v_c, pos = kept[c["index"]]
        id_c = ids0[r, pos]
        val[r, 0], ids0[r, 0] = v_c, id_c
        if k > 1:
            val[r, 1], ids0[r, 1] = NINF, -1
        rec["u"][r], rec["lq"][r], rec["support"][r], rec["written"][r], rec["index"][r] = u, c["lq"], c["support"], True, c["index"]
        rec["near_u"][r], rec["near_p"][r] = c["near_u"], c["near_p"]
    return val, ids0, rec
