"""Test-side restatement of the guided path step (include/irs_hip.h: irs_bind_guide), in plain numpy and Python loops, written
from the header text on top of path_ref and exclusion_ref.

While a guide is bound a greedy step collects the first min(k_c, available) survivors of the row's ranked list (the list as the
unguided step sees it: window, bound list and path struck), and takes the one nearest to the target seq[row][L - 1] in the
feature table; ties go to the better rank, NaN sorts last.  Record and window update are path_ref's."""
import numpy as np

import exclusion_ref
import path_ref

BINARY, FLOAT = 1, 2
MAX_KC, MAX_BITS, MAX_FLOATS = 32, 1024, 512


def scratch_bytes(n_item, kind, F):
    """irs_guide_scratch_bytes as the header states it; 0 for a float guide and for invalid arguments."""
    if kind != BINARY or F < 1 or F > MAX_BITS:
        return 0
    return ((n_item + 1) * ((F + 31) // 32) * 4 + 255) // 256 * 256


def pack_bits(table):
    """uint32 [rows, ceil(F / 32)]: feature f in bit f % 32 of word f / 32, nonzero = 1, the bits behind F zero."""
    table = np.asarray(table) != 0
    rows, F = table.shape
    words = (F + 31) // 32
    out = np.zeros((rows, words), dtype=np.uint32)
    for f in range(F):
        out[:, f // 32] |= table[:, f].astype(np.uint32) << np.uint32(f % 32)
    return out


def _popcount(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8), axis=-1).sum(axis=-1)


def dist_binary_many(table, t, items):
    """Hamming distances of row t to the rows `items`: the popcount of the XOR over the packed words."""
    table = np.asarray(table)
    p = pack_bits(table[[t] + [int(i) for i in items]])
    return _popcount(p[1:] ^ p[:1]).astype(np.int64)


def dist_binary(table, t, c):
    return int(dist_binary_many(table, t, [c])[0])


def fma32(a, b, c):
    """float32 fma(a, b, c) with its single rounding, elementwise.  a * b is exact in float64 (24 x 24 bits); the float64 sum s
    of it and c is rounded once already, so where s lands exactly half-way between two float32 neighbours the exact residual of
    the sum (TwoSum) decides the direction instead of round-half-even.  Anywhere else s and the exact value lie on the same
    side of every float32 midpoint (midpoints are float64 numbers and rounding to float64 is monotone), so float32(s) is right."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)  # exact where everything is finite: p + c == s + e
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        toward = np.where(s > r64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        n = np.nextafter(r, toward)
        n64 = n.astype(np.float64)
        tie = np.isfinite(s) & np.isfinite(n64) & (e != 0) & (r64 != s) & (np.abs(s - r64) == np.abs(n64 - s))
        return np.where(tie & ((e > 0) == (n64 > r64)), n, r).astype(np.float32)


def dist_float_many(table, t, items):
    """Squared Euclidean distances of row t to the rows `items`, each as ONE float32 chain: acc = fmaf(t_f - c_f, t_f - c_f,
    acc), f ascending, acc from 0 (the chains run side by side, one per item)."""
    table = np.asarray(table, dtype=np.float32)
    tr, cr = table[t], table[[int(i) for i in items]]
    acc = np.zeros(len(cr), dtype=np.float32)
    with np.errstate(all="ignore"):
        for f in range(table.shape[1]):
            df = (tr[f] - cr[:, f]).astype(np.float32)
            acc = fma32(df, df, acc)
    return acc


def dist_float(table, t, c):
    return dist_float_many(table, t, [c])[0]


def closer(d, best):
    """Does d replace best?  Strictly smaller only; a NaN never replaces, anything but a NaN replaces a NaN."""
    return bool(d < best) or bool(best != best and d == d)


def choose(table, kind, target, items):
    """Index into `items` (the survivors, 1-based, rank order) of the guided choice."""
    table = np.asarray(table)
    rows = table.shape[0]
    if len(items) == 0:
        return -1
    if not 1 <= target < rows:
        return 0
    inside = [i for i, it in enumerate(items) if 1 <= it < rows]  # an id outside the table is never looked up: the farthest
    if kind == FLOAT:
        dists = np.full(len(items), np.nan, dtype=np.float32)
        if inside:
            dists[inside] = dist_float_many(table, target, [items[i] for i in inside])
    else:
        dists = np.full(len(items), 0xFFFFFFFF, dtype=np.int64)
        if inside:
            dists[inside] = dist_binary_many(table, target, [items[i] for i in inside])
    best = 0
    for i in range(1, len(items)):
        if closer(dists[i], dists[best]):
            best = i
    return best


def path_step(seq, hep, val, ids0, step, paths, status, table, kind, k_c, excl=None, n_item=None, no_repeat=False, user_of=None):
    """irs_path_step while a guide is bound (and exclusions, when excl / no_repeat are given): (seq, hep, paths, status) after the
    step, on copies."""
    seq, hep, paths, status = (np.array(a) for a in (seq, hep, paths, status))
    B, L = seq.shape
    n_item = np.asarray(table).shape[0] - 1 if n_item is None else n_item
    user_of = range(B) if user_of is None else user_of
    for r in range(B):
        v, i = np.asarray(val[r]), np.asarray(ids0[r])
        if excl is not None or no_repeat:
            gone = exclusion_ref.hidden(None if excl is None else excl[user_of[r]], n_item, paths[r], step, no_repeat)
            v, i = exclusion_ref.strike(v, i, gone)
        surv = path_ref.survivors(seq[r, :hep[r] + 1], v, i, k_c)
        if not surv:
            status[r] |= path_ref.NO_CANDIDATE
            paths[r, step] = 0
            continue
        item = surv[choose(table, kind, int(seq[r, L - 1]), [s[0] for s in surv])][0]
        paths[r, step] = item
        seq[r], hep[r] = path_ref.advance(seq[r], int(hep[r]), item)
    return seq, hep, paths, status
