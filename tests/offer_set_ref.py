"""The CPU statement of the offer set (irs_bind_offer_set, irs_score_topk_offer; include/irs_hip.h).

A row's ranked list under a bound set S is the whole catalog's chain scores (oracle.score_chain), restricted to S, in
recommend_ref.ranking's order -- score descending, id ascending -- cut at k and filled with (-inf, -1).  Nothing of the device
code is restated here: the selection is numpy's sort over the restricted scores."""
import numpy as np

import recommend_ref

NINF = np.float32(-np.inf)
TILE, HDR = 64, 256  # ids per workgroup tile of the score kernel; the scratch header (word 0: the hole count)


def sanitise(ids0, n_item):
    """The binding's launch: (ids [C] with -1 for a hole, the hole count).  An entry is a hole when it lies outside [0, n_item) or
    is not greater than its predecessor in the caller's array."""
    ids = np.asarray(ids0, dtype=np.int64)
    prev = np.concatenate([[np.iinfo(np.int64).min], ids[:-1]])
    ok = (ids >= 0) & (ids < n_item) & (ids > prev)
    return np.where(ok, ids, -1), int((~ok).sum())


def topk(scores, set_ids0, k):
    """(val float32 [k], ids0 int64 [k], fewer) of one row: `scores` are the chain scores of the WHOLE catalog, set_ids0 the
    set's valid ids."""
    s = np.asarray(set_ids0, dtype=np.int64)
    s = s[s >= 0]
    vals, order = recommend_ref.ranking(np.asarray(scores, dtype=np.float32)[s])
    n = min(k, len(s))
    val = np.full(k, NINF, dtype=np.float32)
    ids = np.full(k, -1, dtype=np.int64)
    val[:n], ids[:n] = vals[:n], s[order[:n]]
    return val, ids, n < k


def brute_force(scores, set_ids0, k):
    """The same list by repeated selection, without sorting: k times the best item of the set not yet taken."""
    s = np.asarray(scores, dtype=np.float32)
    left = sorted(int(j) for j in set_ids0 if j >= 0)
    val = np.full(k, NINF, dtype=np.float32)
    ids = np.full(k, -1, dtype=np.int64)
    for i in range(min(k, len(left))):
        best = left[0]
        for j in left[1:]:
            if s[j] > s[best]:  # (ascending walk: an equal score never replaces a lower id; -0.0 > 0.0 is false)
                best = j
        left.remove(best)
        val[i], ids[i] = s[best], best
    return val, ids


def scratch_bytes(n_ids, rows, n_item, max_rows):
    """irs_offer_set_scratch_bytes: the header, the sanitised ids padded to whole tiles (rounded up to 256 bytes), one pass of
    float32 scores; 0 for invalid arguments."""
    if not (1 <= n_ids <= n_item and 1 <= rows <= max_rows):
        return 0
    c_pad = (n_ids + TILE - 1) // TILE * TILE
    return HDR + (8 * c_pad + 255) // 256 * 256 + 4 * rows * c_pad


def complement(set_ids0, n_item):
    """The ids an exclusion list must hold so that what is left of the catalog is the set."""
    keep = np.zeros(n_item, dtype=bool)
    keep[np.asarray(set_ids0, dtype=np.int64)] = True
    return np.nonzero(~keep)[0].astype(np.int64)
