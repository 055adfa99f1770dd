"""CPU statement of irs_recommend / irs_recommend_take (include/irs_hip.h, "recommend"): test infrastructure.

A catalog item j (0-based) is admissible for a row when item j + 1 is not in the row's window seq[m, :hep[m] + 1] and j is not in the
bound user's exclusion list.  The slate is the first n admissible items of the whole catalog in the library's total order (score
descending, -0 folded onto +0, id ascending); count = min(n, admissible items); entries behind count are (-inf, -1) with lp -inf;
lp = val - (max + log(sumexp)) in float64 (the device rounds that to float32 once).

`ranking` / `slate` start from a row's chain scores (oracle.score_chain); `take` restates the kernel alone on a caller's list."""
import numpy as np

NINF = -np.inf


def ranking(scores):
    """(values float32 [N], ids0 int64 [N]) of the whole catalog in the library's order."""
    s = np.asarray(scores, dtype=np.float32)
    order = np.lexsort((np.arange(s.shape[0]), -s.astype(np.float64)))  # (-0.0 == 0.0 here: the tie goes to the lower id)
    return s[order], order.astype(np.int64)


def window_items(seq_row, hep):
    """The 1-based items of seq_row[:hep + 1]; None or hep < 0: the empty window.  Pads (0) are no items."""
    if seq_row is None or hep is None or hep < 0:
        return set()
    return {int(v) for v in np.asarray(seq_row)[:int(hep) + 1] if v > 0}


def listed(excl_row, n_item):
    """The 0-based ids a bound exclusion row hides: -1 marks an unused slot, ids >= n_item never match."""
    if excl_row is None:
        return set()
    return {int(v) for v in np.asarray(excl_row) if 0 <= v < n_item}


def lp64(val, mx, sm):
    """The float64 expression behind lp: (double)val - ((double)max + log((double)sumexp))."""
    return np.float64(val) - (np.float64(np.float32(mx)) + np.log(np.float64(np.float32(sm))))


def _fill(vals, ids, n, lse):
    count = min(n, len(ids))
    o_val = np.full(n, NINF, dtype=np.float32)
    o_ids = np.full(n, -1, dtype=np.int64)
    o_val[:count], o_ids[:count] = vals[:count], ids[:count]
    lp = None
    if lse is not None:
        lp = np.full(n, NINF, dtype=np.float64)
        lp[:count] = [lp64(v, *lse) for v in o_val[:count]]
    return o_val, o_ids, lp, count


def take(val_row, ids0_row, n, window, hidden, lse=None):
    """The kernel alone: the first n admissible entries of a list that ends at its first negative id.  window: a set of 1-based
    items, hidden: a set of 0-based ids, lse: (max, sumexp) or None.  Returns (val [n], ids0 [n], lp float64 [n] or None, count)."""
    vals, ids = [], []
    for v, j in zip(val_row, ids0_row):
        if j < 0:
            break
        if int(j) + 1 in window or int(j) in hidden:
            continue
        vals.append(v)
        ids.append(int(j))
        if len(ids) == n:
            break
    return _fill(vals, ids, n, lse)


def slate(scores, n, window=frozenset(), hidden=frozenset(), lse=None):
    """The whole call for one row, from its chain scores over the whole catalog."""
    vals, ids = ranking(scores)
    return take(vals, ids, n, window, hidden, lse)


def is_short(ids0_row, n, window, hidden):
    """The row's list shows all k valid entries and fewer than n admissible ones: irs_recommend repairs it (IRS_ROW_RESCUED)."""
    ids = np.asarray(ids0_row)
    if (ids < 0).any():
        return False
    return sum(1 for j in ids if int(j) + 1 not in window and int(j) not in hidden) < n


def brute_force(scores, n, window, hidden):
    """The slate by repeated selection, without sorting anything: n times the best item not yet taken and admissible."""
    s = np.asarray(scores, dtype=np.float32)
    left = [j for j in range(s.shape[0]) if j + 1 not in window and j not in hidden]
    out = []
    while left and len(out) < n:
        best = left[0]
        for j in left[1:]:
            if s[j] > s[best]:  # (ascending walk: an equal score never replaces a lower id; -0.0 > 0.0 is false)
                best = j
        out.append(best)
        left.remove(best)
    return out


def scratch_bytes(n_local, rows, n, k):
    """irs_recommend_scratch_bytes: the lists, (max, sum exp), the empty windows, then irs_survivor_scratch_bytes(rows, n)."""
    up = lambda v: (v + 15) // 16 * 16
    ns = 1
    while ns < 256 and ns * 2 * 128 <= n_local:
        ns *= 2
    while ns > 1 and rows * ns * n > (1 << 21):
        ns //= 2
    surv = 256 + up(4 * rows) + 8 * rows * ns * n
    return up(8 * rows * k) + up(4 * rows * k) + 3 * up(4 * rows) + surv
