"""Test-side restatement of irs_topk_ensure_survivors (include/irs_hip.h), in plain numpy and Python loops, written from
the header text on top of path_ref.survivors.  The exact ranking of the whole catalog comes from the caller (on the GPU
tests: the oracle's scoring chain and its total order), so nothing here scores anything."""
import numpy as np

from path_ref import survivors

RESCUED = 8  # IRS_ROW_RESCUED


def list_is_full(ids0_row):
    """The list has k valid entries: it does not end at a negative id."""
    return all(int(i) >= 0 for i in ids0_row)


def is_starved(window, val_row, ids0_row, want):
    """A full list with fewer than `want` survivors.  A list that ended early already is the whole catalog."""
    return list_is_full(ids0_row) and len(survivors(window, val_row, ids0_row, want)) < want


def best_admissible(window, rank_val, rank_ids0, want):
    """The first `want` entries of the catalog's exact ranking (score descending, id ascending) whose item is not in the
    window: (values float32 [n], ids0 int64 [n])."""
    present = set(int(v) for v in window)
    keep = [c for c in range(len(rank_ids0)) if int(rank_ids0[c]) + 1 not in present][:want]
    return np.asarray(rank_val, dtype=np.float32)[keep], np.asarray(rank_ids0, dtype=np.int64)[keep]


def ensure_survivors(seq, hep, val, ids0, status, want, ranking, rows_per_status=1, cum=None, fin=None, done=None):
    """Returns (val, ids0, status, starved rows) after the pass, on copies.  ranking(m) -> (values, ids0) of row m's exact
    ranking of the WHOLE catalog.  Skipped rows: cum == -inf, fin != 0, done != 0 for the row's user."""
    seq, hep = np.asarray(seq), np.asarray(hep)
    val, ids0, status = np.array(val, dtype=np.float32), np.array(ids0, dtype=np.int64), np.array(status, dtype=np.int32)
    M, k = ids0.shape
    assert 1 <= want <= min(k, 32) and rows_per_status >= 1 and M % rows_per_status == 0
    starved = []
    for m in range(M):
        u = m // rows_per_status
        if cum is not None and cum[m] == -np.inf:
            continue
        if fin is not None and fin[m] != 0:
            continue
        if done is not None and done[u] != 0:
            continue
        window = seq[m, :int(hep[m]) + 1]  # positions beyond hep do not count, whatever they hold
        if not is_starved(window, val[m], ids0[m], want):
            continue
        starved.append(m)
        v, i = best_admissible(window, *ranking(m), want)
        n = len(i)
        val[m, :n], ids0[m, :n] = v, i
        if n < k:
            val[m, n], ids0[m, n] = -np.inf, -1  # the list ends here; entries behind it keep what they held
        status[u] |= RESCUED
    return val, ids0, status, starved
