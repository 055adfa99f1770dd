"""Test-side restatement of the path replay (include/irs_hip.h, "path replay"), in plain numpy: written from the header's closed
forms, not from the kernel.  replay_window gives the window of one row (user after i forced items); replay_rows the three
values of every row from the row's exact float32 logits, through path_trace_ref.step_values."""
import numpy as np

import path_trace_ref

SLOT, FULL = 0, 1  # IRS_REPLAY_SLOT, IRS_REPLAY_FULL
NO_CANDIDATE = path_trace_ref.NO_CANDIDATE


def first_zero(row):
    z = np.where(np.asarray(row) == 0)[0]
    return len(row) if len(z) == 0 else int(z[0])


def replay_window(seq0, hep0, path, i, layout):
    """(window int64 [L], hep) of a VALID row: seq0 the user's start row, hep0 its start hep (SLOT; None for FULL), path the
    user's items, i the number of forced items."""
    seq0 = np.asarray(seq0, dtype=np.int64)
    L = len(seq0)
    w = np.zeros(L, dtype=np.int64)
    if layout == FULL:
        n0 = first_zero(seq0)
        src = np.concatenate([seq0[:n0], np.asarray(path[:i], dtype=np.int64)])
        n = n0 + i
        s = max(n - L, 0)
        w[:n - s] = src[s:]
        return w, min(n, L) - 1
    h0 = int(hep0)
    g = L - 2 - h0
    if i <= g:
        w[:] = seq0
        w[h0 + 1:h0 + 1 + i] = path[:i]
        return w, h0 + i
    src = np.concatenate([seq0[:h0 + 1], np.asarray(path[:i], dtype=np.int64)])
    w[:L - 1] = src[i - g:]
    w[L - 1] = seq0[L - 1]
    return w, L - 2


def row_valid(seq0, hep0, paths, P, n_item, b, i, layout):
    B, L = np.asarray(seq0).shape
    if not (0 <= b < B and 0 <= i <= P):
        return False
    if any(v < 1 or v > n_item for v in paths[b][:i]):
        return False
    if layout == FULL:
        return first_zero(seq0[b]) + i > 0
    return 0 <= int(hep0[b]) <= L - 2


def fallback_window(seq0, hep0, b, layout):
    """What an invalid row launches: the start window of user b (user 0 when b is no user)."""
    B, L = np.asarray(seq0).shape
    bs = b if 0 <= b < B else 0
    if layout == FULL:
        n0 = first_zero(seq0[bs])
        w = np.zeros(L, dtype=np.int64)
        w[:n0] = seq0[bs][:n0]
        if n0 == 0:
            w[0] = 1
        return w, max(n0, 1) - 1
    return np.array(seq0[bs], dtype=np.int64), min(max(int(hep0[bs]), 0), L - 2)


def replay_windows(seq0, hep0, paths, P, n_item, row_user, row_step, layout):
    """(seq [R, L], hep [R], status [R]) of irs_replay_windows."""
    seq0 = np.asarray(seq0)
    R, L = len(row_user), seq0.shape[1]
    seq, hep, status = np.zeros((R, L), dtype=np.int64), np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    for r, (b, i) in enumerate(zip(row_user, row_step)):
        b, i = int(b), int(i)
        if row_valid(seq0, hep0, paths, P, n_item, b, i, layout):
            seq[r], hep[r] = replay_window(seq0[b], None if layout == FULL else hep0[b], paths[b], i, layout)
        else:
            seq[r], hep[r] = fallback_window(seq0, hep0, b, layout)
            status[r] = NO_CANDIDATE
    return seq, hep, status


def replay_rows(logits, seq, hep, status, targets, items):
    """(lp_item, lp_target float32 [R], rank int32 [R]) from each row's exact logits [R, N], its window seq[r, :hep[r] + 1], its
    target and its forced item (0: none; outside the catalog: no item either).  Invalid rows read zeros."""
    R, N = len(seq), np.asarray(logits).shape[1]
    lp_item, lp_target, rank = np.zeros(R, dtype=np.float32), np.zeros(R, dtype=np.float32), np.zeros(R, dtype=np.int32)
    for r in range(R):
        if status[r]:
            continue
        c = int(items[r]) if 1 <= int(items[r]) <= N else 0
        lp_item[r], lp_target[r], rank[r] = path_trace_ref.step_values(logits[r], seq[r][:int(hep[r]) + 1], targets[r], c)
    return lp_item, lp_target, rank
