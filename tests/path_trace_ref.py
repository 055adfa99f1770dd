"""Test-side restatement of the path trace (include/irs_hip.h, "path trace"), in plain numpy, built on path_ref: written from
the header's text, not from the kernels.  A row's logits are whatever exact float32 scores the caller has (the oracle's chain,
or the library's own dense logits); everything else is walked the slow, obvious way."""
import math

import numpy as np

import path_ref

NO_CANDIDATE = path_ref.NO_CANDIDATE


def lse64(logits):
    """log sum_j exp(e_j) over the whole row, in float64."""
    e = np.asarray(logits, dtype=np.float32).astype(np.float64)
    m = e.max()
    return float(m + math.log(np.exp(e - m).sum()))


def target_rank(logits, window, target):
    """1 + #{ j : j + 1 is not a non-pad entry of `window`, and (e_j, j) ranks before (e_{t-1}, t-1) }: score descending, id
    ascending, -0 folded onto +0 (path_ref.order_key).  0 without a target."""
    t = int(target)
    if t < 1 or t > len(logits):
        return 0
    key = path_ref.order_key(logits)
    hidden = set(int(v) for v in window if int(v) != 0)
    kt = int(key[t - 1])
    n = 0
    for j in range(len(logits)):
        if j + 1 in hidden:
            continue
        kj = int(key[j])
        if kj > kt or (kj == kt and j < t - 1):
            n += 1
    return 1 + n


def step_values(logits, window, target, chosen):
    """(lp_item, lp_target float32, rank_target int) of one row at one step, measured before the step chose `chosen` (1-based;
    0: the step chose nothing)."""
    logits = np.asarray(logits, dtype=np.float32)
    lse = lse64(logits)
    t = int(target)
    has_t = 1 <= t <= len(logits)
    lp_t = np.float32(float(logits[t - 1]) - lse) if has_t else np.float32(0)
    lp_c = np.float32(float(logits[int(chosen) - 1]) - lse) if int(chosen) != 0 else np.float32(0)
    return lp_c, lp_t, target_rank(logits, window, target)


def trace_rows(logits, seq, hep, chosen):
    """step_values over the rows of one step: logits [B, N], seq [B, L] (target last), hep [B], chosen [B]."""
    B = len(seq)
    lp_item, lp_target = np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.float32)
    rank = np.zeros(B, dtype=np.int32)
    for b in range(B):
        lp_item[b], lp_target[b], rank[b] = step_values(logits[b], seq[b][:int(hep[b]) + 1], seq[b][-1], chosen[b])
    return lp_item, lp_target, rank
