"""Test-side restatements of the kernels that turn scores into paths (include/irs_hip.h: irs_path_step,
irs_beam_step, irs_pack_topk / irs_merge_topk / irs_merge_topk_keys, irs_build_eval_batch), in plain numpy and Python
loops.  Written from the header and from the behaviour of the reference's get_seq_in_batch
(influentialRS.py:419-450), not from the kernels: every row is walked the slow, obvious way."""
import math

import numpy as np

NO_CANDIDATE = 2  # IRS_ROW_NO_CANDIDATE


def survivors(window, val_row, ids0_row, want):
    """The first `want` candidates of a ranked list that are absent from `window` (1-based items), as
    [(item, val, position in the list)].  The list ends at its first negative id."""
    present = set(int(v) for v in window)
    out = []
    for c in range(len(ids0_row)):
        if len(out) >= want:
            break
        if ids0_row[c] < 0:
            break
        item = int(ids0_row[c]) + 1
        if item not in present:
            out.append((item, val_row[c], c))
    return out


def advance(win, hep, item):
    """Window after `item` was chosen: grown while there is room before the target, else shifted left by one with
    the target kept last.  Returns (new window, new hep)."""
    L = len(win)
    new = np.array(win, dtype=np.int64)
    if hep < L - 2:
        new[hep + 1] = item
        return new, hep + 1
    new[:L - 2] = win[1:L - 1]
    new[L - 2] = item
    new[L - 1] = win[L - 1]
    return new, hep


def path_step(seq, hep, val, ids0, step, paths, status, sample=False, sample_k=3):
    """One path step on copies of the state.
    greedy: (seq, hep, paths, status) after the step;
    sample: per row (items int64 [n], probabilities float64 [n]) of the first sample_k survivors (softmax of their
    scores); no choice is made."""
    seq, hep, paths, status = (np.array(a) for a in (seq, hep, paths, status))
    B = seq.shape[0]
    dists = []
    for r in range(B):
        surv = survivors(seq[r, :hep[r] + 1], val[r], ids0[r], sample_k if sample else 1)
        if sample:
            items = np.array([s[0] for s in surv], dtype=np.int64)
            v = np.array([s[1] for s in surv], dtype=np.float64)
            p = np.exp(v - v.max()) if len(v) else v
            dists.append((items, p / p.sum() if len(v) else p))
            continue
        if not surv:
            status[r] |= NO_CANDIDATE
            paths[r, step] = 0
            continue
        item = surv[0][0]
        paths[r, step] = item
        seq[r], hep[r] = advance(seq[r], int(hep[r]), item)
    return dists if sample else (seq, hep, paths, status)


def beam_step(state_in, val, ids0, lse_max, lse_sum, step, P, status=None):
    """One beam step.  state = (seq [B, W, L] int64, hep [B, W] int32, cum [B, W] float64, paths [B, W, P] float32);
    val / ids0 [B * W, k]; lse_max / lse_sum [B * W] or None (W == 1).  Returns (state_out, status [B])."""
    seq_i, hep_i, cum_i, paths_i = (np.asarray(a) for a in state_in)
    B, W, L = seq_i.shape
    seq_o, hep_o = np.zeros_like(seq_i), np.zeros_like(hep_i)
    cum_o = np.full((B, W), -np.inf, dtype=np.float64)
    paths_o = np.zeros((B, W, P), dtype=np.float32)
    status = np.zeros(B, dtype=np.int32) if status is None else np.array(status, dtype=np.int32)
    for b in range(B):
        cands = []
        for j in range(W):
            if not cum_i[b, j] > -np.inf:
                continue  # dead beam
            row = b * W + j
            norm = 0.0
            if W > 1:
                norm = float(np.float64(lse_max[row])) + math.log(float(np.float64(lse_sum[row])))
            surv = survivors(seq_i[b, j, :hep_i[b, j] + 1], val[row], ids0[row], W)
            if not surv:
                status[b] |= NO_CANDIDATE
            for rank, (item, v, _) in enumerate(surv):
                cands.append((float(cum_i[b, j]) + (float(np.float64(v)) - norm), j, rank, item))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        for t in range(W):
            if t >= len(cands):  # dead beam: window and hep of input beam 0, empty path
                seq_o[b, t], hep_o[b, t] = seq_i[b, 0], hep_i[b, 0]
                continue
            score, j, _, item = cands[t]
            seq_o[b, t], hep_o[b, t] = advance(seq_i[b, j], int(hep_i[b, j]), item)
            paths_o[b, t, :step] = paths_i[b, j, :step]
            paths_o[b, t, step] = item
            cum_o[b, t] = score
    return (seq_o, hep_o, cum_o, paths_o), status


def order_key(val):
    """uint64 array holding the 32-bit key whose unsigned order is the float32 order, -0.0 folded onto +0.0."""
    u = np.ascontiguousarray(val, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, np.uint64(0), u)
    neg = (u >> np.uint64(31)) == 1
    return np.where(neg, u ^ np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


def pack_keys(val, ids0):
    """The exchange step's wire format: (order key << 32) | (0xFFFFFFFF - id0); 0 where id0 < 0."""
    ids0 = np.asarray(ids0, dtype=np.int64)
    low = (np.int64(0xFFFFFFFF) - np.where(ids0 >= 0, ids0, 0)).astype(np.uint64)
    return np.where(ids0 >= 0, (order_key(val) << np.uint64(32)) | low, np.uint64(0))


def merge(val_in, ids_in, k):
    """[W, M, k'] lists -> the best k of every row by (score descending, id ascending); entries with id -1 do not
    exist, -0.0 counts (and comes out) as +0.0, the tail is (-inf, -1)."""
    val_in = np.asarray(val_in, dtype=np.float32)
    ids_in = np.asarray(ids_in, dtype=np.int64)
    W, M, _ = val_in.shape
    val = np.full((M, k), -np.inf, dtype=np.float32)
    ids = np.full((M, k), -1, dtype=np.int64)
    for m in range(M):
        v, i = val_in[:, m].reshape(-1), ids_in[:, m].reshape(-1)
        v, i = v[i >= 0] + np.float32(0.0), i[i >= 0]  # x + 0.0 turns -0.0 into +0.0 and nothing else
        order = np.lexsort((i, -v.astype(np.float64)))[:k]
        val[m, :len(order)], ids[m, :len(order)] = v[order], i[order]
    return val, ids


def build_eval_batch(items, offsets, L, raw_len, gap_len, targets):
    """The deterministic outputs of the device-side loader: (seq [B, L], label [B], raw [B, raw_len] right-aligned,
    raw_n [B])."""
    B = len(offsets) - 1
    seq = np.zeros((B, L), dtype=np.int64)
    label = np.zeros(B, dtype=np.int64)
    raw = np.zeros((B, raw_len), dtype=np.int64)
    raw_n = np.zeros(B, dtype=np.int32)
    for b in range(B):
        ev = [int(x) for x in items[offsets[b]:offsets[b + 1]]]
        if ev:
            label[b] = ev[-1]
        window = ev[:-1][-raw_len:]
        raw_n[b] = len(window)
        if window:
            raw[b, raw_len - len(window):] = window
        shown = window[-(L - gap_len - 1):]
        end = L - 1 - gap_len
        if shown:
            seq[b, end - len(shown):end] = shown
        seq[b, L - 1] = targets[b]
    return seq, label, raw, raw_n
