"""Test-side restatement of the beam search with an end symbol (include/irs_hip.h: irs_beam_step_until,
irs_beam_search_until), in plain numpy / float64 and Python loops, written from the header.

The end symbol of a window is its target, seq[L - 1].  A beam that has chosen it is finished: it is not expanded again
and competes with its final score as one candidate of index parent * W + 0.  A user is done when no output beam is both
live and unfinished (STOP_ALL), or already when output beam 0 is finished (STOP_BEST); a done user is copied through."""
import math

import numpy as np

import path_ref

STOP_ALL, STOP_BEST = 0, 1


def beam_step_until(state_in, done, val, ids0, lse_max, lse_sum, step, P, stop_rule, status=None):
    """One step.  state = (seq [B, W, L] int64, hep [B, W] int32, cum [B, W] float64, paths [B, W, P] float32,
    fin [B, W] int32); done [B] int32; val / ids0 [B * W, k]; lse_max / lse_sum [B * W] or None (W == 1).
    Returns (state_out, done_out, status [B])."""
    seq_i, hep_i, cum_i, paths_i, fin_i = (np.asarray(a) for a in state_in)
    B, W, L = seq_i.shape
    seq_o, hep_o = np.zeros_like(seq_i), np.zeros_like(hep_i)
    cum_o = np.full((B, W), -np.inf, dtype=np.float64)
    paths_o = np.zeros((B, W, P), dtype=np.float32)
    fin_o = np.zeros((B, W), dtype=np.int32)
    done_o = np.array(done, dtype=np.int32)
    status = np.zeros(B, dtype=np.int32) if status is None else np.array(status, dtype=np.int32)
    for b in range(B):
        if done_o[b]:  # copied through, whatever its lists hold
            seq_o[b], hep_o[b], cum_o[b], paths_o[b], fin_o[b] = seq_i[b], hep_i[b], cum_i[b], paths_i[b, :, :P], fin_i[b]
            continue
        cands = []  # (score, index, parent, item or None for a finished beam)
        for j in range(W):
            if not cum_i[b, j] > -np.inf:
                continue  # dead, or a finished beam without a score (not a state the step produces)
            if fin_i[b, j]:
                cands.append((float(cum_i[b, j]), j * W, j, None))  # itself; its lists are not looked at
                continue
            row = b * W + j
            norm = 0.0
            if W > 1:
                norm = float(np.float64(lse_max[row])) + math.log(float(np.float64(lse_sum[row])))
            surv = path_ref.survivors(seq_i[b, j, :hep_i[b, j] + 1], val[row], ids0[row], W)
            if not surv:
                status[b] |= path_ref.NO_CANDIDATE
            for rank, (item, v, _) in enumerate(surv):
                cands.append((float(cum_i[b, j]) + (float(np.float64(v)) - norm), j * W + rank, j, item))
        cands.sort(key=lambda c: (-c[0], c[1]))
        open_beam = False
        for t in range(W):
            if t >= len(cands):  # dead beam: window and hep of input beam 0, empty path
                seq_o[b, t], hep_o[b, t] = seq_i[b, 0], hep_i[b, 0]
                continue
            score, _, j, item = cands[t]
            if item is None:  # a finished beam that survived: whole and unchanged
                seq_o[b, t], hep_o[b, t], cum_o[b, t], fin_o[b, t] = seq_i[b, j], hep_i[b, j], cum_i[b, j], 1
                paths_o[b, t] = paths_i[b, j, :P]
                continue
            seq_o[b, t], hep_o[b, t] = path_ref.advance(seq_i[b, j], int(hep_i[b, j]), item)
            paths_o[b, t, :step] = paths_i[b, j, :step]
            paths_o[b, t, step] = item
            cum_o[b, t] = score
            fin_o[b, t] = 1 if item == int(seq_i[b, j, L - 1]) else 0
            open_beam |= not fin_o[b, t]
        done_o[b] = 1 if (not open_beam or (stop_rule == STOP_BEST and fin_o[b, 0])) else 0
    return (seq_o, hep_o, cum_o, paths_o, fin_o), done_o, status


def beam_search_until(oracle_np, sd, cfg, seqs, users, max_path_len, beam, stop_rule, gap_len=0, k_cand=100, cache=None):
    """The whole search on the CPU oracle's decode and scoring (modelled on oracle_np.beam_search, one user at a time, every
    step through beam_step_until above).  A user stops being stepped once it is done -- which, a done user being copied
    through, is what any check interval gives.  `cache`: a dict shared between calls on the same model, (user, window, hep)
    -> the row's (val, ids0, max, sumexp); the two stop rules walk mostly the same windows.
    Returns (paths float32 [B, W, P], scores float64 [B, W], fin int32 [B, W], steps int [B]: the steps a user was live)."""
    seqs = np.asarray(seqs, dtype=np.int64)
    B, L = seqs.shape
    W, P = beam, max_path_len
    Wt, bias = sd["project.weight"], sd["project.bias"]
    cache = {} if cache is None else cache
    paths = np.zeros((B, W, P), dtype=np.float32)
    scores = np.zeros((B, W), dtype=np.float64)
    fins = np.zeros((B, W), dtype=np.int32)
    steps = np.zeros(B, dtype=np.int64)

    def row_lists(user, win, hep):
        key = (int(user), win.tobytes(), int(hep))
        if key not in cache:
            x, _ = oracle_np.decode(sd, cfg, win, user)
            s = oracle_np.score_chain(x[hep], Wt, bias)
            vals, ids0 = oracle_np.topk(s, k_cand)
            cache[key] = (vals, ids0) + tuple(oracle_np.max_sumexp(s))
        return cache[key]

    for r in range(B):
        seq = np.repeat(seqs[r][None, None], W, axis=1)
        hep = np.full((1, W), L - (gap_len + 1) - 1, dtype=np.int32)
        cum = np.full((1, W), -np.inf)
        cum[0, 0] = 0.0
        state = (seq, hep, cum, np.zeros((1, W, P), dtype=np.float32), np.zeros((1, W), dtype=np.int32))
        done = np.zeros(1, dtype=np.int32)
        for step in range(P):
            if done[0]:
                break
            val = np.zeros((W, k_cand), dtype=np.float32)
            ids0 = np.full((W, k_cand), -1, dtype=np.int64)
            lmax, lsum = np.zeros(W), np.ones(W)
            for j in range(W):
                if state[2][0, j] > -np.inf and not state[4][0, j]:
                    v, i, m, se = row_lists(users[r], state[0][0, j], state[1][0, j])
                    val[j, :len(v)], ids0[j, :len(i)], lmax[j], lsum[j] = v, i, m, se
            state, done, _ = beam_step_until(state, done, val, ids0, lmax, lsum, step, P, stop_rule)
            steps[r] += 1
        paths[r], scores[r], fins[r] = state[3][0], state[2][0], state[4][0]
    return paths, scores, fins, steps
