"""Test-side restatement of the beam trace (include/irs_hip.h, "beam trace"), in plain numpy and Python loops, written from the
header: a step of path_ref.beam_step / beam_until_ref.beam_step_until, the link of every output beam found the slow way from
the same candidate order, path_trace_ref.step_values on the PARENT's input row, and the recorded columns carried by parent.

The values are path_trace_ref's -- float64 log-sum-exp, rounded to float32 once -- so a device result is compared with them
within a tolerance; ranks and links are exact on exact logits."""
import math

import numpy as np

import beam_until_ref
import path_ref
import path_trace_ref

DEAD, COPY = -1, 256  # IRS_BEAM_LINK_DEAD, IRS_BEAM_LINK_COPY


def step_links(state_in, done, val, ids0, lse_max, lse_sum, until):
    """(link int32 [B, W], link_val float32 [B, W], item int64 [B, W]) of one step: DEAD, the parent p of a child (with the
    list value and the item it took), or COPY | p -- a surviving finished beam, or beam p = t of a user that is done on entry.
    The candidate order is the steps' own: score descending, then index parent * W + rank in the parent."""
    seq_i, hep_i, cum_i = (np.asarray(a) for a in state_in[:3])
    fin_i = np.asarray(state_in[4]) if until else np.zeros(cum_i.shape, dtype=np.int32)
    B, W, _ = seq_i.shape
    link = np.full((B, W), DEAD, dtype=np.int32)
    link_val = np.zeros((B, W), dtype=np.float32)
    item = np.zeros((B, W), dtype=np.int64)
    for b in range(B):
        if until and done[b]:
            link[b] = COPY | np.arange(W)
            continue
        cands = []  # (score, index, parent, item or None, list value)
        for j in range(W):
            if not cum_i[b, j] > -np.inf:
                continue
            if fin_i[b, j]:
                cands.append((float(cum_i[b, j]), j * W, j, None, 0.0))
                continue
            row = b * W + j
            norm = 0.0
            if W > 1:
                norm = float(np.float64(lse_max[row])) + math.log(float(np.float64(lse_sum[row])))
            surv = path_ref.survivors(seq_i[b, j, :hep_i[b, j] + 1], val[row], ids0[row], W)
            for rank, (it, v, _) in enumerate(surv):
                cands.append((float(cum_i[b, j]) + (float(np.float64(v)) - norm), j * W + rank, j, it, v))
        cands.sort(key=lambda c: (-c[0], c[1]))
        for t, (_, _, j, it, v) in enumerate(cands[:W]):
            if it is None:
                link[b, t] = COPY | j
            else:
                link[b, t], link_val[b, t], item[b, t] = j, v, it
    return link, link_val, item


def carry(arrays, link, new_cols, step):
    """The three [B, W, ld] arrays after the links of one step: a child takes its parent's columns [0, step), then
    new_cols[b][t] = (lp_item, lp_target, rank_target) at column step, then zeros; a copy takes its parent's whole row; a dead
    slot reads zero.  A slot that copies itself is left alone."""
    out = [np.array(a) for a in arrays]
    B, W = link.shape
    for b in range(B):
        for t in range(W):
            l = int(link[b, t])
            if l == (COPY | t):
                continue
            for a, o, c in zip(arrays, out, range(3)):
                o[b, t] = 0
                if l == DEAD:
                    continue
                if l & COPY:
                    o[b, t] = a[b, l & (COPY - 1)]
                else:
                    o[b, t, :step] = a[b, l, :step]
                    o[b, t, step] = new_cols[b][t][c]
    return tuple(out)


def traced_step(arrays, state_in, done, val, ids0, lse_max, lse_sum, logits_of, step, P, stop_rule=None):
    """One step with its trace.  state: path_ref.beam_step's four arrays (stop_rule None), or beam_until_ref's five with
    done [B].  logits_of(row) -> the exact float32 logits [N] of input row b * W + j; it is asked for the parents of children
    only.  Returns (arrays_out, state_out, done_out, status, link, link_val)."""
    until = stop_rule is not None
    if until:
        state_out, done_out, status = beam_until_ref.beam_step_until(state_in, done, val, ids0, lse_max, lse_sum, step, P, stop_rule)
    else:
        state_out, status = path_ref.beam_step(state_in, val, ids0, lse_max, lse_sum, step, P)
        done_out = None
    link, link_val, item = step_links(state_in, done, val, ids0, lse_max, lse_sum, until)
    seq_i, hep_i = np.asarray(state_in[0]), np.asarray(state_in[1])
    B, W, L = seq_i.shape
    new_cols = [[None] * W for _ in range(B)]
    for b in range(B):
        for t in range(W):
            l = int(link[b, t])
            # the links say what the step itself did
            if l == DEAD:
                assert not state_out[2][b, t] > -np.inf and not state_out[3][b, t].any()
            elif l & COPY:
                p = l & (COPY - 1)
                assert np.array_equal(state_out[3][b, t], np.asarray(state_in[3])[b, p, :P]) and state_out[2][b, t] == state_in[2][b, p]
            else:
                assert state_out[3][b, t, step] == item[b, t]
                assert np.array_equal(state_out[3][b, t, :step], np.asarray(state_in[3])[b, l, :step])
                new_cols[b][t] = path_trace_ref.step_values(logits_of(b * W + l), seq_i[b, l, :int(hep_i[b, l]) + 1],
                                                            seq_i[b, l, L - 1], item[b, t])
    return carry(arrays, link, new_cols, step), state_out, done_out, status, link, link_val


def initial_state(seqs, hep0, W, P, until):
    """Beam 0 = the input window with score 0, the others dead copies (irs_beam_search's beam init)."""
    seqs = np.asarray(seqs, dtype=np.int64)
    B, L = seqs.shape
    seq = np.repeat(seqs[:, None, :], W, axis=1)
    hep = np.repeat(np.asarray(hep0, dtype=np.int32)[:, None], W, axis=1)
    cum = np.full((B, W), -np.inf)
    cum[:, 0] = 0.0
    state = (seq, hep, cum, np.zeros((B, W, P), dtype=np.float32))
    return state + (np.zeros((B, W), dtype=np.int32),) if until else state


def search(oracle_np, sd, cfg, seqs, users, hep0, W, P, k=100, stop_rule=None, ld=None):
    """The whole search with its trace on the CPU oracle's decode and exact scoring.  Returns (arrays (lp_item, lp_target,
    rank_target) [B, W, ld], paths [B, W, P], scores [B, W], fin [B, W] or None, links: the (link, link_val) of every step)."""
    until = stop_rule is not None
    ld = P if ld is None else ld
    state = initial_state(seqs, hep0, W, P, until)
    B = len(seqs)
    done = np.zeros(B, dtype=np.int32) if until else None
    arrays = (np.zeros((B, W, ld), dtype=np.float32), np.zeros((B, W, ld), dtype=np.float32), np.zeros((B, W, ld), dtype=np.int32))
    Wt, bias = sd["project.weight"], sd["project.bias"]
    links = []
    for step in range(P):
        logits = {}
        val = np.zeros((B * W, k), dtype=np.float32)
        ids0 = np.full((B * W, k), -1, dtype=np.int64)
        lmax, lsum = np.zeros(B * W), np.ones(B * W)
        for b in range(B):
            for j in range(W):
                if (until and (done[b] or state[4][b, j])) or not state[2][b, j] > -np.inf:
                    continue
                row = b * W + j
                x, _ = oracle_np.decode(sd, cfg, state[0][b, j], users[b])
                logits[row] = oracle_np.score_chain(x[state[1][b, j]], Wt, bias)
                v, i = oracle_np.topk(logits[row], k)
                val[row, :len(v)], ids0[row, :len(i)] = v, i
                lmax[row], lsum[row] = oracle_np.max_sumexp(logits[row])
        arrays, state, done, _, link, link_val = traced_step(arrays, state, done, val, ids0, lmax, lsum, logits.__getitem__, step, P,
                                                             stop_rule)
        links.append((link, link_val))
    return arrays, state[3], state[2], (state[4] if until else None), links


def pick_beam_ref(paths, scores, lp_target, n_steps, targets):
    """beam_pick="target", the slow way: per user the live beam that contains the target at the earliest step (ties: the higher
    score, then the lower index); if none does, the live beam with the largest lp_target in its last recorded column (ties the
    same way); beam 0 if no beam is live."""
    B, W, _ = paths.shape
    out = np.zeros(B, dtype=np.int64)
    for b in range(B):
        live = [j for j in range(W) if scores[b, j] > -np.inf]
        if not live:
            continue
        hits = []
        for j in live:
            pos = np.where(paths[b, j] == targets[b])[0]
            if len(pos):
                hits.append((int(pos[0]), -float(scores[b, j]), j))
        if hits:
            out[b] = min(hits)[2]
            continue
        out[b] = min((-float(lp_target[b, j, max(int(n_steps[b, j]) - 1, 0)]), -float(scores[b, j]), j) for j in live)[2]
    return out
