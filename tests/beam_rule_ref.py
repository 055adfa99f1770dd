"""Test-side restatement of the beam rule (include/irs_hip.h, "beam rule": irs_set_beam_rule, irs_beam_step_ruled), in plain
numpy / float64 and Python loops, written from the header on top of path_ref / beam_until_ref (the step), beam_trace_ref (the
links), arrival_ref (the clauses, lp_target's expression, admissibility) and exclusion_ref (the bound list).

One step on explicit inputs.  A live unfinished beam whose rule fires contributes the target alone (index parent * W + 0, list
value ts); every candidate keeps its acceptance score and is ORDERED by key = score + lambda * lp_target(parent); a finished
beam re-enters with bonus 0.  With lambda = 0 the key is the score: no product is formed."""
import math

import numpy as np

import arrival_ref
import beam_trace_ref
import exclusion_ref
import path_ref

DEAD, COPY = beam_trace_ref.DEAD, beam_trace_ref.COPY
NO_CANDIDATE, OFFERED = path_ref.NO_CANDIDATE, arrival_ref.OFFERED
STOP_ALL, STOP_BEST = 0, 1


def bonus(ts, mx, sm, rk):
    """lp_target of a parent row as the key takes it: arrival_ref.lp_value, 0 without a target or where it is NaN."""
    lp = arrival_ref.lp_value(ts, mx, sm, rk)
    return 0.0 if (int(rk) == 0 or np.isnan(lp)) else float(lp)


def key_of(score, weight, bon):
    """score + (double)weight * (double)bonus; weight == 0 forms no product (0 * -inf)."""
    w = float(np.float32(weight))
    with np.errstate(all="ignore"):
        return float(score) if not w > 0 else float(np.float64(score) + np.float64(w) * np.float64(bon))


def candidates(state_in, b, val, ids0, lse_max, lse_sum, sweep, rule, n_item, step, excl=None, no_repeat=False, offer=None,
               user_of=None):
    """User b's candidates [(key, score, index, parent, item or None, list value)] in index order, the beam rows that fired, and
    whether some live unfinished beam found nothing.  state_in: four arrays (plain) or five (fin last)."""
    seq_i, hep_i, cum_i, paths_i = (np.asarray(a) for a in state_in[:4])
    fin_i = np.asarray(state_in[4]) if len(state_in) == 5 else np.zeros(cum_i.shape, dtype=np.int32)
    _, W, L = seq_i.shape
    mx, sm, ts, rank = sweep
    rank_max, lp_min, weight = rule
    u = b if user_of is None else int(user_of[b])
    out, fired, starved = [], [], False
    for j in range(W):
        cj = float(cum_i[b, j])
        if not cj > -np.inf:
            continue
        if fin_i[b, j]:
            out.append((cj, cj, j * W, j, None, np.float32(0)))  # itself: bonus 0
            continue
        row = b * W + j
        norm = 0.0
        if W > 1:
            norm = float(np.float64(lse_max[row])) + math.log(float(np.float64(lse_sum[row])))
        bon = bonus(ts[row], mx[row], sm[row], rank[row])
        window = seq_i[b, j, :int(hep_i[b, j]) + 1]
        t = int(seq_i[b, j, L - 1])
        excl_row = None if excl is None else excl[u]
        fire = arrival_ref.fires(rank[row], arrival_ref.lp_value(ts[row], mx[row], sm[row], rank[row]), rank_max, lp_min)
        fire = fire and arrival_ref.admissible(t, window, n_item, excl_row, paths_i[b, j], step, no_repeat)
        if fire and offer is not None:
            fire = (t - 1) in set(int(i) for i in offer)
        if fire:
            fired.append(j)
            s = cj + (float(np.float64(np.float32(ts[row]))) - norm)
            out.append((key_of(s, weight, bon), s, j * W, j, t, np.float32(ts[row])))
            continue
        v_row, i_row = val[row], ids0[row]
        if excl is not None or no_repeat:
            v_row, i_row = exclusion_ref.strike(v_row, i_row, exclusion_ref.hidden(excl_row, n_item, paths_i[b, j], step, no_repeat))
        surv = path_ref.survivors(window, v_row, i_row, W)
        starved |= not surv
        for r, (item, v, _) in enumerate(surv):
            s = cj + (float(np.float64(v)) - norm)
            out.append((key_of(s, weight, bon), s, j * W + r, j, item, np.float32(v)))
    return out, fired, starved


def ruled_step(state_in, done, val, ids0, lse_max, lse_sum, sweep, rule, n_item, step, P, stop_rule=None, excl=None,
               no_repeat=False, offer=None, status=None, user_of=None):
    """One ruled step.  done None: the plain form (four-array state); else the until form (five arrays, fin last).
    sweep = (mx, sm, ts, rank) [B * W]; rule = (rank_max, lp_min, weight) -- rank_max 0 and lp_min None / NaN / > 0 turn a clause
    off; excl [users, E] 0-based (-1 unused); offer: the 0-based ids of a bound offer set; user_of[b]: the bound user of b.
    Returns (state_out, link, link_val, done_out or None, status [B], offered bool [B, W] by INPUT beam row)."""
    until = done is not None
    seq_i, hep_i, cum_i, paths_i = (np.asarray(a) for a in state_in[:4])
    fin_i = np.asarray(state_in[4]) if until else None
    B, W, L = seq_i.shape
    rule = (int(rule[0] or 0), np.float32(np.nan if rule[1] is None else rule[1]), rule[2])
    seq_o, hep_o = np.zeros_like(seq_i), np.zeros_like(hep_i)
    cum_o = np.full((B, W), -np.inf, dtype=np.float64)
    paths_o = np.zeros((B, W, P), dtype=np.float32)
    fin_o = np.zeros((B, W), dtype=np.int32)
    done_o = np.array(done, dtype=np.int32) if until else None
    status = np.zeros(B, dtype=np.int32) if status is None else np.array(status, dtype=np.int32)
    link = np.full((B, W), DEAD, dtype=np.int32)
    link_val = np.zeros((B, W), dtype=np.float32)
    offered = np.zeros((B, W), dtype=bool)
    for b in range(B):
        if until and done_o[b]:
            seq_o[b], hep_o[b], cum_o[b], paths_o[b], fin_o[b] = seq_i[b], hep_i[b], cum_i[b], paths_i[b, :, :P], fin_i[b]
            link[b] = COPY | np.arange(W)
            continue
        cands, fired, starved = candidates(state_in, b, val, ids0, lse_max, lse_sum, sweep, rule, n_item, step, excl, no_repeat,
                                           offer, user_of)
        offered[b, fired] = True
        if fired:
            status[b] |= OFFERED
        if starved:
            status[b] |= NO_CANDIDATE
        cands.sort(key=lambda c: (-c[0], c[2]))
        open_beam = False
        for t in range(W):
            if t >= len(cands):
                seq_o[b, t], hep_o[b, t] = seq_i[b, 0], hep_i[b, 0]
                continue
            _, score, _, j, item, v = cands[t]
            if item is None:
                seq_o[b, t], hep_o[b, t], cum_o[b, t], fin_o[b, t] = seq_i[b, j], hep_i[b, j], cum_i[b, j], 1
                paths_o[b, t] = paths_i[b, j, :P]
                link[b, t] = COPY | j
                continue
            seq_o[b, t], hep_o[b, t] = path_ref.advance(seq_i[b, j], int(hep_i[b, j]), item)
            paths_o[b, t, :step] = paths_i[b, j, :step]
            paths_o[b, t, step] = item
            cum_o[b, t] = score
            link[b, t], link_val[b, t] = j, v
            fin_o[b, t] = 1 if (until and item == int(seq_i[b, j, L - 1])) else 0
            open_beam |= not fin_o[b, t]
        if until:
            done_o[b] = 1 if (not open_beam or (stop_rule == STOP_BEST and fin_o[b, 0])) else 0
    state_out = (seq_o, hep_o, cum_o, paths_o) + ((fin_o,) if until else ())
    return state_out, link, link_val, done_o, status, offered


def min_key_gap(state_in, done, val, ids0, lse_max, lse_sum, sweep, rule, n_item, step, **kw):
    """The smallest |key difference| over each user's pairs of candidates that include one of its W survivors (inf where a user
    has fewer than two candidates): the precondition of an exact comparison with a device whose log() may differ in its last
    bits."""
    B, W = np.asarray(state_in[2]).shape
    rule = (int(rule[0] or 0), np.float32(np.nan if rule[1] is None else rule[1]), rule[2])
    gap = np.inf
    for b in range(B):
        if done is not None and done[b]:
            continue
        cands, _, _ = candidates(state_in, b, val, ids0, lse_max, lse_sum, sweep, rule, n_item, step, **kw)
        cands.sort(key=lambda c: (-c[0], c[2]))
        for a in range(min(W, len(cands))):
            for c in range(len(cands)):
                if c == a:
                    continue
                with np.errstate(invalid="ignore"):
                    d = abs(cands[a][0] - cands[c][0])
                gap = min(gap, d if not np.isnan(d) else np.inf)
    return gap


def replay_offered(paths, lp_target, rank_target, targets, rank_max, lp_min):
    """(offered bool [B, W], arrival_step int64 [B, W]) from recorded arrays alone: a beam was offered at step i exactly when
    paths[i] == target (its first such i) and a clause holds on (rank_target[i], lp_target[i])."""
    paths = np.asarray(paths)
    B, W, P = paths.shape
    offered = np.zeros((B, W), dtype=bool)
    at = np.full((B, W), -1, dtype=np.int64)
    for b in range(B):
        for j in range(W):
            pos = np.where(paths[b, j] == targets[b])[0]
            if len(pos):
                i = int(pos[0])
                at[b, j] = i
                offered[b, j] = arrival_ref.fires(rank_target[b, j, i], lp_target[b, j, i], rank_max or 0, np.float32(np.nan if lp_min is None else lp_min))
    return offered, at


def search(oracle_np, sd, cfg, seqs, users, hep0, W, P, rule, stop_rule=None, k=100, cache=None):
    """The whole search on the CPU oracle's decode and exact scoring, every step through ruled_step, with its trace: column
    `step` of a child is arrival_ref.lp_value on the PARENT's sweep values (lp_item from the list value the child took), carried
    by beam_trace_ref.carry.  `cache`: a dict shared between calls on the same model, (user, window, hep) -> the row's lists and
    sweep values.  Returns dict(paths, scores, fin (None: plain), status, offered [B, W] by OUTPUT beam (replay_offered on the
    recorded arrays), offered_own (the steps' own fired bits, carried along the links), arrays = (lp_item, lp_target, rank_target) [B, W, P], steps int [B]: the steps a user was not done on entry)."""
    import path_trace_ref
    seqs = np.asarray(seqs, dtype=np.int64)
    until = stop_rule is not None
    B = len(seqs)
    state = beam_trace_ref.initial_state(seqs, hep0, W, P, until)
    done = np.zeros(B, dtype=np.int32) if until else None
    arrays = (np.zeros((B, W, P), dtype=np.float32), np.zeros((B, W, P), dtype=np.float32), np.zeros((B, W, P), dtype=np.int32))
    status = np.zeros(B, dtype=np.int32)
    steps = np.zeros(B, dtype=np.int64)
    Wt, bias = sd["project.weight"], sd["project.bias"]
    cache = {} if cache is None else cache
    n_item = Wt.shape[0]
    own = np.zeros((B, W), dtype=bool)
    for step in range(P):
        val = np.zeros((B * W, k), dtype=np.float32)
        ids0 = np.full((B * W, k), -1, dtype=np.int64)
        lmax, lsum = np.zeros(B * W), np.ones(B * W)  # (the step's lse pair as beam_until_ref keeps it; the sweep's is float32)
        ts, rank = np.zeros(B * W, dtype=np.float32), np.zeros(B * W, dtype=np.int32)
        for b in range(B):
            if until and done[b]:
                continue
            steps[b] += 1
            for j in range(W):
                if (until and state[4][b, j]) or not state[2][b, j] > -np.inf:
                    continue
                win, hep = state[0][b, j], int(state[1][b, j])
                key = (int(users[b]), win.tobytes(), hep)
                if key not in cache:
                    x, _ = oracle_np.decode(sd, cfg, win, users[b])
                    logits = oracle_np.score_chain(x[hep], Wt, bias)
                    t = int(win[-1])
                    cache[key] = oracle_np.topk(logits, k) + tuple(oracle_np.max_sumexp(logits)) + (
                        logits[t - 1] if 1 <= t <= n_item else np.float32(0),
                        path_trace_ref.target_rank(logits, win[:hep + 1], t) if 1 <= t <= n_item else 0)
                v, i, m, se, tsv, rk = cache[key]
                row = b * W + j
                val[row, :len(v)], ids0[row, :len(i)], lmax[row], lsum[row], ts[row], rank[row] = v, i, m, se, tsv, rk
        state_in = state
        mx32, sm32 = lmax.astype(np.float32), lsum.astype(np.float32)
        state, link, link_val, done, status, fired = ruled_step(state_in, done, val, ids0, lmax, lsum, (mx32, sm32, ts, rank), rule, n_item,
                                                            step, P, stop_rule, status=status)
        new_cols = [[None] * W for _ in range(B)]
        for b in range(B):
            for t in range(W):
                l = int(link[b, t])
                if l >= 0 and not l & COPY:
                    row = b * W + l
                    new_cols[b][t] = (arrival_ref.lp_value(link_val[b, t], mx32[row], sm32[row], 1),
                                      arrival_ref.lp_value(ts[row], mx32[row], sm32[row], rank[row]), rank[row])
        arrays = beam_trace_ref.carry(arrays, link, new_cols, step)
        was, own = own, np.zeros((B, W), dtype=bool)  # the statement's own bits follow the beams through the links
        for b in range(B):
            for t in range(W):
                l = int(link[b, t])
                if l >= 0:
                    own[b, t] = was[b, l & (COPY - 1)] or (not l & COPY and fired[b, l])
    targets = seqs[:, -1]
    offered, _ = replay_offered(state[3], arrays[1], arrays[2], targets, rule[0], rule[1])
    return dict(paths=state[3], scores=state[2], fin=state[4] if until else None, status=status, offered=offered, offered_own=own,
                arrays=arrays, steps=steps)
