"""Test-side restatement of the lookahead choice (include/irs_hip.h, "lookahead choice": irs_bind_lookahead, irs_lookahead_expand,
irs_lookahead_choose), in plain numpy and Python loops, written from the header text on top of path_ref and exclusion_ref.

While a lookahead is bound a greedy step collects the first min(k_c, available) survivors of the row's ranked list (the list as
the plain step sees it: window, bound list and path struck), builds for each the window the row would have after choosing it
(path_ref.advance), asks a scorer for the target's log-probability on every child, and takes the child with the highest value:
ties go to the better rank, a NaN never wins, the target itself wins outright.  The list is then rewritten to the chosen
candidate alone and the plain step (path_ref.path_step) takes it."""
import math

import numpy as np

import exclusion_ref
import path_ref

MAX_KC = 32
NINF = np.float32(-np.inf)


def expand(seq, hep, users, val, ids0, k_c, excl=None, n_item=None, paths=None, step=0, no_repeat=False, user_of=None, fin=None):
    """irs_lookahead_expand: (child_seq [M k_c, L], child_hep [M k_c], child_user [M k_c], child_target0 [M k_c], cand_ids0
    [M, k_c], cand_val [M, k_c]).  Row r reads the list of user_of[r] (default r) and path row user_of[r]."""
    seq, hep = np.asarray(seq, dtype=np.int64), np.asarray(hep, dtype=np.int32)
    M, L = seq.shape
    user_of = range(M) if user_of is None else user_of
    c_seq = np.zeros((M * k_c, L), dtype=np.int64)
    c_hep = np.zeros(M * k_c, dtype=np.int32)
    c_user = np.zeros(M * k_c, dtype=np.int64)
    c_tgt = np.zeros(M * k_c, dtype=np.int64)
    c_ids = np.full((M, k_c), -1, dtype=np.int64)
    c_val = np.full((M, k_c), NINF, dtype=np.float32)
    for r in range(M):
        v, i = np.asarray(val[r]), np.asarray(ids0[r])
        if excl is not None or no_repeat:
            u = user_of[r]
            gone = exclusion_ref.hidden(None if excl is None else excl[u], n_item, None if paths is None else paths[u], step, no_repeat)
            v, i = exclusion_ref.strike(v, i, gone)
        surv = [] if (fin is not None and fin[r]) else path_ref.survivors(seq[r, :hep[r] + 1], v, i, k_c)
        for j in range(k_c):
            c = r * k_c + j
            c_user[c] = 0 if users is None else users[r]
            c_tgt[c] = seq[r, L - 1] - 1
            if j < len(surv):
                c_seq[c], c_hep[c] = path_ref.advance(seq[r], int(hep[r]), surv[j][0])
                c_ids[r, j], c_val[r, j] = surv[j][0] - 1, surv[j][1]
            else:
                c_seq[c], c_hep[c] = seq[r], hep[r]
    return c_seq, c_hep, c_user, c_tgt, c_ids, c_val


def lp_values(ts, mx, sm, cand_ids0):
    """The values the choose step compares: (float)((double)ts - ((double)max + log((double)sumexp))), -inf without a candidate."""
    ts, mx, sm = (np.asarray(a, dtype=np.float32).reshape(np.shape(cand_ids0)) for a in (ts, mx, sm))
    out = np.full(np.shape(cand_ids0), NINF, dtype=np.float32)
    for idx in np.ndindex(*np.shape(cand_ids0)):
        if cand_ids0[idx] >= 0:
            with np.errstate(all="ignore"):
                out[idx] = np.float32(np.float64(ts[idx]) - (np.float64(mx[idx]) + math.log(np.float64(sm[idx]))))
    return out


def better(v, best):
    """Does v replace best?  Strictly greater only; a NaN never replaces, anything but a NaN replaces a NaN."""
    return bool(v > best) or bool(best != best and v == v)


def choose_index(lp_row, items, target):
    """Index into `items` (the row's candidates, 1-based, rank order, the live ones only) of the choice; -1 without one."""
    if len(items) == 0:
        return -1
    for j, it in enumerate(items):
        if int(it) == int(target):
            return j
    best = 0
    for j in range(1, len(items)):
        if better(lp_row[j], lp_row[best]):
            best = j
    return best


def choose(seq, cand_ids0, cand_val, lp, val, ids0, fin=None):
    """irs_lookahead_choose on emitted lp: (val, ids0, choice) with the lists rewritten, on copies."""
    val, ids0 = np.array(val, dtype=np.float32), np.array(ids0, dtype=np.int64)
    M, k = ids0.shape
    choice = np.full(M, -1, dtype=np.int32)
    for r in range(M):
        if fin is not None and fin[r]:
            continue
        n = int((np.asarray(cand_ids0[r]) >= 0).sum())
        items = [int(i) + 1 for i in cand_ids0[r][:n]]
        c = choose_index(lp[r], items, int(seq[r][-1]))
        choice[r] = c
        if c < 0:
            continue
        val[r, 0], ids0[r, 0] = cand_val[r][c], cand_ids0[r][c]
        if k > 1:
            val[r, 1], ids0[r, 1] = NINF, -1
    return val, ids0, choice


def step(seq, hep, users, val, ids0, i, paths, status, k_c, scorer, excl=None, n_item=None, no_repeat=False, user_of=None, fin=None):
    """One bound step on copies: expand, `scorer(child_seq, child_hep, child_user, child_target0) -> (ts, mx, sm)` each [M k_c],
    choose, then the plain step on the rewritten lists.  `paths` rows are the caller's (user_of maps a row to its user; the
    step itself writes row r).  Returns (seq, hep, paths, status, record) with record = dict(items int32 [M, k_c] 1-based,
    lp [M, k_c], choice [M], child_seq, child_hep)."""
    M = len(seq)
    user_of = range(M) if user_of is None else user_of
    c_seq, c_hep, c_user, c_tgt, c_ids, c_val = expand(seq, hep, users, val, ids0, k_c, excl, n_item, paths, i, no_repeat, user_of, fin)
    ts, mx, sm = scorer(c_seq, c_hep, c_user, c_tgt)
    lp = lp_values(ts, mx, sm, c_ids)
    v2, i2, choice = choose(seq, c_ids, c_val, lp, val, ids0, fin)
    if excl is not None or no_repeat:
        out = exclusion_ref.path_step(seq, hep, v2, i2, i, paths, status, excl, n_item, no_repeat, user_of=user_of)
    else:
        out = path_ref.path_step(seq, hep, v2, i2, i, paths, status)
    rec = dict(items=(c_ids + 1).astype(np.int32), lp=lp, choice=choice, child_seq=c_seq, child_hep=c_hep)
    return out + (rec,)


def search(seq, hep, users, P, k_c, ranker, scorer, excl=None, n_item=None, no_repeat=False, until=False):
    """The greedy loop with a bound lookahead, stepped on the host: `ranker(seq, hep, users) -> (val, ids0)`.  until: a user is
    frozen after the step that chose its target, its tail (path and record) zero.
    Returns (paths [B, P], seq, hep, status, items [B, P, k_c], lp [B, P, k_c], choice [B, P])."""
    seq, hep = np.array(seq, dtype=np.int64), np.array(hep, dtype=np.int32)
    B, L = seq.shape
    paths, status = np.zeros((B, P), dtype=np.float32), np.zeros(B, dtype=np.int32)
    items, lps = np.zeros((B, P, k_c), dtype=np.int32), np.zeros((B, P, k_c), dtype=np.float32)
    choice = np.full((B, P), -1, dtype=np.int32)
    fin = np.zeros(B, dtype=np.int32)
    for i in range(P):
        if until and fin.all():
            break
        val, ids0 = ranker(seq, hep, users)
        s2, h2, p2, st2, rec = step(seq, hep, users, val, ids0, i, paths, status, k_c, scorer, excl, n_item, no_repeat, fin=fin)
        live = fin == 0
        seq[live], hep[live], paths[live], status[live] = s2[live], h2[live], p2[live], st2[live]
        items[live, i], lps[live, i], choice[live, i] = rec["items"][live], rec["lp"][live], rec["choice"][live]
        if until:
            fin |= (live & (paths[:, i] == seq[:, L - 1])).astype(np.int32)
    return paths, seq, hep, status, items, lps, choice
