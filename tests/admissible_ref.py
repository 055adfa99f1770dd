"""Test-side restatement of the admissible rank (include/irs_hip.h, "admissible rank"), in plain numpy, built on
exclusion_ref.hidden and path_trace_ref.target_rank: written from the header's text, not from the kernel.

rank_adm = 1 + #{ j in U \\ H, j != t-1 : (e_j, j) ranks before (e_{t-1}, t-1) }: the trace's rank with "the window" read as
window + list + path, and every item outside a bound offer set struck as well."""
import numpy as np

import arrival_ref
import exclusion_ref
import path_ref
import path_trace_ref


def hidden(excl_row, n_item, path_row=None, step=0):
    """H without the window, 1-based: the valid ids of the user's list and the non-zero path entries [0, step) (the caller passes
    a path only where the step would hide it: under no_repeat, or in the standalone call)."""
    return exclusion_ref.hidden(excl_row, n_item, path_row, step, no_repeat=path_row is not None)


def target_rank_admissible(logits, window, target, hidden, offer=None):
    """logits: the row's exact float32 scores over the whole catalog; window: seq[row][0 .. hep] (pads are 0); target: 1-based;
    hidden: a set of 1-based items (hidden() above); offer: the offer set's valid 0-based ids, None for the whole catalog.
    0 without a target.  The target's own membership in window, hidden or offer does not matter."""
    n_item = len(logits)
    gone = {int(v) for v in window if int(v) != 0} | {int(h) for h in hidden}
    if offer is not None:
        inside = {int(j) + 1 for j in np.asarray(offer).reshape(-1) if 0 <= int(j) < n_item}
        gone |= set(range(1, n_item + 1)) - inside
    return path_trace_ref.target_rank(logits, sorted(gone), target)


def rows(logits, seq, hep, excl=None, paths=None, step=0, offer=None, user_of=None):
    """target_rank_admissible over the rows of one call: row m reads list user_of[m] (default m) and its own path row."""
    M, L = seq.shape
    out = np.zeros(M, dtype=np.int32)
    for m in range(M):
        u = m if user_of is None else int(user_of[m])
        h = hidden(None if excl is None else excl[u], logits.shape[1], None if paths is None else paths[m], step)
        out[m] = target_rank_admissible(logits[m], seq[m, :int(hep[m]) + 1], seq[m, L - 1], h, offer)
    return out


def slate_position(logits, window, target, hidden, offer=None):
    """The target's 0-based position among the admissible items of U in the library's order, None where it is not admissible."""
    n_item, t = len(logits), int(target)
    gone = {int(v) for v in window if int(v) != 0} | {int(h) for h in hidden}
    inside = set(range(1, n_item + 1)) if offer is None else {int(j) + 1 for j in np.asarray(offer).reshape(-1) if 0 <= int(j) < n_item}
    if t < 1 or t > n_item or t in gone or t not in inside:
        return None
    key = path_ref.order_key(logits)
    order = sorted((j for j in range(n_item) if j + 1 in inside and j + 1 not in gone), key=lambda j: (-int(key[j]), j))
    return order.index(t - 1)


def replay(seq, hep, paths, trace, rank_adm, rank_max, lp_min, n_item, excl=None, no_repeat=False, offer=None):
    """arrival_ref.replay for a rule on the ADMISSIBLE rank: the rank clause reads the recorded rank_adm, the probability clause
    the recorded lp_target; the target must be admissible under the step's own test and inside a bound offer set.  Returns
    (paths, (lp_item, lp_target, rank_target, rank_adm), n_steps, arrived, offered), everything cut behind the arrival."""
    paths = np.array(paths, dtype=np.float32)
    lp_item, lp_target, rank_target = (np.array(a) for a in trace)
    rank_adm = np.array(rank_adm)
    inside = None if offer is None else {int(j) + 1 for j in np.asarray(offer).reshape(-1) if 0 <= int(j) < n_item}
    B, P = paths.shape
    n_steps = np.full(B, P, dtype=np.int64)
    arrived, offered = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    for b in range(B):
        win, he = np.array(seq[b]), int(hep[b])
        t = int(win[-1])
        for i in range(P):
            fire = arrival_ref.fires(rank_adm[b, i], lp_target[b, i], rank_max, lp_min) and (inside is None or t in inside) and \
                arrival_ref.admissible(t, win[:he + 1], n_item, None if excl is None else excl[b], paths[b], i, no_repeat)
            if fire or int(paths[b, i]) == t:
                offered[b], arrived[b], n_steps[b] = fire, True, i + 1
                if fire:
                    paths[b, i], lp_item[b, i] = t, lp_target[b, i]
                for a in (paths, lp_item, lp_target, rank_target, rank_adm):
                    a[b, i + 1:] = 0
                break
            if int(paths[b, i]) == 0:
                continue
            win, he = path_ref.advance(win, he, int(paths[b, i]))
    return paths, (lp_item, lp_target, rank_target, rank_adm), n_steps, arrived, offered


def ml1m_lists(B, n_item, seed, longest=None, width=None):
    """Exclusion lists shaped like ml-1m histories scaled to the catalog: lengths log-normal with the median at 93 / 3415 of the
    catalog and the longest at 2276 / 3415 of it; 0-based ids, -1 behind a list, a repeated id in every list of two or more."""
    g = np.random.default_rng(seed)
    med, top = max(2, round(93 * n_item / 3415)), max(3, round(2276 * n_item / 3415)) if longest is None else longest
    n = np.clip(np.round(med * np.exp(g.standard_normal(B))).astype(np.int64), 1, top)
    n[0] = top
    width = int(n.max()) + 1 if width is None else width
    out = np.full((B, width), -1, dtype=np.int64)
    for b in range(B):
        ids = g.permutation(n_item)[:n[b]]
        out[b, :n[b]] = ids
        if n[b] >= 2:
            out[b, n[b]] = ids[0]  # a duplicate
    return out
