"""Test-side restatement of the arrival rule (include/irs_hip.h, "arrival rule"), in plain numpy: the fire test, the list
rewrite, and the replay of a rule-off search (its paths and its trace) into what the rule-on search must return.  Written from
the header's text, not from the kernel."""
import numpy as np

import exclusion_ref
import path_ref

OFFERED = 16


def lp_value(ts, mx, sm, rk):
    """The float32 the trace stores as lp_target: (double)ts - ((double)max + log((double)sumexp)), 0 without a target."""
    if int(rk) == 0:
        return np.float32(0)
    with np.errstate(all="ignore"):
        return np.float32(np.float64(np.float32(ts)) - (np.float64(np.float32(mx)) + np.log(np.float64(np.float32(sm)))))


def clauses(rank_max, lp_min):
    """(rank clause on, probability clause on): rank_max >= 1; lp_min <= 0, -inf included, NaN and positive values off."""
    return int(rank_max) >= 1, bool(np.float32(lp_min) <= np.float32(0))


def fires(rk, lp, rank_max, lp_min):
    """The clauses alone (admissibility is the caller's): rk != 0 and (rk <= rank_max or lp >= lp_min); a NaN lp never fires."""
    rank_on, lp_on = clauses(rank_max, lp_min)
    if int(rk) == 0:
        return False
    if rank_on and int(rk) <= int(rank_max):
        return True
    return bool(lp_on and np.float32(lp) >= np.float32(lp_min))


def admissible(t, window, n_item, excl_row=None, path_row=None, step=0, no_repeat=False):
    """The step's own test for the target t: a catalog item outside window (= seq[row][0 .. hep]), the user's list and, under
    no_repeat, the path entries [0, step)."""
    t = int(t)
    if t < 1 or t > n_item:
        return False
    if t in set(int(v) for v in window):
        return False
    if excl_row is not None or no_repeat:
        row = excl_row if excl_row is not None else np.zeros(0, dtype=np.int64)
        if t in exclusion_ref.hidden(row, n_item, path_row, step, no_repeat):
            return False
    return True


def offer(seq, hep, mx, sm, ts, rank, val, ids0, status, rank_max, lp_min, n_item, fin=None, excl=None, no_repeat=False,
          paths=None, step=0, user_of=None):
    """irs_arrival_offer on copies: returns (val, ids0, status, fired).  excl [users, E] 0-based ids (-1 unused) and paths
    [users, ld] are looked up at user_of[row] (None: the identity)."""
    val, ids0, status = np.array(val, dtype=np.float32), np.array(ids0, dtype=np.int64), np.array(status, dtype=np.int32)
    M, k = val.shape
    L = seq.shape[1]
    fired = np.zeros(M, dtype=bool)
    for m in range(M):
        if fin is not None and fin[m]:
            continue
        if not fires(rank[m], lp_value(ts[m], mx[m], sm[m], rank[m]), rank_max, lp_min):
            continue
        u = m if user_of is None else int(user_of[m])
        if not admissible(seq[m, L - 1], seq[m, :int(hep[m]) + 1], n_item, None if excl is None else excl[u],
                          None if paths is None else paths[u], step, no_repeat):
            continue
        fired[m] = True
        val[m, 0], ids0[m, 0] = ts[m], int(seq[m, L - 1]) - 1
        if k > 1:
            val[m, 1], ids0[m, 1] = -np.inf, -1
        status[m] |= OFFERED
    return val, ids0, status, fired


def replay(seq, hep, paths, trace, rank_max, lp_min, n_item, excl=None, no_repeat=False):
    """What irs_generate_paths_until returns with the rule set, from a rule-off search of the same batch: paths [B, P] and trace
    = (lp_item, lp_target, rank_target) [B, P].  User b keeps its rule-off path up to the first step where the rule fires (on the
    recorded rank_target / lp_target, the target admissible against the window rebuilt from the path) or where the search chose
    the target itself; that step's entry is the target, everything behind it 0; the trace is cut there and, at a fired step,
    lp_item is lp_target.  Returns (paths, (lp_item, lp_target, rank_target), n_steps, arrived, offered)."""
    paths = np.array(paths, dtype=np.float32)
    lp_item, lp_target, rank_target = (np.array(a) for a in trace)
    B, P = paths.shape
    n_steps = np.full(B, P, dtype=np.int64)
    arrived, offered = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    for b in range(B):
        win, he = np.array(seq[b]), int(hep[b])
        t = int(win[-1])
        for i in range(P):
            fire = fires(rank_target[b, i], lp_target[b, i], rank_max, lp_min) and admissible(
                t, win[:he + 1], n_item, None if excl is None else excl[b], paths[b], i, no_repeat)
            if fire or int(paths[b, i]) == t:
                offered[b], arrived[b], n_steps[b] = fire, True, i + 1
                if fire:
                    paths[b, i], lp_item[b, i] = t, lp_target[b, i]
                for a in (paths, lp_item, lp_target, rank_target):
                    a[b, i + 1:] = 0
                break
            if int(paths[b, i]) == 0:  # a step without a candidate leaves the window as it is
                continue
            win, he = path_ref.advance(win, he, int(paths[b, i]))
    return paths, (lp_item, lp_target, rank_target), n_steps, arrived, offered


def until_stats(n_steps, arrived, P, check_every):
    """(steps_run, row_steps) of irs_generate_paths_until: a step runs on every row that was live at the last compaction."""
    B = len(n_steps)
    live, steps, row_steps = B, 0, 0
    for i in range(P):
        if live == 0:
            break
        steps += 1
        row_steps += live
        if (i + 1) % check_every or i + 1 == P:
            continue
        live = int(sum(1 for b in range(B) if not (arrived[b] and n_steps[b] <= i + 1)))
    return steps, row_steps


# ---------------------------------------------------------------- the model and the batches of the loop tests
WEIGHT_SEED = 1234
P = 8


def model_config():
    """n_item = 500, d = 32, 2 layers, L = 24: small enough for the CPU oracle to walk a batch in seconds."""
    from influentialrs_amd import synth
    return synth.make_config("tiny", n_item=500, emb_dim=32, n_heads=2, n_layers=2, max_len=24, ffn_dim=64, n_user=64)


def batch(B, seed):
    """(seq [B, L] with the target last, users [B], hep [B] = L - 2: every step shifts the window; histories of 4 to L - 1 items behind leading pads)."""
    from influentialrs_amd import synth
    cfg = model_config()
    seq = synth.random_windows(B, cfg.max_len, cfg.n_item, seed=seed, min_hist=4)
    return seq, (np.arange(B) % cfg.n_user).astype(np.int64), np.full(B, cfg.max_len - 2, dtype=np.int32)


def thresholds(trace, n_steps=None):
    """(rank_max, lp_min) of the replay tests from a rule-off trace: the median over users of the best rank_target over steps
    1 .. P - 1, and the median over users of the best lp_target over all steps."""
    _, lp_target, rank_target = trace
    rk = np.where(rank_target[:, 1:] > 0, rank_target[:, 1:], np.iinfo(np.int32).max).min(axis=1)
    return int(np.median(rk)), float(np.float32(np.median(lp_target.max(axis=1))))
