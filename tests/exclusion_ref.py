"""Test-side restatement of the bound exclusion set (include/irs_hip.h: irs_bind_exclusions), in plain numpy and Python loops,
written from the header text on top of path_ref, beam_until_ref and survivors_ref.

While a set is bound, every place that drops "the items in the row's window" drops window + the user's list + (no_repeat) the
row's own non-zero path entries [0, step).  For the steps that is the same as striking the listed and the path items from the
row's candidate list, in place and in order, and running the unbound step on what is left: a step only ever looks at the first
entries of the list that are outside the window.  The survivor pass also asks whether the list was full BEFORE anything was
struck, so it is restated on its own."""
import numpy as np

import beam_until_ref
import path_ref
import survivors_ref

MAX_EXCL = 4096


def hidden(excl_row, n_item, path_row=None, step=0, no_repeat=False):
    """The 1-based items a row never sees besides its window: the valid ids of its user's list (-1 marks an unused slot, ids
    >= n_item never match, duplicates count once) and, under no_repeat, the non-zero path entries [0, step)."""
    out = set()
    if excl_row is not None:
        out |= {int(i) + 1 for i in np.asarray(excl_row).reshape(-1) if 0 <= int(i) < n_item}
    if no_repeat and path_row is not None:
        out |= {int(p) for p in np.asarray(path_row)[:step] if p != 0}
    return out


def is_member(item, window, excl_row, n_item, path_row=None, step=0, no_repeat=False):
    """The membership test itself: window + list + path."""
    return int(item) in {int(v) for v in window} or int(item) in hidden(excl_row, n_item, path_row, step, no_repeat)


def sorted_row(excl_row, n_item, stride=None):
    """What the prepare launch writes for one user: (the valid ids ascending, INT64_MAX up to the next power of two, count)."""
    ids = sorted(int(i) for i in np.asarray(excl_row).reshape(-1) if 0 <= int(i) < n_item)
    n = len(np.asarray(excl_row).reshape(-1))
    if stride is None:
        stride = 1
        while stride < n:
            stride <<= 1
        stride = stride if n else 0
    return np.array(ids + [np.iinfo(np.int64).max] * (stride - len(ids)), dtype=np.int64), len(ids)


def scratch_bytes(users, n_excl):
    """irs_exclusion_scratch_bytes as the header states it; 0 for invalid arguments."""
    if users < 1 or n_excl < 0 or n_excl > MAX_EXCL:
        return 0
    stride = 1
    while stride < n_excl:
        stride <<= 1
    return (4 * users + 15) // 16 * 16 + 8 * users * (stride if n_excl else 0)


def strike(val_row, ids0_row, gone):
    """The list without the items of `gone`, order kept; it ends where it ended (first negative id), or behind its last entry."""
    val_o = np.full(len(val_row), -np.inf, dtype=np.float32)
    ids_o = np.full(len(ids0_row), -1, dtype=np.int64)
    n = 0
    for c in range(len(ids0_row)):
        if ids0_row[c] < 0:
            break
        if int(ids0_row[c]) + 1 not in gone:
            val_o[n], ids_o[n] = val_row[c], ids0_row[c]
            n += 1
    return val_o, ids_o


def _struck_lists(val, ids0, gone_of_row):
    val_o, ids_o = np.array(val, dtype=np.float32), np.array(ids0, dtype=np.int64)
    for r in range(ids_o.shape[0]):
        g = gone_of_row(r)
        if g is not None:
            val_o[r], ids_o[r] = strike(val_o[r], ids_o[r], g)
    return val_o, ids_o


def path_step(seq, hep, val, ids0, step, paths, status, excl, n_item, no_repeat=False, sample=False, sample_k=3, user_of=None):
    """irs_path_step while bound.  excl [users, n_excl] or None; row r reads list user_of[r] (default r) and its own path."""
    user_of = range(len(seq)) if user_of is None else user_of
    v, i = _struck_lists(val, ids0, lambda r: hidden(None if excl is None else excl[user_of[r]], n_item, paths[r], step, no_repeat))
    return path_ref.path_step(seq, hep, v, i, step, paths, status, sample=sample, sample_k=sample_k)


def _beam_gone(state_in, excl, n_item, step, no_repeat, user_of, fin=None):
    seq_i, _, cum_i, paths_i = state_in[:4]
    B, W, _ = np.asarray(seq_i).shape

    def gone(row):
        b, j = divmod(row, W)
        if not cum_i[b][j] > -np.inf or (fin is not None and fin[b][j]):
            return None  # a dead or a finished beam: its lists are never looked at
        return hidden(None if excl is None else excl[user_of[b]], n_item, paths_i[b][j], step, no_repeat)
    return gone


def beam_step(state_in, val, ids0, lse_max, lse_sum, step, P, excl, n_item, no_repeat=False, status=None, user_of=None):
    """irs_beam_step while bound: all W beams of user b read list user_of[b] (default b); a beam's path is its own input path,
    which is the parent's path of whatever it becomes."""
    user_of = range(len(state_in[0])) if user_of is None else user_of
    v, i = _struck_lists(val, ids0, _beam_gone(state_in, excl, n_item, step, no_repeat, user_of))
    return path_ref.beam_step(state_in, v, i, lse_max, lse_sum, step, P, status)


def beam_step_until(state_in, done, val, ids0, lse_max, lse_sum, step, P, stop_rule, excl, n_item, no_repeat=False, status=None,
                    user_of=None):
    """irs_beam_step_until while bound; a finished beam contributes only itself and its (garbage) lists are not touched."""
    user_of = range(len(state_in[0])) if user_of is None else user_of
    v, i = _struck_lists(val, ids0, _beam_gone(state_in, excl, n_item, step, no_repeat, user_of, fin=state_in[4]))
    return beam_until_ref.beam_step_until(state_in, done, v, i, lse_max, lse_sum, step, P, stop_rule, status)


def ensure_survivors(seq, hep, val, ids0, status, want, ranking, excl, n_item, rows_per_status=1, cum=None, fin=None, done=None,
                     paths=None, step=0, no_repeat=False, user_of=None):
    """irs_topk_ensure_survivors while bound: survivors_ref.ensure_survivors with "window" read as window + list (+ path: the
    loops pass one, the standalone entry point has none).  Row m reads the list of user_of[m // rows_per_status]."""
    seq, hep = np.asarray(seq), np.asarray(hep)
    val, ids0, status = np.array(val, dtype=np.float32), np.array(ids0, dtype=np.int64), np.array(status, dtype=np.int32)
    M, k = ids0.shape
    user_of = range(M // rows_per_status) if user_of is None else user_of
    starved = []
    for m in range(M):
        u = m // rows_per_status
        if (cum is not None and cum[m] == -np.inf) or (fin is not None and fin[m] != 0) or (done is not None and done[u] != 0):
            continue
        gone = hidden(None if excl is None else excl[user_of[u]], n_item, None if paths is None else paths[m], step, no_repeat)
        window = [int(x) for x in seq[m, :int(hep[m]) + 1]] + sorted(gone)
        if not survivors_ref.is_starved(window, val[m], ids0[m], want):
            continue
        starved.append(m)
        v, i = survivors_ref.best_admissible(window, *ranking(m), want)
        n = len(i)
        val[m, :n], ids0[m, :n] = v, i
        if n < k:
            val[m, n], ids0[m, n] = -np.inf, -1
        status[u] |= survivors_ref.RESCUED
    return val, ids0, status, starved
