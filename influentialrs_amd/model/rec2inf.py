"""The paper's Rec2Inf framework on the library's plain recommender: MI355X-native counterpart of the reference's get_path
(main_baselines.py:93-121) over a SampleNet (model/uRS.py).

Rec2Inf turns any next-item recommender into a persuader: at each step it takes the recommender's best k_c items the user
has not seen, offers the one whose feature vector lies nearest to the target's (utils.py:202-206, cal_fv_dist) and stops the
user when the target itself has been offered.  Here the whole loop runs on the device: decode -> exact top-100 -> guided
step (include/irs_hip.h: irs_bind_guide), through the same search loops IRSNN.get_seq_in_batch uses.  Only get_path's rule
is built; the reference's baseline recommenders themselves (main_baselines.py's models) are out of scope."""
import functools

import numpy as np
import torch
import torch.nn as nn

from .._lib import IRS_ROW_NO_CANDIDATE
from .influentialRS import STOP_CHECK_EVERY, SearchOptions, exclusion_ids0, _takes_offer, _takes_rank_admissible, offer_ids0, path_trace_summary, search_option_kwargs
from .layers import get_item_index


def rec2inf_windows(seqs, targets, max_len: int, device):
    """The window layout of Rec2Inf on a causal context, from B histories (a list of arrays / tensors of 1-based ids, oldest
    first, or a [B, n] tensor padded with 0) and B targets: the last min(n, L - 1) history items left-aligned from slot 0, then
    zeros, the target in slot L - 1; hep = n - 1.  The consumed row hep <= L - 2 never attends slot L - 1 under the causal
    mask, and the path step keeps slot L - 1 through every shift, so the target only rides along for the choice rule and the
    stop.  Returns (windows int64 [B, L], hep int32 [B], list of B history arrays)."""
    L = max_len
    if torch.is_tensor(seqs):
        if seqs.dim() != 2:
            raise ValueError(f"seqs: a [B, n] tensor padded with 0, or a list of B id arrays (got {tuple(seqs.shape)})")
        rows = [r[r != 0] for r in seqs.detach().cpu().numpy()]
    else:
        rows = [(s.detach().cpu().numpy() if torch.is_tensor(s) else np.asarray(s)).reshape(-1) for s in seqs]
    tg = (targets.detach().cpu().numpy() if torch.is_tensor(targets) else np.asarray(targets)).reshape(-1).astype(np.int64)
    if len(rows) != len(tg):
        raise ValueError(f"{len(rows)} histories for {len(tg)} targets")
    win = np.zeros((len(rows), L), dtype=np.int64)
    hep = np.zeros(len(rows), dtype=np.int32)
    for b, r in enumerate(rows):
        if len(r) == 0:
            raise ValueError(f"user {b} has an empty history: Rec2Inf needs at least one item to recommend from")
        n = min(len(r), L - 1)
        win[b, :n] = r[len(r) - n:]
        win[b, L - 1] = tg[b]
        hep[b] = n - 1
    return torch.from_numpy(win).to(device), torch.from_numpy(hep).to(device), [np.asarray(r) for r in rows]


def _takes_sampler(fn):
    """Gives get_seq_in_batch the keywords temperature=None, top_p=None and draw_k=None, keyword only, the way _takes_offer gives
    it offer.  The method reads them from self._call_sampler, SearchOptions' keywords."""
    @functools.wraps(fn)
    def call(self, *args, temperature=None, top_p=None, draw_k=None, **kw):
        prev = getattr(self, "_call_sampler", {})
        self._call_sampler = dict(temperature=temperature, top_p=top_p, draw_k=draw_k)
        try:
            return fn(self, *args, **kw)
        finally:
            self._call_sampler = prev
    return call


class Rec2Inf(nn.Module):
    """Task handler: Rec2Inf(config, net, device) over a SampleNet."""

    def __init__(self, config, net, device):
        super().__init__()
        self.PAD_ID = 0
        self.n_item = config.n_item
        self.net = net.module if isinstance(net, nn.DataParallel) else net
        self.device = device

    @_takes_offer
    @_takes_rank_admissible
    @_takes_sampler
    def get_seq_in_batch(self, seqs, targets, guide, guide_k=5, max_path_len=20, stop_at_target=True, exclude=None,
                         no_repeat=False, exact_candidates=False, trace=False):
        """Persuasion paths by the Rec2Inf rule: returns (paths float32 [B, max_path_len], targets int64 [B], list of B history
        arrays, n_success), IRSNN.get_seq_in_batch's tuple; n_success is get_path's count of users who were offered their
        target.  Paths are zero behind the target.
        guide: [n_item + 1, F] feature table on the net's device, row i = the 1-based item i (the reference's fv[i]); integer /
        bool: Hamming distance; floating: squared Euclidean distance.  guide_k: the reference's k_c.
        stop_at_target=True stops decoding a user once it has arrived (irs_generate_paths_until), as get_path does; False runs
        every step and cuts on the host: the same paths.
        exclude / no_repeat / exact_candidates / trace: as in IRSNN.get_seq_in_batch.  exclude with the users' whole histories
        is the reference's predict_next(use_h=True), which drops the history and not only the window.
        offer=None (keyword only, taken by _takes_offer; 1-based item ids): as in IRSNN.get_seq_in_batch -- the path is made of items of the set.
        rank_admissible=False, arrive_among="window" (keyword only, taken by _takes_rank_admissible): as in IRSNN.get_seq_in_batch --
        with trace=True, self.last_trace grows rank_adm and slate_step.
        temperature=None, top_p=None, draw_k=None (keyword only, taken by _takes_sampler): IRSNN.get_seq_in_batch's sampler
        keywords; the Rec2Inf rule and the sampler are two rules for the same choice, so any of them raises ValueError."""
        if guide is None:
            raise ValueError("Rec2Inf needs a guide: a [n_item + 1, F] feature table (for the plain greedy path use guide_k=1)")
        # (the guide's own checks, as IRSNN.get_seq_in_batch makes them; the sharded catalog is refused below in this handler's words)
        options = search_option_kwargs(SearchOptions(exact_candidates=exact_candidates, trace=trace, guide=guide, guide_k=guide_k,
                                                     rank_admissible=self._call_rank[0], arrive_among=self._call_rank[1],
                                                     **self._call_sampler), 1, False, 1)
        hip = self.net._hip
        if hip.world != 1:
            raise ValueError("Rec2Inf is not built for an item-sharded catalog: irs_bind_guide needs the whole catalog on one "
                             "device")
        self.net.eval()
        L = self.net.max_len
        dev = next(self.net.parameters()).device
        work, hep, histories = rec2inf_windows(seqs, targets, L, dev)
        B = work.shape[0]
        ids0 = exclusion_ids0(exclude, no_repeat, work, L - 2, dev)
        excl = dict(exclude=ids0, no_repeat=no_repeat) if (ids0 is not None or no_repeat) else {}
        eng = hip.get(B, B)
        off = offer_ids0(self._call_offer, self.n_item, dev)
        common = dict(k=100, sweep=hip.sweep, **options, **excl, **(dict(offer=off) if off is not None else {}))
        if stop_at_target:
            paths_t, status, _, _, *traced = eng.generate_paths_until(work, None, hep, max_path_len, check_every=STOP_CHECK_EVERY,
                                                                      **common)
        else:
            paths_t, status, *traced = eng.generate_paths(work, None, hep, max_path_len, use_graph=False, **common)
        if int((status & IRS_ROW_NO_CANDIDATE).sum().item()) > 0:
            raise IndexError("index 0 is out of bounds: every admissible item is excluded (window"
                             + (" + exclusion list" if excl else "") + (" + path)" if no_repeat else ")")
                             + ("" if exact_candidates else " among the top-100 candidates"))
        paths = paths_t.detach().cpu().numpy()
        tg = (targets.detach().cpu().numpy() if torch.is_tensor(targets) else np.asarray(targets)).reshape(-1).astype(np.int64)
        if trace:
            tr = [a.detach().cpu().numpy() for a in traced[0]]
            self.last_trace = path_trace_summary(*tr[:3], paths, tg, rank_adm=tr[3] if len(tr) > 3 else None)
        n_success = 0
        for i in range(B):
            pos = get_item_index(paths[i], tg[i])
            if pos != -1:
                n_success += 1
                paths[i][pos + 1:] = 0
        return paths, tg, histories, n_success
