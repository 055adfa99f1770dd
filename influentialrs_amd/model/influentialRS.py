"""MI355X-native counterpart of the reference's model/influentialRS.py.

Same classes, constructor arguments, method names, argument meaning, return
tuples and state_dict key set as the reference, so
`pipeline.py` can import this module in place of `model.influentialRS`
unchanged.  In eval mode every forward / scoring / path-search call runs on the
hand-written gfx950 kernels behind include/irs_hip.h; there is no CPU
fallback (IrsError if the network is not on a GPU).  Training mode runs the
stock PyTorch autograd modules by default; net.trunk = "hip" (or
IRS_TRAIN_TRUNK=hip) runs the decoder trunk's forward and backward on the
native kernels instead.

Behaviour pinned by the reference (file:line = /root/reference/model/influentialRS.py):
  * mask semantics are the AS-CALLED ones (allowed = r_u, last column = 1.0,
    :183-184 passing pi_factor into w_h), applied per row, so batches > 1 work
    where the published code raises;
  * logits index j <-> item id j+1 (:376, :422); pad id 0;
  * ranking filters the full raw history (:372-379), path search filters the
    current window (:423-427); rr skips rows whose label is filtered (:386);
  * candidate width 100 (:421); all 100 in the window -> IndexError (:429);
  * selection order is (score desc, id asc); torch's tie order is unspecified.
"""
import dataclasses
import functools
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim

from .._lib import IRS_BEAM_STOP_ALL, IRS_BEAM_STOP_BEST, IRS_MASK_IRN, IRS_REPLAY_SLOT, IRS_ROW_NO_CANDIDATE, IRS_ROW_OFFERED
from ._backend import HipBackend, check_trunk, make_scheduler, pad_ragged_ids, project_ce, project_ce_sharded, train_trunk_default, trunk_hip
from .layers import PositionalEncoding, get_item_index

_SHARDED_GRAPH = os.environ.get("IRS_SHARDED_GRAPH", "0") == "1"  # captured sharded steps: opt-in (see _beam_paths)
# get_seq_in_batch(stop_at_target=True): live users are counted (one 4-byte host read) and compacted after every step; larger
# values trade finished users stepped for fewer reads.  1 is the issue's default, not a measured choice: nothing is measured yet.
STOP_CHECK_EVERY = 1
# get_seq_in_batch(beam_width > 1, beam_stop=...): the same trade for irs_beam_search_until, as unmeasured
BEAM_STOP_CHECK_EVERY = 1
_BEAM_STOP_RULES = {"best": IRS_BEAM_STOP_BEST, "all": IRS_BEAM_STOP_ALL}


class InfluentialNet(nn.Module):
    """Influential Recommender Network (reference :22-216)."""

    def __init__(self, config):
        super().__init__()
        self.PAD_ID = 0
        self.item_embed_path = None
        self.user_embed_path = None
        self.n_item = config.n_item
        self.n_user = config.n_user
        self.use_u = False
        self.max_len = config.max_len
        self.n_layers = config.n_layers
        self.n_heads = config.n_heads
        self.embed_dim = config.emb_dim
        self.u_embed_dim = config.u_emb_dim
        self.ffn_dim = config.ffn_dim
        self.dropout = config.dropout

        self.item_embedder = nn.Embedding(self.n_item + 1, self.embed_dim, padding_idx=self.PAD_ID)
        self.user_embedder = nn.Embedding(self.n_user, self.u_embed_dim)
        self.pos_embedder = PositionalEncoding(self.embed_dim, self.max_len)
        self.decoder = nn.TransformerDecoder(
            decoder_layer=nn.TransformerDecoderLayer(d_model=self.embed_dim, nhead=self.n_heads,
                                                     dim_feedforward=self.ffn_dim, dropout=self.dropout,
                                                     activation="relu"),
            num_layers=self.n_layers)
        self.user_mask_layer = nn.Linear(self.u_embed_dim, 1)
        self.project = nn.Linear(self.embed_dim, self.n_item)

        self.optimizer = optim.Adam(filter(lambda x: x.requires_grad, self.parameters()), betas=(0.9, 0.98),
                                    eps=1e-09, lr=config.lr1)
        self.pla_lr_scheduler = make_scheduler(self.optimizer)
        self._hip = HipBackend(self, IRS_MASK_IRN)
        self.trunk = train_trunk_default()

    @property
    def trunk(self) -> str:
        """Train-mode decoder trunk: "torch" (stock nn.TransformerDecoder autograd) or "hip" (native forward + backward,
        include/irs_hip.h irs_train_*).  Default from IRS_TRAIN_TRUNK."""
        return self._trunk

    @trunk.setter
    def trunk(self, v: str):
        self._trunk = check_trunk(v)

    @property
    def ce_backward(self) -> str:
        """Backward of projection + cross entropy: "chunked" (dL/dlogits per row chunk + torch GEMMs) or "fused"
        (include/irs_hip.h irs_ce_backward: no dL/dlogits buffer).  Default from IRS_CE_BACKWARD."""
        return self._hip.ce_backward

    @ce_backward.setter
    def ce_backward(self, v: str):
        self._hip.ce_backward = v

    # ---- checkpoint contract: accept nn.DataParallel's "module." prefix (pipeline.py:140-142)
    def load_state_dict(self, state_dict, strict=True, **kw):
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        return super().load_state_dict(sd, strict=strict, **kw)

    def shard_items(self, rank: int, world: int, drop_full: bool = True):
        """Hold only rows [lo, hi) of the catalog on this GPU.  With drop_full (default) the
        module's own project.weight / project.bias are cut down to the shard -- call it after
        load_state_dict: from then on this rank's state_dict() carries the LOCAL rows only.  forward() (the
        [B, L, n_item] logits of a full nn.Linear) is not available on such a module; the handlers' losses are:
        IRSNN / Evaluator.train_batch and get_loss_on_eval_data take the vocabulary-parallel projection + cross
        entropy (include/irs_hip.h irs_ce_forward_sharded / irs_ce_backward_sharded) -- every rank passes its own
        slice of the batch (the same number of sequences), gets the loss of the WHOLE batch, and train_batch
        SUM-all-reduces the gradients of the replicated parameters before its optimizer step; project.* gradients
        are the shard's own.  Both ce_backward settings run the fused kernels there.  A module kept whole
        (drop_full=False) keeps the reference's own formulation on its full nn.Linear."""
        self._hip.set_sharding(rank, world, drop_full)

    # ---- training-mode path: stock PyTorch autograd, per-row as-called mask
    def _generate_square_subsequent_mask(self, size, pi_factor):
        """[B*H, L, L] float mask: allowed = r_u[b], future = -inf, last column = 1.0
        (the as-called semantics of reference :120-155 / :183-184, per row)."""
        pi_factor = pi_factor.detach()  # the reference calls float() on it (:141): no gradient reaches the user tensors
        B = pi_factor.size(0)
        dev = pi_factor.device
        tril = torch.ones(size, size, device=dev).tril().bool()
        m = torch.full((B, size, size), float("-inf"), device=dev)
        m = torch.where(tril.unsqueeze(0), pi_factor.view(B, 1, 1).expand(B, size, size).float(), m)
        m[:, :, -1] = 1.0
        return torch.repeat_interleave(m, self.n_heads, dim=0)

    def _decoding_autograd(self, dec_input_seq, user):
        if self.trunk == "hip":
            pi = self.user_mask_layer(self.user_embedder(user))
            return trunk_hip(self, dec_input_seq, user, "item_embedder.weight"), pi
        pad = dec_input_seq.eq(self.PAD_ID)
        enc = torch.zeros(self.max_len, dec_input_seq.size(0), self.embed_dim, device=dec_input_seq.device)
        x = self.item_embedder(dec_input_seq) * math.sqrt(self.embed_dim) + self.pos_embedder(dec_input_seq)
        x = F.dropout(x, self.dropout, self.training).transpose(0, 1)
        pi = self.user_mask_layer(self.user_embedder(user))
        mask = self._generate_square_subsequent_mask(dec_input_seq.size(1), pi)
        padf = torch.zeros_like(pad, dtype=torch.float32).masked_fill(pad, float("-inf"))
        out = self.decoder(tgt=x, memory=enc, tgt_mask=mask, tgt_key_padding_mask=padf)
        return out.transpose(0, 1), pi

    # ---- reference API
    def decoding(self, dec_input_seq, user, return_pi=False):
        """[B, L] ids, [B] users -> [B, L, d] (and r_u [B, 1] if return_pi)."""
        if self.training:
            x, pi = self._decoding_autograd(dec_input_seq, user)
        else:
            eng = self._hip.get(dec_input_seq.size(0), 1)
            x, _, ru = eng.decode(dec_input_seq, user, want_x=True, want_r_u=True)
            pi = ru.view(-1, 1)
        return (x, pi) if return_pi else x

    def forward(self, dec_input_seq, user):
        """[B, L, n_item] logits (reference :202-216).  The reference materialises
        this tensor on every call; here it exists for API compatibility (and
        training) -- the task handlers below never build it."""
        if self.training:
            x, _ = self._decoding_autograd(dec_input_seq, user)
            return self.project(x)
        B, L = dec_input_seq.shape
        eng = self._hip.get(B, B * L)
        if eng.world != 1:
            raise RuntimeError("forward() materialises [B, L, n_item]; with item sharding use the IRSNN handlers")
        x, _, _ = eng.decode(dec_input_seq, user, want_x=True)
        return eng.score_dense(x.view(B * L, self.embed_dim)).view(B, L, self.n_item)

    # rows of the decoder output at one position per sequence, without materialising [B, L, d] on the host side
    def decode_rows(self, seqs, users, pos):
        eng = self._hip.get(seqs.size(0), seqs.size(0))
        _, xr, _ = eng.decode(seqs, users, want_x=False, pos=pos)
        return xr


@dataclasses.dataclass(frozen=True)
class SearchOptions:
    """get_seq_in_batch's keyword-only extensions, as _takes_exact_candidates holds them for the time of one call."""
    exact_candidates: bool = False
    exclude: object = None
    no_repeat: bool = False
    trace: bool = False
    guide: object = None
    guide_k: int = 5
    arrive_rank: object = None
    arrive_lp: object = None
    lookahead: object = None
    lookahead_record: bool = False
    offer: object = dataclasses.field(default=None, kw_only=True)  # (keyword only: no positional constructor shifts)
    beam_arrive_rank: object = dataclasses.field(default=None, kw_only=True)  # the beam rule (irs_set_beam_rule), likewise
    beam_arrive_lp: object = dataclasses.field(default=None, kw_only=True)
    beam_target_weight: float = dataclasses.field(default=0.0, kw_only=True)
    rank_admissible: bool = dataclasses.field(default=False, kw_only=True)  # irs_bind_trace_admissible: last_trace["rank_adm"]
    arrive_among: str = dataclasses.field(default="window", kw_only=True)  # the rank arrive_rank reads (irs_set_arrival_rule_ex)
    temperature: object = dataclasses.field(default=None, kw_only=True)  # the bound sampler (irs_bind_sampler): any of the three binds it
    top_p: object = dataclasses.field(default=None, kw_only=True)
    draw_k: object = dataclasses.field(default=None, kw_only=True)
    draw_record: bool = dataclasses.field(default=False, kw_only=True)  # last_draws
    beam_trace: bool = False
    beam_pick: str = "score"


def beam_rule_kwargs(opts: SearchOptions, beam_width: int, world: int) -> dict:
    """The engine's beam-loop keywords for beam_arrive_rank / beam_arrive_lp / beam_target_weight ({} when none is given);
    ValueError for a value out of range, for beam_width == 1 and for an item-sharded catalog.  That the rule needs
    beam_trace=True is the library's own answer (IrsError, IRS_E_STATE)."""
    rank, lp, lam = opts.beam_arrive_rank, opts.beam_arrive_lp, opts.beam_target_weight
    if rank is None and lp is None and not lam:
        return {}
    if rank is not None and (isinstance(rank, bool) or int(rank) != rank or rank < 1):
        raise ValueError(f"beam_arrive_rank={rank!r}: a rank of 1 or more (None: no rank clause)")
    if lp is not None and not float(lp) <= 0:
        raise ValueError(f"beam_arrive_lp={lp!r}: a log-probability, at most 0 (None: no probability clause)")
    if not 0 <= float(lam) < float("inf"):
        raise ValueError(f"beam_target_weight={lam!r}: finite and at least 0 (0: rank by acceptance alone)")
    if beam_width == 1:
        raise ValueError("beam_arrive_rank / beam_arrive_lp / beam_target_weight need beam_width > 1: use arrive_rank / arrive_lp "
                         "for the greedy / sampled search")
    if world != 1:
        raise ValueError("the beam rule is not built for an item-sharded catalog: irs_set_beam_rule needs the whole catalog on "
                         "one device")
    return dict(arrive_rank=None if rank is None else int(rank), arrive_lp=None if lp is None else float(lp), target_weight=float(lam))


def search_option_kwargs(opts: SearchOptions, beam_width: int, sample: bool, world: int) -> dict:
    """What the options ask of a search over `world` item shards with this beam width and choice: ValueError where an option
    has no such form or a value is out of range, else the engine's greedy-loop keywords for them (exclude / no_repeat aside: the
    lists need the windows, exclusion_ids0; offer aside as well: offer_ids0 makes its device array).  An arrival rule implies
    trace=True."""
    trace = opts.trace
    kw = {}
    if opts.arrive_rank is not None or opts.arrive_lp is not None:
        rank, lp = opts.arrive_rank, opts.arrive_lp
        if rank is not None and (isinstance(rank, bool) or int(rank) != rank or rank < 1):
            raise ValueError(f"arrive_rank={rank!r}: a rank of 1 or more (None: no rank clause)")
        if lp is not None and not float(lp) <= 0:
            raise ValueError(f"arrive_lp={lp!r}: a log-probability, at most 0 (None: no probability clause)")
        if beam_width > 1:
            raise ValueError("arrive_rank / arrive_lp is not built for beam search (beam_width > 1): the arrival rule reads "
                             "the path trace, which is not carried through beam state")
        if world != 1:
            raise ValueError("arrive_rank / arrive_lp is not built for an item-sharded catalog: irs_set_arrival_rule needs "
                             "the whole catalog on one device")
        kw.update(arrive_rank=None if rank is None else int(rank), arrive_lp=None if lp is None else float(lp))
        trace = True
    if opts.arrive_among not in ("window", "admissible"):
        raise ValueError(f"arrive_among={opts.arrive_among!r}: use \"window\" (rank_target) or \"admissible\" (rank_adm)")
    if opts.arrive_among == "admissible":
        if not opts.rank_admissible:
            raise ValueError("arrive_among=\"admissible\" reads the admissible rank: use rank_admissible=True")
        kw.update(arrive_among="admissible")
    if opts.rank_admissible:
        if not trace:
            raise ValueError("rank_admissible=True adds a column to the path trace: use trace=True")
        kw.update(rank_admissible=True)
    if opts.lookahead is not None:
        k_c = opts.lookahead
        if isinstance(k_c, bool) or not isinstance(k_c, (int, np.integer)) or not 1 <= k_c <= 32:
            raise ValueError(f"lookahead={k_c!r}: an int from 1 to 32, the candidates a step looks ahead from (None: off)")
        if opts.guide is not None:
            raise ValueError("lookahead and guide are two rules for the same choice: use one of them")
        if sample:
            raise ValueError("lookahead is not built for the sampled search: the choice is deterministic, use sample=False")
        if beam_width > 1:
            raise ValueError("lookahead is not built for beam search (beam_width > 1): use beam_width=1 (the lookahead choice "
                             "is a rule of the greedy step)")
        if world != 1:
            raise ValueError("lookahead is not built for an item-sharded catalog: irs_bind_lookahead needs the whole catalog "
                             "on one device")
        kw.update(lookahead=int(k_c), lookahead_record=opts.lookahead_record)
    elif opts.lookahead_record:
        raise ValueError("lookahead_record=True needs lookahead=k_c")
    if opts.guide is not None:
        if beam_width > 1:
            raise ValueError("guide is not built for beam search (beam_width > 1): use beam_width=1 (the guided choice is a "
                             "rule of the greedy step)")
        if sample:
            raise ValueError("guide is not built for the sampled search: the guided choice is deterministic, use sample=False")
        if world != 1:
            raise ValueError("guide is not built for an item-sharded catalog: irs_bind_guide needs the whole catalog on one "
                             "device")
        if not 1 <= opts.guide_k <= 32:
            raise ValueError(f"guide_k={opts.guide_k}: the guided step chooses among 1 to 32 candidates")
        kw.update(guide=opts.guide, guide_k=opts.guide_k)
    if opts.temperature is not None or opts.top_p is not None or opts.draw_k is not None:
        t = 1.0 if opts.temperature is None else opts.temperature
        p = 1.0 if opts.top_p is None else opts.top_p
        draw_k = 3 if opts.draw_k is None else opts.draw_k
        if isinstance(t, bool) or not 0 < float(t) < float("inf"):
            raise ValueError(f"temperature={t!r}: finite and above 0 (1: the model's own distribution among the candidates)")
        if isinstance(p, bool) or not 0 < float(p) <= 1:
            raise ValueError(f"top_p={p!r}: in (0, 1] (1: no nucleus cut)")
        if isinstance(draw_k, bool) or not isinstance(draw_k, (int, np.integer)) or not 1 <= draw_k <= 100:
            raise ValueError(f"draw_k={draw_k!r}: an int from 1 to 100, the candidates a step draws among (the loops rank 100)")
        if sample:
            raise ValueError("temperature / top_p / draw_k bind the sampler and sample=True is the stock sampled step: two "
                             "samplers, use sample=False")
        if opts.guide is not None:
            raise ValueError("temperature / top_p / draw_k and guide are two rules for the same choice: use one of them")
        if opts.lookahead is not None:
            raise ValueError("temperature / top_p / draw_k and lookahead are two rules for the same choice: use one of them")
        if beam_width > 1:
            raise ValueError("temperature / top_p / draw_k is not built for beam search (beam_width > 1): use beam_width=1 (the "
                             "sampler is a rule of the greedy step)")
        if world != 1:
            raise ValueError("temperature / top_p / draw_k is not built for an item-sharded catalog: irs_bind_sampler needs the "
                             "whole catalog on one device")
        if opts.exact_candidates and draw_k > 32:
            raise ValueError(f"draw_k={draw_k} with exact_candidates=True: a row is repaired to at most 32 candidates")
        from ..engine import Sampler
        kw.update(sampler=Sampler(int(draw_k), float(t), float(p), bool(opts.draw_record)))
    elif opts.draw_record:
        raise ValueError("draw_record=True needs the sampler: give temperature, top_p or draw_k")
    if opts.beam_pick not in ("score", "target"):
        raise ValueError(f"beam_pick={opts.beam_pick!r}: use \"score\" (beam 0) or \"target\"")
    if opts.beam_pick == "target" and not opts.beam_trace:
        raise ValueError("beam_pick=\"target\" reads the beam trace: use beam_trace=True")
    if opts.beam_trace:
        if beam_width == 1:
            raise ValueError("beam_trace needs beam_width > 1: use trace=True for the greedy / sampled search")
        if world != 1:
            raise ValueError("beam_trace is not built for an item-sharded catalog: irs_bind_beam_trace needs the whole catalog "
                             "on one device")
    if trace and beam_width > 1:
        raise ValueError("trace is not built for beam search (beam_width > 1): no trace is carried through beam state")
    if trace and world != 1:
        raise ValueError("trace is not built for an item-sharded catalog: irs_bind_path_trace needs the whole catalog on "
                         "one device")
    if (opts.exclude is not None or opts.no_repeat) and world != 1:
        raise ValueError("exclude / no_repeat is not built for an item-sharded catalog: irs_bind_exclusions needs the whole "
                         "catalog on one device")
    if opts.offer is not None and world != 1:
        raise ValueError("offer is not built for an item-sharded catalog: irs_bind_offer_set needs the whole catalog on one "
                         "device")
    if opts.exact_candidates and world != 1:
        raise ValueError("exact_candidates is not built for an item-sharded catalog: a shard can only rescue a row against "
                         "its own items")
    return dict(exact_candidates=opts.exact_candidates, trace=trace, **kw)


def _takes_exact_candidates(fn):
    """Gives get_seq_in_batch its keywords exact_candidates=False, exclude=None, no_repeat=False, trace=False, guide=None,
    guide_k=5, arrive_rank=None, arrive_lp=None, lookahead=None, lookahead_record=False, beam_trace=False,
    beam_pick="score", offer=None, beam_arrive_rank=None, beam_arrive_lp=None, beam_target_weight=0.0, rank_admissible=False,
    arrive_among="window", temperature=None, top_p=None, draw_k=None and draw_record=False.  They are taken here,
    keyword only,
    so that the declared parameter list stays what it was (it ends with beam_stop): positional callers and code that reads the
    signature are not disturbed.  The search reads them from self._search_options, a SearchOptions, for the time of the call."""
    @functools.wraps(fn)
    def call(self, *args, exact_candidates=False, exclude=None, no_repeat=False, trace=False, guide=None, guide_k=5,
             arrive_rank=None, arrive_lp=None, lookahead=None, lookahead_record=False, beam_trace=False, beam_pick="score", offer=None,
             beam_arrive_rank=None, beam_arrive_lp=None, beam_target_weight=0.0, rank_admissible=False, arrive_among="window",
             temperature=None, top_p=None, draw_k=None, draw_record=False, **kw):
        prev = self._search_options
        self._search_options = SearchOptions(bool(exact_candidates), exclude, bool(no_repeat), bool(trace), guide, int(guide_k),
                                             arrive_rank, arrive_lp, lookahead, bool(lookahead_record), bool(beam_trace), beam_pick, offer=offer,
                                             beam_arrive_rank=beam_arrive_rank, beam_arrive_lp=beam_arrive_lp,
                                             beam_target_weight=beam_target_weight, rank_admissible=bool(rank_admissible),
                                             arrive_among=arrive_among, temperature=temperature, top_p=top_p, draw_k=draw_k,
                                             draw_record=bool(draw_record))
        try:
            return fn(self, *args, **kw)
        finally:
            self._search_options = prev
    return call


def _takes_offer(fn):
    """Gives a front-end method its keyword offer=None (1-based item ids: offer_ids0), keyword only, the way
    _takes_exact_candidates gives get_seq_in_batch its keywords: the declared parameter list stays what it was.  The method reads
    it from self._call_offer for the time of the call."""
    @functools.wraps(fn)
    def call(self, *args, offer=None, **kw):
        prev = getattr(self, "_call_offer", None)
        self._call_offer = offer
        try:
            return fn(self, *args, **kw)
        finally:
            self._call_offer = prev
    return call


def _takes_rank_admissible(fn):
    """Gives a front-end method its keywords rank_admissible=False and arrive_among="window", keyword only, the way _takes_offer
    gives it offer: the declared parameter list stays what it was.  The method reads them from self._call_rank, a pair."""
    @functools.wraps(fn)
    def call(self, *args, rank_admissible=False, arrive_among="window", **kw):
        prev = getattr(self, "_call_rank", (False, "window"))
        self._call_rank = (bool(rank_admissible), arrive_among)
        try:
            return fn(self, *args, **kw)
        finally:
            self._call_rank = prev
    return call


def slate_steps(rank_adm, n_steps, r):
    """The first live step of every user at which the target stands among the first r admissible items (0 < rank_adm <= r), -1
    where it never does: int64 [B]."""
    rank_adm = np.asarray(rank_adm)
    B, P = rank_adm.shape
    hit = (rank_adm > 0) & (rank_adm <= int(r)) & (np.arange(P)[None, :] < np.asarray(n_steps)[:, None])
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1).astype(np.int64)


def path_trace_summary(lp_item, lp_target, rank_target, paths, targets, n_live=None, rank_adm=None):
    """get_seq_in_batch's last_trace from the search's arrays ([B, P] each; `paths` before the host cut or after it, `targets`
    [B]).  A user's live steps end with its arrival (the first path entry equal to its target) or run to P (n_live[b] where
    given: a replayed path that ends early); behind them the three arrays are cut to 0 like the path.  Over the live steps, as
    Evaluator.get_grad_in_batch forms iois and avg_ps:
    ioi = last lp_target - first, ior = first rank_target - last (positive: the target moved up), avg_lp_item = mean lp_item.
    rank_adm (irs_bind_trace_admissible's array, where given) is cut the same way and comes with slate_step, a function of r:
    slate_steps(rank_adm, n_steps, r)."""
    lp_item = np.array(lp_item, dtype=np.float32)
    lp_target = np.array(lp_target, dtype=np.float32)
    rank_target = np.array(rank_target, dtype=np.int32)
    B, P = lp_item.shape
    n_steps = np.full(B, P, dtype=np.int64) if n_live is None else np.array(n_live, dtype=np.int64)
    for i in range(B):
        pos = get_item_index(np.asarray(paths[i]), np.asarray(targets).reshape(-1)[i])
        if pos != -1:
            n_steps[i] = pos + 1
        for a in (lp_item, lp_target, rank_target):
            a[i, n_steps[i]:] = 0
    last = n_steps - 1
    rows = np.arange(B)
    out = dict(lp_item=lp_item, lp_target=lp_target, rank_target=rank_target, n_steps=n_steps,
               ioi=lp_target[rows, last].astype(np.float64) - lp_target[:, 0].astype(np.float64),
               ior=rank_target[:, 0].astype(np.int64) - rank_target[rows, last].astype(np.int64),
               avg_lp_item=np.array([lp_item[i, :n_steps[i]].astype(np.float64).mean() for i in range(B)]))
    if rank_adm is not None:
        rank_adm = np.array(rank_adm, dtype=np.int32)
        for i in range(B):
            rank_adm[i, n_steps[i]:] = 0
        out.update(rank_adm=rank_adm, slate_step=lambda r: slate_steps(rank_adm, n_steps, r))
    return out


def beam_trace_summary(lp_item, lp_target, rank_target, paths, scores, targets):
    """get_seq_in_batch's last_beam_trace from a beam search's arrays ([B, W, P] each, scores [B, W], targets [B]).  A beam's
    recorded steps end with its arrival (the first path entry equal to the user's target) or run to P; a dead beam (score
    -inf) has none.  Behind them the three arrays are cut to 0, as path_trace_summary cuts a greedy trace."""
    lp_item = np.array(lp_item, dtype=np.float32)
    lp_target = np.array(lp_target, dtype=np.float32)
    rank_target = np.array(rank_target, dtype=np.int32)
    paths, scores = np.asarray(paths), np.asarray(scores)
    B, W, P = lp_item.shape
    n_steps = np.full((B, W), P, dtype=np.int64)
    for b in range(B):
        for j in range(W):
            if not scores[b, j] > -np.inf:
                n_steps[b, j] = 0
            else:
                pos = get_item_index(paths[b, j], np.asarray(targets).reshape(-1)[b])
                if pos != -1:
                    n_steps[b, j] = pos + 1
            for a in (lp_item, lp_target, rank_target):
                a[b, j, n_steps[b, j]:] = 0
    return dict(lp_item=lp_item, lp_target=lp_target, rank_target=rank_target, paths=np.array(paths), scores=np.array(scores),
                n_steps=n_steps)


def beam_rule_summary(trace, targets, rank_max=None, lp_min=None):
    """What a beam rule adds to last_beam_trace, from the recorded arrays alone (trace: beam_trace_summary's dict): arrival_step
    int64 [B, W], the step at which a live beam's path holds the user's target (-1: never), and offered bool [B, W]: at that
    step a clause of the rule holds on (rank_target, lp_target) -- rank_target != 0 and (rank_target <= rank_max, or lp_target >=
    lp_min as float32; a NaN never holds) -- which is exactly when the rule offered the target there."""
    paths, n_steps = trace["paths"], trace["n_steps"]
    B, W, _ = paths.shape
    tg = np.asarray(targets).reshape(B, 1)
    rows, cols = np.arange(B)[:, None], np.arange(W)[None, :]
    last = np.maximum(n_steps - 1, 0)
    arrived = (n_steps > 0) & (paths[rows, cols, last] == tg)
    rk, lp = trace["rank_target"][rows, cols, last], trace["lp_target"][rows, cols, last]
    holds = np.zeros((B, W), dtype=bool)
    if rank_max is not None and int(rank_max) >= 1:
        holds |= rk <= int(rank_max)
    if lp_min is not None and np.float32(lp_min) <= 0:
        with np.errstate(invalid="ignore"):
            holds |= lp >= np.float32(lp_min)
    return dict(arrival_step=np.where(arrived, last, -1).astype(np.int64), offered=arrived & (rk != 0) & holds)


def pick_beam(paths, scores, lp_target, n_steps, targets, how="score"):
    """The beam get_seq_in_batch returns per user, int64 [B].  "score": beam 0, the best score.  "target": the live beam (score
    > -inf) whose path holds the user's target at the earliest step -- ties go to the higher score, then to the lower index;
    if no live beam holds it, the live beam with the largest lp_target in its last recorded column n_steps - 1, ties broken
    the same way.  A user without a live beam gets beam 0."""
    paths, scores, lp_target, n_steps = (np.asarray(a) for a in (paths, scores, lp_target, n_steps))
    B, W, P = paths.shape
    if how == "score":
        return np.zeros(B, dtype=np.int64)
    if how != "target":
        raise ValueError(f"beam_pick={how!r}: use \"score\" or \"target\"")
    tg = np.asarray(targets).reshape(B, 1, 1)
    hit = paths == tg
    first = np.where(hit.any(axis=2), hit.argmax(axis=2), P)  # P: the path never holds the target
    last = lp_target[np.arange(B)[:, None], np.arange(W)[None, :], np.maximum(n_steps - 1, 0)].astype(np.float64)
    live = scores > -np.inf
    out = np.zeros(B, dtype=np.int64)
    for b in range(B):
        if not live[b].any():
            continue
        arrived = live[b] & (first[b] < P)
        # lexsort: the last key is the primary one; every key ascending, the index last among ties
        if arrived.any():
            order = np.lexsort((np.arange(W), -scores[b], first[b]))
            out[b] = next(j for j in order if arrived[j])
        else:
            order = np.lexsort((np.arange(W), -scores[b], -last[b]))
            out[b] = next(j for j in order if live[b, j])
    return out


def offer_ids0(offer, n_item: int, device):
    """The array irs_bind_offer_set takes (int64, 0-based ids) from a front end's `offer`: 1-based item ids in any order, a
    tensor, an array or a list; repeats are dropped by the binding.  None: no offer set."""
    if offer is None:
        return None
    ids = (offer.detach().to(device) if torch.is_tensor(offer) else torch.as_tensor(np.asarray(offer), device=device)).reshape(-1)
    if ids.numel() == 0:
        raise ValueError("offer: an empty set leaves nothing to offer (None: no offer set)")
    if ids.dtype.is_floating_point or ids.dtype == torch.bool:
        raise ValueError(f"offer: 1-based integer item ids (got {ids.dtype})")
    ids = ids.to(torch.int64)
    if int(ids.min().item()) < 1 or int(ids.max().item()) > n_item:
        raise ValueError(f"offer: item ids must be in [1, n_item={n_item}]")
    return ids - 1


def exclusion_ids0(exclude, no_repeat, seqs, hep: int, device):
    """The lists irs_bind_exclusions takes (int64 [B, E], 0-based ids, -1 = unused) from get_seq_in_batch's `exclude`: a list of
    B arrays / tensors of 1-based ids like `raw`, or a [B, E] tensor padded with 0; None: no list.  no_repeat appends the
    user's initial window seqs[b, :hep + 1], so that nothing the window ever held is offered again.  None when there is nothing."""
    parts = []
    if exclude is not None:
        if torch.is_tensor(exclude):
            if exclude.dim() != 2 or exclude.shape[0] != seqs.shape[0]:
                raise ValueError(f"exclude: a [B, E] tensor padded with 0, or a list of B id arrays (got {tuple(exclude.shape)})")
            parts.append(exclude.to(device).to(torch.int64) - 1)
        else:
            if len(exclude) != seqs.shape[0]:
                raise ValueError(f"exclude: {len(exclude)} lists for {seqs.shape[0]} users")
            parts.append(pad_ragged_ids(exclude, device))
    if no_repeat:
        parts.append(seqs[:, :hep + 1].to(device).to(torch.int64) - 1)
    if not parts:
        return None
    return torch.cat(parts, dim=1).contiguous()


class IRSNN(nn.Module):
    """Task handler (reference :219-470)."""
    _search_options = SearchOptions()  # (off between calls: _takes_exact_candidates)

    def __init__(self, config, net, device):
        super().__init__()
        self.PAD_ID = 0
        self.n_item = config.n_item
        self.embed_dim = config.emb_dim
        # pipeline.py:43-44,140-141 wraps the net in nn.DataParallel on multi-GPU hosts; the
        # handlers need the module itself (the reference fails at :337 in that case)
        self.net = net.module if isinstance(net, nn.DataParallel) else net
        self.device = device
        self.loss_function = nn.CrossEntropyLoss()
        self.optimizer = optim.Adam(filter(lambda x: x.requires_grad, self.net.parameters()), betas=(0.9, 0.98),
                                    eps=1e-09, lr=config.lr1)
        self.pla_lr_scheduler = make_scheduler(self.optimizer)
        self.softmax = nn.Softmax(dim=2)

    # ---- training side: the decoder trunk is stock autograd (train mode) or the HIP engine (eval mode); projection +
    #      cross entropy go through the HIP engine in both, never materialising [B (L-1), n_item]
    def _masked_loss(self, seqs, users):
        net = self.net
        if net.training:
            x, _ = net._decoding_autograd(seqs.clone(), users)
        else:
            x = net.decoding(seqs.clone(), users)
        rows = x[:, :-1, :].reshape(-1, net.embed_dim)
        tgt = seqs[:, 1:].reshape(-1)
        labels0 = torch.where(tgt.gt(self.PAD_ID), tgt - 1, torch.full_like(tgt, -1)).to(torch.int64)
        if rows.device.type == "cuda" and net._hip.holds_shard():  # the module holds only its rows of project.*
            return project_ce_sharded(rows, net.project, labels0, net._hip)
        if net._hip.world != 1 or rows.device.type != "cuda":  # whole module on a sharded engine, or CPU: the reference's own formulation
            out = net.project(rows)
            mask = labels0.ge(0)
            return self.loss_function(out[mask], labels0[mask])
        return project_ce(rows, net.project, labels0, net._hip)

    def get_loss_on_eval_data(self, seqs, users):
        """Mean next-item cross entropy over non-pad targets (reference :252-276)."""
        self.net.eval()
        with torch.no_grad():
            return self._masked_loss(seqs, users).item()

    def train_batch(self, seqs, users):
        """One Adam step (reference :278-310)."""
        self.net.train()
        loss = self._masked_loss(seqs, users)
        self.optimizer.zero_grad()
        loss.backward()
        if self.net._hip.holds_shard():  # replicated parameters: SUM of the ranks' gradients; project.* stay local
            self.net._hip.allreduce_replicated_grads()
        self.optimizer.step()
        return loss.item()

    # ---- inference hot path
    def get_pif_in_batch(self, seqs, users):
        """r_u [B, 1] float32 (reference :325-338; the reference runs the whole
        decoder to obtain it, here it is the two-op scalar it actually is)."""
        self.net.eval()
        eng = self.net._hip.get(seqs.size(0), 1)
        return eng.pif(users).view(-1, 1).detach().cpu().numpy()

    def get_accuracy_metrics_in_batch(self, raw, seqs, users, targets, labels, top_k=20, gap_len=20, use_h=True):
        """(hit_count, rr array) -- Hit@top_k and reciprocal ranks (reference :340-390).
        rank = 1 + #{items outside the raw history that precede the label}; no sort,
        no [N, |hist|] boolean blow-up."""
        self.net.eval()
        B, L = seqs.shape
        dev = seqs.device
        hep = L - (gap_len + 1) - 1
        pos = torch.full((B,), hep, dtype=torch.int32, device=dev)
        xr = self.net.decode_rows(seqs.clone(), users, pos)
        hip = self.net._hip
        lab0 = labels.to(dev).to(torch.int64).view(B) - 1
        excl = pad_ragged_ids(raw, dev) if use_h else None
        if hip.world > 1:  # rows are data-parallel: every rank scores all rows against its item shard
            g = hip.group
            xr = g.gather_rows(xr)
            lab0_all = g._all_gather(lab0).view(-1)
            if excl is not None:
                w = torch.tensor([excl.shape[1]], device=dev)
                torch.distributed.all_reduce(w, op=torch.distributed.ReduceOp.MAX)
                excl = F.pad(excl, (0, int(w.item()) - excl.shape[1]), value=-1)
                excl = g._all_gather(excl).view(-1, excl.shape[1])
            ref = hip.gather(xr, lab0_all.view(-1, 1))[:, 0].contiguous()
            cnt = hip.count_before(xr, ref, lab0_all, excl)[g.my_slice(B)]
        else:
            ref = hip.gather(xr, lab0.view(B, 1))[:, 0].contiguous()
            cnt = hip.count_before(xr, ref, lab0, excl)
        ranks = (cnt + 1).cpu().numpy()
        labels_np = labels.detach().cpu().numpy().reshape(-1)
        hit_count, rr = 0, []
        for i in range(B):
            if use_h:
                h = raw[i].detach().cpu().numpy() if torch.is_tensor(raw[i]) else np.asarray(raw[i])
                if labels_np[i] in h:  # label filtered out: neither a hit nor an rr entry (:383-389)
                    continue
            if ranks[i] <= top_k:
                hit_count += 1
            rr.append(np.reciprocal(float(ranks[i])))
        return hit_count, np.array(rr)

    @_takes_offer
    def predict_next(self, raw, seqs, users, top_k=20, gap_len=20, use_h=True):
        """The top_k items the model would show each user next (extension; the baselines' predict_next, reference sas.py:357-388):
        int64 [B, top_k] of 1-based ids, best first, 0 where fewer exist.  It is the list get_accuracy_metrics_in_batch cuts
        top_k_items from (reference :375-383): row L - gap_len - 2 of the decoder, the raw history `raw` (a list of B arrays /
        tensors of 1-based ids) left out when use_h, nothing left out otherwise -- the reference filters no window here.  Exact
        whatever the history hides of the top 100 (irs_recommend).  self.last_recommend holds ids, scores, log_probs, count and
        status of the call.  `raw` is bound as an exclusion set for the call and unbound afterwards, as
        get_seq_in_batch(exclude=) does.  offer=None (keyword only, taken by _takes_offer; 1-based item ids): the slate is taken from these items
        only (irs_bind_offer_set, bound for the call); count is then the number of admissible items of the set, cut at top_k, and
        log_probs stay the model's over the whole catalog.  One device holds the catalog."""
        hip = self.net._hip
        if hip.world != 1:
            raise ValueError("predict_next is not built for an item-sharded catalog")
        dev = seqs.device
        B, L = seqs.shape
        if not 1 <= int(top_k) <= 100:
            raise ValueError(f"top_k={top_k!r}: 1 to 100 items (the ranked list a slate is taken from holds 100)")
        if use_h:
            if len(raw) != B:
                raise ValueError(f"raw: {len(raw)} histories for {B} users")
            longest = max([len(a) for a in raw] + [0])
            if longest > 4096:
                raise ValueError(f"raw: a history of {longest} ids, irs_bind_exclusions takes at most 4096 per user")
        if dev.type != "cuda" or next(self.net.parameters()).device.type != "cuda":
            raise ValueError("predict_next runs on the HIP engine only: move the network and its batch to a GPU (there is no "
                             "CPU fallback in this package)")
        excl = pad_ragged_ids(raw, dev) if use_h else None
        self.net.eval()
        pos = torch.full((B,), L - (gap_len + 1) - 1, dtype=torch.int32, device=dev)
        xr = self.net.decode_rows(seqs.clone(), users, pos)
        eng = hip.get(B, B)
        off = offer_ids0(self._call_offer, eng.n_item, dev)
        held = eng.bind_exclusions(excl, B) if excl is not None else None
        held_off = None
        try:
            held_off = eng.bind_offer_set(off, B) if off is not None else None
            val, ids0, lp, count, status = eng.recommend(xr, int(top_k), k=100, sweep=hip.sweep)
        finally:
            if held_off is not None:
                held_off.record_stream(torch.cuda.current_stream(dev))
                eng.unbind_offer_set()
            if held is not None:
                held.record_stream(torch.cuda.current_stream(dev))
                eng.unbind_exclusions()
        ids = ids0 + 1  # (-1 behind count: 0, the pad id)
        self.last_recommend = dict(ids=ids, scores=val, log_probs=lp, count=count, status=status)
        return ids

    REPLAY_CHUNK = 4096  # rows per pass of replay_paths: one decode and one catalog sweep each

    def replay_paths(self, seqs, users, paths, gap_len=0):
        """The path trace of SAVED paths (extension; irs_replay_paths, the search loops' layout): what get_seq_in_batch(trace=True)
        leaves in self.last_trace, for paths from any search -- greedy, beam, the sharded loops' front end, paths_d_<n>.npy.
        seqs [B, L] are the search's input windows (target in the last slot, gap_len as passed to the search), paths [B, P] the
        chosen items (float or integer, 0 = nothing).  A path is teacher-forced, so all steps of all users are decoded and
        scored in one batch: user b's rows run up to and including its arrival (the first entry equal to its target), or over
        its entries before the first 0.  Returns path_trace_summary's dict: lp_item, lp_target, rank_target [B, P] cut behind
        the live steps, n_steps [B], ioi, ior, avg_lp_item.  One device holds the catalog."""
        hip = self.net._hip
        if hip.world != 1:
            raise ValueError("replay_paths is not built for an item-sharded catalog: irs_replay_paths needs the whole catalog "
                             "on one device")
        dev = seqs.device
        if dev.type != "cuda":
            raise ValueError("replay_paths runs on the HIP engine only: move the network and its batch to a GPU (there is no "
                             "CPU fallback in this package)")
        self.net.eval()
        B, L = seqs.shape
        paths_np = np.asarray(paths.detach().cpu().numpy() if torch.is_tensor(paths) else paths)
        if paths_np.ndim != 2 or paths_np.shape[0] != B:
            raise ValueError(f"replay_paths: paths must be [B = {B}, P], got {paths_np.shape}")
        items = paths_np.astype(np.int64)
        P = items.shape[1]
        targets = seqs[:, -1].detach().cpu().numpy()
        n_live = np.zeros(B, dtype=np.int64)
        for i in range(B):
            zero = np.where(items[i] == 0)[0]
            n_live[i] = zero[0] if len(zero) else P
            pos = get_item_index(items[i, :n_live[i]], targets[i])
            if pos != -1:
                n_live[i] = pos + 1
        if int(n_live.min()) < 1:
            raise ValueError("replay_paths: every path needs at least one step")
        n_t = torch.from_numpy(n_live)
        R = int(n_live.sum())
        row_user = torch.repeat_interleave(torch.arange(B), n_t)
        row_step = torch.arange(R) - torch.repeat_interleave(torch.cumsum(n_t, 0) - n_t, n_t)
        chunk = min(R, self.REPLAY_CHUNK)
        eng = hip.get(chunk, chunk)
        hep0 = torch.full((B,), L - (gap_len + 1) - 1, dtype=torch.int32, device=dev)
        lp_item, lp_target, rank, status = eng.replay_paths(
            IRS_REPLAY_SLOT, seqs.to(torch.int64).contiguous(), torch.from_numpy(items).to(dev), row_user.to(torch.int32).to(dev),
            row_step.to(torch.int32).to(dev), hep0=hep0, users=users.to(dev).to(torch.int64), chunk=chunk)
        if int(status.ne(0).sum().item()) > 0:
            raise IndexError("replay_paths: a path item outside [1, n_item], or gap_len outside the window")
        out = [np.zeros((B, P), dtype=np.float32), np.zeros((B, P), dtype=np.float32), np.zeros((B, P), dtype=np.int32)]
        ru, rs = row_user.numpy(), row_step.numpy()
        for a, v in zip(out, (lp_item, lp_target, rank)):
            a[ru, rs] = v.cpu().numpy()
        return path_trace_summary(*out, items, targets, n_live=n_live)

    def _beam_paths(self, seqs, users, max_path_len, gap_len, beam_width, beam_stop=None, exact_candidates=False, excl=None,
                    beam_trace=False, rule=None):
        """Best-beam paths [B, P] + status via the build-defined beam search (no reference
        counterpart; beam_width == 1 equals the greedy search).  All beams and their
        cumulative log-probabilities are kept in self.last_beams = (paths[B,W,P], scores[B,W]).
        beam_stop "best" / "all": irs_beam_search_until -- a beam ends at its target, finished users are retired;
        self.last_beam_stop = dict(finished [B,W], steps, window_steps).
        beam_trace (one device): the search also returns the three [B, W, P] arrays of irs_bind_beam_trace, the last value.
        rule (one device): beam_rule_kwargs' keywords, the beam rule of this call (irs_set_beam_rule)."""
        B, L = seqs.shape
        dev = seqs.device
        hip = self.net._hip
        W = beam_width
        hep = torch.full((B,), L - (gap_len + 1) - 1, dtype=torch.int32, device=dev)
        traced = ()
        if beam_stop is not None:
            eng = hip.get(B * W, B * W)
            paths, scores, status, fin, steps, window_steps, *traced = eng.beam_search_until(
                seqs.contiguous(), users, hep, max_path_len, W, k=100, sweep=hip.sweep, stop_rule=_BEAM_STOP_RULES[beam_stop],
                check_every=BEAM_STOP_CHECK_EVERY, exact_candidates=exact_candidates, trace=beam_trace, **(excl or {}),
                **(rule or {}))
            self.last_beam_stop = dict(finished=fin.detach().cpu().numpy(), steps=steps, window_steps=window_steps)
        elif hip.world == 1:
            eng = hip.get(B * W, B * W)
            paths, scores, status, *traced = eng.beam_search(seqs.contiguous(), users, hep, max_path_len, W, k=100, sweep=hip.sweep,
                                                             exact_candidates=exact_candidates, trace=beam_trace, **(excl or {}),
                                                             **(rule or {}))
        else:  # item-sharded: the whole loop runs below the C ABI (irs_beam_search_sharded: row all-gather, packed top-100
            # all-to-all, log-sum-exp all-reduce per step, one stream-ordered sequence; captured into a hipGraph over RCCL)
            eng = hip.get(B * W, B * W * hip.world)
            # (replaying the step from a hipGraph with the RCCL calls inside is covered by one-rank tests only: opt in with
            #  IRS_SHARDED_GRAPH=1 once a multi-device capture run is on record -- the same switch bench.py honours)
            paths, scores, status = eng.beam_search_sharded(hip.comm, seqs.contiguous(), users, hep, max_path_len, W, k=100,
                                                            sweep=hip.sweep, split_decode=False,
                                                            use_graph=hip.comm.is_rccl and _SHARDED_GRAPH)
        self.last_beams = (paths.detach().cpu().numpy(), scores.detach().cpu().numpy())
        return paths, status, (traced[0] if traced else None)

    @_takes_exact_candidates
    def get_seq_in_batch(self, seqs, users, targets, max_path_len=20, gap_len=20, sample=False, sample_k=3,
                         beam_width=1, stop_at_target=False, beam_stop=None):
        """Persuasion-path generation (reference :392-470): returns
        (paths float32 [B, max_path_len], targets int64 [B], list of B history arrays, n_early_success).
        beam_width > 1 (extension, not in the reference) returns the best beam's path.
        stop_at_target=True (extension; greedy / sampled search on one device): a user is no longer decoded once its path has
        reached the window's target, and the search returns when nobody is left (irs_generate_paths_until).  Same return
        values: the reference computes those steps and zeroes them here, on the host.
        beam_stop="best" / "all" (extension; beam_width > 1 on one device): the beam search with the window's target as its end
        symbol (irs_beam_search_until) -- a beam that has chosen the target is frozen and competes with its final score, and a
        user is retired once its best beam is finished ("best") or all its live beams are ("all").  A different search from
        beam_stop=None, not the same paths cut short; self.last_beam_stop holds which beams finished and the work done.
        exact_candidates=True (extension, keyword only, taken by _takes_exact_candidates; one device, off by default): a row
        whose top-100 candidates are hidden by its window chooses among the exact best admissible items of the whole catalog
        (irs_bind_survivor_scratch), so the search returns what it would return with k = n_item; the IndexError below remains
        only for a catalog contained in the window.
        exclude=None, no_repeat=False (extension, keyword only, taken the same way; one device, off by default): never offer
        an item the user has already seen (irs_bind_exclusions).  exclude: a list of B arrays / tensors of 1-based ids like
        `raw`, or a [B, E] tensor padded with 0; every step then drops window + the user's list.  no_repeat=True also drops
        the path so far, and adds the user's initial window to its list: the search never offers anything the window ever held
        nor anything it chose itself.  At most 4096 ids per user, the window's included.  A target that is in the user's
        list can no longer be reached.  Combine with exact_candidates=True: a long list regularly hides the whole top-100.
        trace=True (extension, keyword only, taken the same way; greedy / sampled search on one device): the search records,
        at every step and before it chooses, the log-probability and the rank of the target and the log-probability of the item
        it then chose, under this model's softmax over the whole catalog (irs_bind_path_trace).  The return value is unchanged;
        self.last_trace is path_trace_summary's dict: lp_item, lp_target, rank_target [B, max_path_len] cut after the arrival,
        n_steps [B], ioi, ior, avg_lp_item.
        guide=None, guide_k=5 (extension, keyword only, taken the same way; greedy search on one device, off by default): the
        Rec2Inf choice on IRN's own ranking (irs_bind_guide).  guide: a [n_item + 1, F] feature table on the net's device, row i
        = the 1-based item i; integer / bool: binary features, Hamming distance; floating: squared Euclidean distance.  Every
        step then offers, among its first guide_k admissible top-100 candidates, the one nearest to the user's target (ties: the
        better rank) instead of the first.  model/rec2inf.py is the same rule on the plain recommender.
        arrive_rank=None, arrive_lp=None (extension, keyword only, taken the same way; greedy / sampled search on one device,
        off by default): the arrival rule (irs_set_arrival_rule).  A recommender shows a slate, so a user counts as arrived at
        the first step where the target stands at rank <= arrive_rank (>= 1) among what its window leaves, or where the model
        gives it a log-probability >= arrive_lp (<= 0): the step then offers the target itself.  With stop_at_target=True the
        user is retired there.  rank_admissible=True (needs trace=True or an arrival keyword) records the ADMISSIBLE rank as well
        (irs_bind_trace_admissible): self.last_trace["rank_adm"] [B, max_path_len], the target's rank among what exclude,
        no_repeat, the window and offer leave -- its position in the slate the user would be shown -- and
        self.last_trace["slate_step"](r), the first step of every user with rank_adm <= r (-1: none); arrive_among="admissible"
        (needs rank_admissible=True, else ValueError) makes arrive_rank read that rank instead of the window's.
        The keywords imply trace=True: self.last_trace is filled, and its `offered` (bool [B]) says for
        whom the rule fired.  A target that the window, the exclusion list or (no_repeat) the path hides is never offered.
        lookahead=None, lookahead_record=False (extension, keyword only, taken the same way; greedy search on one device, off by
        default): the one-step lookahead choice (irs_bind_lookahead).  lookahead=k_c in [1, 32]: every step decodes, for each
        of its first k_c admissible top-100 candidates, the window the user would have after accepting it, and offers the
        candidate under which the model gives the target the highest log-probability at the NEXT step (ties: the better rank;
        the target itself, once among the candidates, is offered outright).  k_c = 1 is the greedy search.  A step then decodes
        B (1 + k_c) windows and runs one more float32 catalog pass.  Not with guide, sample=True or beam_width > 1.
        lookahead_record=True: self.last_lookahead = dict(items int32 [B, max_path_len, k_c] -- each step's candidates, 1-based,
        0 = none -- and lp float32 [B, max_path_len, k_c], the values compared), cut to 0 after the arrival like last_trace.
        beam_trace=False, beam_pick="score" (extension, keyword only, taken the same way; beam_width > 1 on one device, off by
        default): the beam search carries the trace of every beam through its state (irs_bind_beam_trace), with or without
        beam_stop.  self.last_beam_trace = dict(lp_item, lp_target, rank_target [B, W, max_path_len], cut to 0 after each beam's
        arrival; paths, scores; n_steps [B, W]; picked [B]).  beam_pick="target" (needs beam_trace=True) returns, per user,
        the beam pick_beam names instead of beam 0: the live beam that reaches the target first, else the one that ends with the
        target most probable.  The returned tuple keeps its shape.
        beam_arrive_rank=None, beam_arrive_lp=None, beam_target_weight=0.0 (extension, keyword only, taken the same way; beam_width
        > 1 on one device with beam_trace=True, off by default): the beam rule (irs_set_beam_rule), with or without beam_stop.  A
        beam whose target stands at rank <= beam_arrive_rank among what its window leaves, or at log-probability >=
        beam_arrive_lp, is offered the target itself (with beam_stop it ends there); the candidates of a step are ordered by
        acceptance score + beam_target_weight * lp_target of their parent, while the returned scores stay acceptance sums (with
        a weight they need not be descending).  Without beam_trace=True the library refuses (IrsError).  self.last_beam_trace
        gains arrival_step int64 [B, W] (-1: the beam never holds the target) and offered bool [B, W], both computed from the
        recorded arrays (beam_rule_summary).
        offer=None (extension, keyword only, taken the same way; one device, off by default): the offer set (irs_bind_offer_set).
        offer: 1-based item ids, a tensor, an array or a list, shared by all users; every step of every search form then offers
        items of the set only -- the persuasion path is made of items that may be shown.  A target outside the set is never
        offered: put it in the set to make it reachable.  What describes the model (last_trace, beam scores, the lookahead's
        and the arrival rule's values) stays a statement about the whole catalog.  Combine with exact_candidates=True where
        the window can hide the best 100 of a small set.
        temperature=None, top_p=None, draw_k=None, draw_record=False (extension, keyword only, taken the same way; greedy search
        on one device, off by default): any of the first three binds the sampler (irs_bind_sampler) for the call, the others at
        their defaults temperature 1, top_p 1, draw_k 3: every step draws among its first draw_k admissible candidates with
        weights exp((score - best score) / temperature), cut to the smallest head that holds top_p of the weight; the draws
        are keyed by (seed, user row, step), so stop_at_target=True draws what stop_at_target=False draws.  Not with
        sample=True (ValueError: two samplers), guide, lookahead, beam_width > 1 or a sharded catalog.  draw_record=True:
        self.last_draws = dict(u, lq float32 [B, max_path_len], support int32 [B, max_path_len]): every step's draw, the chosen
        item's log-probability under the distribution it was drawn from, and the candidates the nucleus kept; cut to 0 after
        the arrival like last_trace."""
        opts = self._search_options
        greedy_kw = search_option_kwargs(opts, beam_width, sample, self.net._hip.world)
        rule = beam_rule_kwargs(opts, beam_width, self.net._hip.world)
        exact_candidates, exclude, no_repeat = opts.exact_candidates, opts.exclude, opts.no_repeat
        trace, lookahead = greedy_kw["trace"], greedy_kw.get("lookahead")
        if stop_at_target and beam_width > 1:
            raise ValueError("stop_at_target is not built for beam search (beam_width > 1): irs_beam_search runs every step")
        if beam_stop is not None:
            if beam_stop not in _BEAM_STOP_RULES:
                raise ValueError(f"beam_stop={beam_stop!r}: use \"best\", \"all\" or None (irs_beam_search, every step)")
            if beam_width == 1:
                raise ValueError("beam_stop needs beam_width > 1: use stop_at_target=True for the greedy / sampled search")
            if self.net._hip.world != 1:
                raise ValueError("beam_stop is not built for an item-sharded catalog: use beam_stop=None "
                                 "(irs_beam_search_sharded runs every step)")
        self.net.eval()
        B, L = seqs.shape
        dev = seqs.device
        hip = self.net._hip
        if sample and sample_k > 8:
            raise ValueError("sample_k > 8 is not supported by the HIP path step (include/irs_hip.h)")
        work = seqs.to(torch.int64).clone(memory_format=torch.contiguous_format)  # the search updates it in place
        hep = torch.full((B,), L - (gap_len + 1) - 1, dtype=torch.int32, device=dev)
        sampler = greedy_kw.get("sampler")
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if sample or sampler is not None else 0
        ids0 = exclusion_ids0(exclude, no_repeat, seqs, L - (gap_len + 1) - 1, dev)
        excl = dict(exclude=ids0, no_repeat=no_repeat) if (ids0 is not None or no_repeat) else {}
        off = offer_ids0(opts.offer, self.n_item, dev)
        off = dict(offer=off) if off is not None else {}
        n_eng = B * (lookahead or 1)  # (the children of a lookahead step are decoded and scored in one call each)
        if beam_width > 1:
            all_paths, status, beam_traced = self._beam_paths(work, users, max_path_len, gap_len, beam_width, beam_stop, exact_candidates,
                                                              {**excl, **off}, opts.beam_trace, rule)
            paths_t = all_paths[:, 0].contiguous()
            if opts.beam_trace:  # (what beam_pick="target" names is decided on the host, from the trace as the caller will see it)
                allp, alls = self.last_beams
                self.last_beam_trace = beam_trace_summary(*(a.detach().cpu().numpy() for a in beam_traced), allp, alls,
                                                          targets.detach().cpu().numpy())
                bt = self.last_beam_trace
                pick = pick_beam(allp, alls, bt["lp_target"], bt["n_steps"], targets.detach().cpu().numpy(), opts.beam_pick)
                self.last_beam_trace["picked"] = pick
                if rule:
                    self.last_beam_trace.update(beam_rule_summary(bt, targets.detach().cpu().numpy(), rule["arrive_rank"],
                                                                  rule["arrive_lp"]))
                paths_t = all_paths[torch.arange(B, device=dev), torch.from_numpy(pick).to(dev)].contiguous()
        elif stop_at_target:
            if hip.world != 1:
                raise ValueError("stop_at_target is not built for an item-sharded catalog: irs_generate_paths_sharded runs "
                                 "every step")
            eng = hip.get(n_eng, n_eng)
            paths_t, status, _, _, *traced = eng.generate_paths_until(work, users, hep, max_path_len, k=100, sweep=hip.sweep,
                                                                      sample=sample, sample_k=sample_k, seed=seed,
                                                                      check_every=STOP_CHECK_EVERY, **excl, **off, **greedy_kw)
        elif hip.world == 1:
            eng = hip.get(n_eng, n_eng)
            paths_t, status, *traced = eng.generate_paths(work, users, hep, max_path_len, k=100, sweep=hip.sweep,
                                                          sample=sample, sample_k=sample_k, seed=seed, use_graph=False, **excl,
                                                          **off, **greedy_kw)
        else:  # item-sharded: irs_generate_paths_sharded (decode, row all-gather, shard sweep, key all-to-all, merge, path
            # step per search step, below the C ABI on one stream)
            eng = hip.get(B, B * hip.world)
            paths_t, status = eng.generate_paths_sharded(hip.comm, work, users, hep, max_path_len, k=100, sweep=hip.sweep,
                                                         sample=sample, sample_k=sample_k, seed=seed, use_graph=False)
        if int((status & IRS_ROW_NO_CANDIDATE).sum().item()) > 0:
            if off and not excl:
                raise IndexError("index 0 is out of bounds: every item of the offer set is already in the window"
                                 + ("" if exact_candidates else " (among its best 100)"))
            if excl:
                raise IndexError("index 0 is out of bounds: every admissible item is excluded (window + exclusion list"
                                 + (" + path)" if no_repeat else ")") + ("" if exact_candidates else " among the top-100 candidates"))
            raise IndexError("index 0 is out of bounds: every top-100 candidate is already in the window "
                             "(same condition as reference influentialRS.py:429)" if not exact_candidates else
                             "index 0 is out of bounds: every item of the catalog is already in the window")
        n_early_success = 0
        paths = paths_t.detach().cpu().numpy()
        targets = targets.detach().cpu().numpy()
        if trace:
            tr = [a.detach().cpu().numpy() for a in traced[0]]  # (a fourth array: rank_adm, under rank_admissible=True)
            self.last_trace = path_trace_summary(*tr[:3], paths, targets, rank_adm=tr[3] if len(tr) > 3 else None)
            self.last_trace["offered"] = (status & IRS_ROW_OFFERED).ne(0).detach().cpu().numpy()
        if lookahead is not None and opts.lookahead_record:
            items, lp = (a.detach().cpu().numpy().copy() for a in traced[-1])
            for i in range(B):  # (cut after the arrival, like last_trace)
                pos = get_item_index(paths[i], targets[i])
                if pos != -1:
                    items[i, pos + 1:] = 0
                    lp[i, pos + 1:] = 0
            self.last_lookahead = dict(items=items, lp=lp)
        if sampler is not None and sampler.record:
            u, lq, support = (a.detach().cpu().numpy().copy() for a in traced[-1])
            for i in range(B):  # (cut after the arrival, like last_trace)
                pos = get_item_index(paths[i], targets[i])
                if pos != -1:
                    u[i, pos + 1:] = 0
                    lq[i, pos + 1:] = 0
                    support[i, pos + 1:] = 0
            self.last_draws = dict(u=u, lq=lq, support=support)
        histories = seqs[:, :-1].detach().cpu().numpy()
        actual_history = []
        for i in range(B):
            pos = get_item_index(paths[i], targets[i])
            if pos != -1:
                n_early_success += 1
                paths[i][pos + 1:] = 0
            actual_history.append(histories[i][histories[i] != 0])
        return paths, targets, actual_history, n_early_success


# the options of the running call under the keywords' own names, read-only: irn._trace, irn._guide_k, ... (False / None / 5 between calls)
for _f in dataclasses.fields(SearchOptions):
    setattr(IRSNN, "_" + _f.name, property(lambda self, _n=_f.name: getattr(self._search_options, _n)))
