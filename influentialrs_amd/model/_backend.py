"""Glue between the nn.Module front-ends and the HIP engine: keeps one Engine per
network, (re)binds its parameters when they move or change, and offers the
row-level operations the task handlers need.  No arithmetic of the hot path is
done in torch here; torch supplies tensors, streams and collectives."""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from .._lib import IRS_MASK_CAUSAL, IRS_MASK_IRN, IRS_SWEEP_BF16
from ..dist import ShardGroup
from ..engine import Comm, Engine, IrsError


class HipBackend:
    def __init__(self, net: nn.Module, mask_mode: int):
        self.net = net
        self.mask_mode = mask_mode
        self.engine: Optional[Engine] = None
        self._fp = None
        self.group: Optional[ShardGroup] = None
        self.sweep = IRS_SWEEP_BF16
        self.rank, self.world = 0, 1
        self._stale = False  # a training entry point ran since the derived weights were built
        self.comm: Optional[Comm] = None  # collectives below the C ABI (item-sharded search loops)
        self.ce_backward = ce_backward_default()

    @property
    def ce_backward(self) -> str:
        """Backward of projection + cross entropy: "chunked" (irs_ce_grad_logits per row chunk + torch GEMMs) or "fused"
        (irs_ce_backward: no dL/dlogits buffer).  Default from IRS_CE_BACKWARD."""
        return self._ce_backward

    @ce_backward.setter
    def ce_backward(self, v: str):
        self._ce_backward = check_ce_backward(v)

    def __deepcopy__(self, memo):
        """copy.deepcopy(net): the copy gets its own backend and builds its own engine on first use (an engine is a
        handle to device state bound to THIS module's parameter storage; it is never shared or copied)."""
        import copy
        new = HipBackend.__new__(HipBackend)
        memo[id(self)] = new
        new.net = copy.deepcopy(self.net, memo)
        new.mask_mode, new.sweep = self.mask_mode, self.sweep
        new.engine, new._fp, new.group, new._stale, new.comm = None, None, None, False, None
        new.rank, new.world = self.rank, self.world
        new._ce_backward = self._ce_backward
        return new

    def set_sharding(self, rank: int, world: int, drop_full: bool = True):
        """Item-dimension sharding over `world` ranks (torch.distributed must be
        initialised by the caller when world > 1).  drop_full: keep only the shard's rows of
        project.weight / project.bias in the module (the engine binds local rows either way)."""
        if (rank, world) != (self.rank, self.world):
            self.rank, self.world = rank, world
            self.engine = None
        proj = getattr(self.net, "project", None)
        if drop_full and world > 1 and proj is not None and proj.weight.shape[0] == self.net.n_item:
            from ..engine import shard_bounds
            lo, hi = shard_bounds(self.net.n_item, world, rank)
            with torch.no_grad():
                # shrink the SAME Parameter objects: optimizers built earlier (InfluentialNet.__init__, IRSNN, Evaluator)
                # keep pointing at live tensors, and no reference to the full [n_item, d] storage survives
                for p_ in (proj.weight, proj.bias):
                    p_.data = p_.data[lo:hi].clone()
                    p_.grad = None
                proj.out_features = hi - lo
            self._fp = None

    def holds_shard(self) -> bool:
        """Item-sharded AND the module's own project.* are cut down to this rank's rows (set_sharding with drop_full): the
        loss then has to be the vocabulary-parallel one (project_ce_sharded)."""
        proj = getattr(self.net, "project", None)
        if self.world <= 1 or proj is None:
            return False
        from ..engine import shard_bounds
        lo, hi = shard_bounds(self.net.n_item, self.world, self.rank)
        return proj.weight.shape[0] == hi - lo < self.net.n_item

    def allreduce_replicated_grads(self):
        """After loss.backward() of a sharded training step: every parameter but project.* is replicated and holds the
        gradient of this rank's rows only -- SUM over torch.distributed, as ONE flat buffer, so that the replicas take
        the same optimizer step.  project.* gradients are complete for the shard (irs_ce_backward_sharded) and stay."""
        import torch.distributed as dist
        grads = [p_.grad for n, p_ in self.net.named_parameters() if not n.startswith("project.") and p_.grad is not None]
        if self.world <= 1 or not grads:
            return
        flat = torch.cat([g.reshape(-1) for g in grads])
        if dist.get_backend() == "gloo" and flat.is_cuda:  # (gloo is only dependable on host tensors: ..dist.ShardGroup)
            h = flat.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
            flat.copy_(h)
        else:
            dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        off = 0
        for g in grads:
            g.copy_(flat[off:off + g.numel()].view_as(g))
            off += g.numel()

    def _fingerprint(self):
        return tuple((t.data_ptr(), t._version) for t in self.net.state_dict(keep_vars=True).values())

    def invalidate(self):
        """Weights were changed behind autograd's back (`.data` writes outside a training step, which bump no version
        counter): the next get() re-binds and re-derives (bf16 catalog, packed decoder streams, captured graphs)."""
        self._stale = True

    def get(self, n_seqs: int, n_rows: int, for_training: bool = False, may_update: bool = True) -> Engine:
        net = self.net
        dev = next(net.parameters()).device
        if dev.type != "cuda":
            raise IrsError("inference runs on the HIP engine only: move the network to a GPU "
                           "(there is no CPU fallback in this package)")
        need_new = (self.engine is None or self.engine.device != dev or self.engine.max_seqs < n_seqs
                    or self.engine.max_rows < n_rows)
        if need_new:
            prev_s = self.engine.max_seqs if self.engine else 0
            prev_r = self.engine.max_rows if self.engine else 0
            self.engine = None
            self.engine = Engine(
                n_item=net.n_item, n_user=getattr(net, "n_user", 0), d=net.embed_dim, max_len=net.max_len,
                n_heads=net.n_heads, ffn_dim=net.ffn_dim, n_layers=net.n_layers,
                u_dim=getattr(net, "u_embed_dim", 0) if self.mask_mode == IRS_MASK_IRN else 0,
                mask_mode=self.mask_mode, device=dev, max_rows=max(n_rows, prev_r, 64),
                max_seqs=max(n_seqs, prev_s, 8), max_k=100, rank=self.rank, world=self.world)
            self._fp = None
            self.group = ShardGroup(self.engine) if self.world > 1 else None
            if self.world > 1 and (self.comm is None or self.comm.device != dev):
                self.comm = Comm(dev)  # RCCL under torch.distributed's nccl backend, gloo callbacks otherwise
        fp = self._fingerprint()
        if for_training and self._fp is not None and [a for a, _ in fp] == [a for a, _ in self._fp]:
            # same storage: the CE entry points read project.* in place, nothing derived is used -- but whatever the
            # caller does with the gradients (an optimizer step, also through .data, which bumps no version counter)
            # leaves the bf16 catalog and the filter's norms behind: the next inference get() re-finalises.  A loss that
            # cannot reach an optimizer (no_grad / nothing requires grad: the Evaluator's eval-only loss, alternating with
            # rankings batch after batch) changes no weight and must not cost a re-pack of a multi-GB catalog every batch.
            self._stale = self._stale or may_update
            return self.engine
        if fp != self._fp or self._stale:
            sd = {k: v.detach() for k, v in net.state_dict(keep_vars=True).items() if v.dtype == torch.float32}
            self.engine.bind_state_dict(sd)
            self._fp = fp
            self._stale = for_training and may_update
        return self.engine

    # ---- row-level helpers (single shard or sharded group) ---------------
    def topk(self, xrows, k=100):
        if self.group is not None:
            return self.group.topk(xrows, k, self.sweep)
        return self.engine.score_topk(xrows, k, self.sweep)

    def gather(self, xrows, ids0):
        return self.group.gather(xrows, ids0) if self.group is not None else self.engine.score_gather(xrows, ids0)

    def count_before(self, xrows, ref_score, ref_id0, excl):
        if self.group is not None:
            return self.group.count_before(xrows, ref_score, ref_id0, excl)
        return self.engine.score_count_before(xrows, ref_score, ref_id0, excl)

    def lse(self, xrows):
        return self.group.lse(xrows) if self.group is not None else self.engine.score_lse(xrows)


class _ProjectCE(torch.autograd.Function):
    """mean over valid rows of CrossEntropy(project(x), label) -- nn.Linear + nn.CrossEntropyLoss of the reference's
    train_batch (influentialRS.py:278-310, evaluator.py:53-68) -- without the [M, n_item] logits: forward =
    irs_ce_forward (float32 log-sum-exp sweep + label gather), backward = irs_ce_grad_logits per row chunk (the
    softmax gradient written once by the sweep's epilogue) followed by the two plain GEMMs dX = G W, dW = G^T X -- or,
    with backend.ce_backward == "fused", irs_ce_backward per block of ROWS rows, which never stores dL/dlogits."""
    ROWS = 8192          # rows per engine call
    CHUNK_BYTES = 1 << 30  # budget of the dL/dlogits chunk

    @staticmethod
    def forward(ctx, x, weight, bias, labels0, backend, may_update):
        M = x.shape[0]
        eng = backend.get(1, min(M, _ProjectCE.ROWS), for_training=True, may_update=may_update)
        xd = x.detach().contiguous()
        lse = torch.empty(M, dtype=torch.float32, device=x.device)
        tot = torch.zeros(3, dtype=torch.float64, device=x.device)
        for c0 in range(0, M, _ProjectCE.ROWS):
            c1 = min(M, c0 + _ProjectCE.ROWS)
            l, _, t = eng.ce_forward(xd[c0:c1], labels0[c0:c1])
            lse[c0:c1] = l
            tot += t
        _, n_valid, n_bad = tot.tolist()  # one host read per loss, as nn.CrossEntropyLoss's own target check costs
        if n_bad > 0:
            raise IndexError(f"Target out of bounds: {int(n_bad)} label(s) >= n_item {weight.shape[0]} (nn.CrossEntropyLoss "
                             "raises here, reference influentialRS.py:270,301)")
        ctx.save_for_backward(xd, weight, labels0, lse, tot)
        ctx.backend = backend
        ctx.n_valid = n_valid
        if n_valid == 0:  # every target is a pad: the reference's mean over an empty selection is nan, its gradient zero
            return torch.full((), float("nan"), dtype=torch.float32, device=x.device)
        return (tot[0] / tot[1]).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        xd, weight, labels0, lse, tot = ctx.saved_tensors
        M, d = xd.shape
        N = weight.shape[0]
        if ctx.n_valid == 0:
            return torch.zeros_like(xd), torch.zeros_like(weight), torch.zeros(N, dtype=torch.float32, device=xd.device), None, None, None
        eng = ctx.backend.get(1, min(M, _ProjectCE.ROWS), for_training=True)
        if ctx.backend.ce_backward == "fused":
            dx = torch.empty_like(xd)
            dW = torch.empty_like(weight)
            db = torch.empty(N, dtype=torch.float32, device=xd.device)
            # (the size follows the split of each pass, which is not monotone in the row count: ask for every block size used)
            blocks = {min(M, _ProjectCE.ROWS), M % _ProjectCE.ROWS or _ProjectCE.ROWS} if M > _ProjectCE.ROWS else {M}
            scratch = torch.empty(max(eng.ce_backward_scratch_bytes(m) for m in blocks), dtype=torch.uint8, device=xd.device)
            for c0 in range(0, M, _ProjectCE.ROWS):
                c1 = min(M, c0 + _ProjectCE.ROWS)
                eng.ce_backward(xd[c0:c1], labels0[c0:c1], lse[c0:c1], 1.0, c0 > 0, dx[c0:c1], dW, db, scratch)
            sc = (g.double() / tot[1]).to(torch.float32)
            return dx.mul_(sc), dW.mul_(sc), db.mul_(sc), None, None, None
        mc = max(32, min(_ProjectCE.ROWS, M, (_ProjectCE.CHUNK_BYTES // (4 * N)) // 32 * 32))
        G = torch.empty((mc, N), dtype=torch.float32, device=xd.device)
        dx = torch.empty_like(xd)
        dW = torch.zeros_like(weight)
        db = torch.zeros(N, dtype=torch.float32, device=xd.device)
        for c0 in range(0, M, mc):
            c1 = min(M, c0 + mc)
            Gc = eng.ce_grad_logits(xd[c0:c1], labels0[c0:c1], lse[c0:c1], 1.0, G)[:c1 - c0]
            torch.mm(Gc, weight, out=dx[c0:c1])
            dW.addmm_(Gc.t(), xd[c0:c1])
            db += Gc.sum(0)
        sc = (g.double() / tot[1]).to(torch.float32)  # dL/dloss / n_valid, kept on the device
        return dx * sc, dW * sc, db * sc, None, None, None


class _ProjectCESharded(torch.autograd.Function):
    """_ProjectCE over an item-sharded catalog: `weight` / `bias` are this rank's rows of project.*, x / labels0 this rank's
    rows of the batch (the SAME number on every rank; labels global), and the loss is the mean over the valid rows of the
    WHOLE world -- identical on every rank.  forward = irs_ce_forward_sharded per row block, backward =
    irs_ce_backward_sharded with `accumulate` across blocks, scaled by g / global n_valid: dx of the own rows, dW / db of
    the own shard over the world's rows (complete: never reduced over ranks).  Both ce_backward settings take this route:
    under sharding "chunked" runs the fused kernels too (a dL/dlogits chunk of the world's rows per rank is what sharding
    is there to avoid).  A block is ROWS / world rows per rank, so the engine's workspace is that of the unsharded loss."""

    @staticmethod
    def _block(world):
        return max(1, _ProjectCE.ROWS // world)

    @staticmethod
    def forward(ctx, x, weight, bias, labels0, backend, may_update):
        M = x.shape[0]
        blk = _ProjectCESharded._block(backend.world)
        eng = backend.get(1, backend.world * min(M, blk), for_training=True, may_update=may_update)
        xd = x.detach().contiguous()
        lse = torch.empty(M, dtype=torch.float32, device=x.device)
        tot = torch.zeros(3, dtype=torch.float64, device=x.device)
        for c0 in range(0, M, blk):
            c1 = min(M, c0 + blk)
            l, _, t = eng.ce_forward_sharded(backend.comm, xd[c0:c1], labels0[c0:c1])
            lse[c0:c1] = l
            tot += t
        _, n_valid, n_bad = tot.tolist()  # (the triple is the world's: every rank takes the same branch below)
        if n_bad > 0:
            raise IndexError(f"Target out of bounds: {int(n_bad)} label(s) >= n_item {backend.net.n_item} (nn.CrossEntropyLoss "
                             "raises here, reference influentialRS.py:270,301)")
        ctx.save_for_backward(xd, weight, labels0, lse, tot)
        ctx.backend = backend
        ctx.n_valid = n_valid
        if n_valid == 0:
            return torch.full((), float("nan"), dtype=torch.float32, device=x.device)
        return (tot[0] / tot[1]).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        xd, weight, labels0, lse, tot = ctx.saved_tensors
        M, d = xd.shape
        N = weight.shape[0]
        if ctx.n_valid == 0:
            return torch.zeros_like(xd), torch.zeros_like(weight), torch.zeros(N, dtype=torch.float32, device=xd.device), None, None, None
        backend = ctx.backend
        blk = _ProjectCESharded._block(backend.world)
        eng = backend.get(1, backend.world * min(M, blk), for_training=True)
        dx = torch.empty_like(xd)
        dW = torch.empty_like(weight)
        db = torch.empty(N, dtype=torch.float32, device=xd.device)
        blocks = {min(M, blk), M % blk or blk} if M > blk else {M}
        scratch = torch.empty(max(eng.ce_backward_sharded_scratch_bytes(m) for m in blocks), dtype=torch.uint8, device=xd.device)
        for c0 in range(0, M, blk):
            c1 = min(M, c0 + blk)
            eng.ce_backward_sharded(backend.comm, xd[c0:c1], labels0[c0:c1], lse[c0:c1], 1.0, c0 > 0, dx[c0:c1], dW, db, scratch)
        sc = (g.double() / tot[1]).to(torch.float32)
        return dx.mul_(sc), dW.mul_(sc), db.mul_(sc), None, None, None


def project_ce_sharded(x: torch.Tensor, project: nn.Linear, labels0: torch.Tensor, backend: "HipBackend") -> torch.Tensor:
    """project_ce for a module that holds only its shard of project.* (HipBackend.holds_shard): the global loss, the same
    scalar on every rank.  Every rank calls it together, with the same number of rows."""
    may_update = torch.is_grad_enabled() and (x.requires_grad or project.weight.requires_grad or project.bias.requires_grad)
    return _ProjectCESharded.apply(x, project.weight, project.bias, labels0, backend, may_update)


def project_ce(x: torch.Tensor, project: nn.Linear, labels0: torch.Tensor, backend: "HipBackend") -> torch.Tensor:
    """Scalar loss; x [M, d] rows of the decoder, labels0 [M] 0-based with -1 = ignored."""
    # (grad mode is off inside Function.forward: whether this loss can lead to a weight update is decided here)
    may_update = torch.is_grad_enabled() and (x.requires_grad or project.weight.requires_grad or project.bias.requires_grad)
    return _ProjectCE.apply(x, project.weight, project.bias, labels0, backend, may_update)


CE_BACKWARDS = ("chunked", "fused")


def ce_backward_default() -> str:
    """The projection + cross-entropy backward a new network selects: IRS_CE_BACKWARD = chunked (default) or fused
    (include/irs_hip.h irs_ce_backward).  Any other value raises."""
    return check_ce_backward(os.environ.get("IRS_CE_BACKWARD", "chunked"), "IRS_CE_BACKWARD")


def check_ce_backward(v, what: str = "ce_backward") -> str:
    if v not in CE_BACKWARDS:
        raise ValueError(f"{what} must be one of {CE_BACKWARDS}, got {v!r}")
    return v


TRUNKS = ("torch", "hip")


def train_trunk_default() -> str:
    """The training trunk a new network selects: IRS_TRAIN_TRUNK = torch (default: stock nn.TransformerDecoder autograd) or
    hip (the native trunk of include/irs_hip.h irs_train_*).  Any other value raises."""
    v = os.environ.get("IRS_TRAIN_TRUNK", "torch")
    return check_trunk(v, "IRS_TRAIN_TRUNK")


def check_trunk(v, what: str = "trunk") -> str:
    if v not in TRUNKS:
        raise ValueError(f"{what} must be one of {TRUNKS}, got {v!r}")
    return v


class _TrunkHip(torch.autograd.Function):
    """The train-mode decoder trunk (embedding, dropout, n_layers nn.TransformerDecoderLayer over the zero memory) on the
    native kernels: forward = irs_train_forward (keeps its saved state), backward = irs_train_backward, whose gradient arena
    is handed to autograd per parameter so that .grad accumulates as with the stock modules."""

    @staticmethod
    def forward(ctx, seq, user, p, seed, backend, names, *params):
        eng = backend.get(1, 1, for_training=True)
        x, saved = eng.train_forward(seq, user, p, seed)
        ctx.save_for_backward(seq, user if user is not None else seq, saved)
        ctx.has_user = user is not None
        ctx.p, ctx.seed, ctx.backend, ctx.names = p, seed, backend, names
        ctx.shapes = [prm.shape for prm in params]
        return x

    @staticmethod
    def backward(ctx, gx):
        seq, user, saved = ctx.saved_tensors
        eng = ctx.backend.get(1, 1, for_training=True)
        g = eng.train_backward(seq, user if ctx.has_user else None, ctx.p, ctx.seed, saved, gx.contiguous())
        grads = []
        for name, shape in zip(ctx.names, ctx.shapes):
            off = eng.train_grad_offset(name)
            grads.append(g[off:off + shape.numel()].view(shape))
        return (None, None, None, None, None, None) + tuple(grads)


def _trunk_params(net: nn.Module, emb_name: str):
    out = [(n, p_) for n, p_ in net.named_parameters() if n == emb_name or n.startswith("decoder.layers.")]
    return [n for n, _ in out], [p_ for _, p_ in out]


def trunk_hip(net: nn.Module, seq: torch.Tensor, user: Optional[torch.Tensor], emb_name: str) -> torch.Tensor:
    """[B, L, d] decoder output of the train-mode trunk on the native kernels (net.trunk == "hip")."""
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        raise IrsError("trunk='hip' runs the decoder trunk on the HIP engine: move the network to a GPU "
                       "(or select trunk='torch')")
    p = float(net.dropout) if net.training else 0.0
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout p={p} outside [0, 1)")
    # one 62-bit dropout key per step from torch's default CPU generator: torch.manual_seed / utils.set_seed make runs
    # reproducible, and no device sync is needed
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    names, params = _trunk_params(net, emb_name)
    seq = seq.contiguous().to(torch.int64)
    user = user.contiguous().to(torch.int64) if user is not None else None
    return _TrunkHip.apply(seq, user, p, seed, net._hip, names, *params)


def pad_ragged_ids(lists: Sequence, device, minus: int = 1) -> torch.Tensor:
    """List of 1-based id sequences -> int64 [B, n] of 0-based ids, -1 padded."""
    n = max([len(a) for a in lists] + [1])
    out = np.full((len(lists), n), -1, dtype=np.int64)
    for i, a in enumerate(lists):
        a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.int64)
        out[i, :len(a)] = a - minus
    return torch.from_numpy(out).to(device)


def make_scheduler(optimizer):
    """ReduceLROnPlateau(factor=0.5, patience=4) as the reference builds it
    (influentialRS.py:92-95); its `verbose=True` no longer exists in current torch."""
    from torch.optim import lr_scheduler
    return lr_scheduler.ReduceLROnPlateau(optimizer, factor=0.5, patience=4)
