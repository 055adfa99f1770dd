"""Host-side engine: owns one irs_ctx (one device, one item shard), the derived
weight arena and the workspace (as torch tensors: torch is only the allocator
and stream provider here), and exposes the C-ABI calls on torch tensors.

All methods enqueue work on torch's current stream for the engine's device and
return device tensors; nothing synchronises unless the caller does.
"""
from __future__ import annotations

import contextlib
import ctypes
import dataclasses
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import (IRS_MASK_CAUSAL, IRS_MASK_IRN, IRS_SWEEP_BF16, IRS_SWEEP_EXHAUSTIVE, IRS_SWEEP_F32, IrsDims,
                   IrsShard)


class IrsError(RuntimeError):
    pass


def shard_bounds(n_item: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous item shard [lo, hi) of rank `rank` out of `world`, sizes
    differing by at most one tile-aligned chunk: boundaries are multiples of 32
    items so that every shard but the last is made of whole MFMA tiles."""
    tiles = (n_item + 31) // 32
    per, rem = divmod(tiles, world)
    lo_t = rank * per + min(rank, rem)
    hi_t = lo_t + per + (1 if rank < rem else 0)
    return min(lo_t * 32, n_item), min(hi_t * 32, n_item)


def arrive_among_kind(among: str) -> int:
    """arrive_among="window" | "admissible" as irs_set_arrival_rule_ex's rank_kind; ValueError for anything else."""
    kinds = {"window": _lib.IRS_RANK_WINDOW, "admissible": _lib.IRS_RANK_ADMISSIBLE}
    if among not in kinds:
        raise ValueError(f"arrive_among={among!r}: use \"window\" (rank_target) or \"admissible\" (rank_adm)")
    return kinds[among]


def check_rank_options(trace: bool, rank_admissible: bool, arrive_among: str):
    """The per-call keywords of the greedy loops: rank_admissible adds a column to the path trace, and an arrival rule among the
    admissible reads that column.  ValueError otherwise."""
    arrive_among_kind(arrive_among)
    if rank_admissible and not trace:
        raise ValueError("rank_admissible=True adds a column to the path trace: use trace=True")
    if arrive_among == "admissible" and not rank_admissible:
        raise ValueError("arrive_among=\"admissible\" reads the admissible rank: use rank_admissible=True")


@dataclasses.dataclass(frozen=True)
class Sampler:
    """sampler= of Engine.generate_paths[_until] (irs_bind_sampler): a step draws among its first top_k admissible candidates with
    weights exp((v - v_0) / temperature), cut to the nucleus top_p; record: the call also returns (u, lq, support)."""
    top_k: int
    temperature: float = 1.0
    top_p: float = 1.0
    record: bool = False


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Engine:
    def __init__(self, *, n_item: int, n_user: int, d: int, max_len: int, n_heads: int, ffn_dim: int, n_layers: int,
                 u_dim: int, mask_mode: int, device: torch.device, max_rows: int = 1024, max_seqs: int = 0,
                 max_k: int = 100, rank: int = 0, world: int = 1):
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise IrsError("the HIP engine needs a GPU device (no CPU fallback exists)")
        lo, hi = shard_bounds(n_item, world, rank)
        if hi <= lo:
            raise IrsError(f"rank {rank} of {world} would hold an empty item shard of a {n_item}-item catalog")
        self.item_lo, self.item_hi = lo, hi
        self.n_local = hi - lo
        self.n_item, self.d, self.L = n_item, d, max_len
        self.max_rows, self.max_k = max_rows, max_k
        self.max_seqs = max_seqs or max_rows
        self.mask_mode = mask_mode
        self.world, self.rank = world, rank
        dims = IrsDims(n_item, n_user, d, max_len, n_heads, ffn_dim, n_layers, u_dim, mask_mode, max_rows, max_k,
                       self.max_seqs)
        shard = IrsShard(rank, world, lo, hi)
        h = ctypes.c_void_p()
        self._weights: Dict[str, torch.Tensor] = {}
        with torch.cuda.device(self.device):
            if max_len > 256:  # long windows are opened explicitly (up to IRS_MAX_LEN_LONG; beyond: the library's message)
                rc = self.lib.irs_create_ex(ctypes.byref(h), ctypes.byref(dims), ctypes.byref(shard),
                                            _lib.IRS_CREATE_LONG_WINDOWS)
            else:
                rc = self.lib.irs_create(ctypes.byref(h), ctypes.byref(dims), ctypes.byref(shard))
            if rc != 0:
                raise IrsError(f"irs_create failed ({rc}): {self.lib.irs_last_error(None).decode()}")
            self.h = h
            self._ws = torch.empty(self.lib.irs_workspace_bytes(self.h) + 256, dtype=torch.uint8, device=self.device)
            self._check(self.lib.irs_bind_workspace(self.h, _ptr(self._ws), self._ws.numel()))
        self._arena = None
        self._grad_off: Dict[str, int] = {}  # train_grad_offset cache

    # ------------------------------------------------------------------
    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.irs_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise IrsError(f"libirs_hip error {rc}: {self.lib.irs_last_error(self.h).decode()}")

    def _call(self, fn, *args):
        """Every library entry point launches on the CURRENT HIP device (include/irs_hip.h): make the engine's
        device current around the call, whatever the caller's current device is."""
        with torch.cuda.device(self.device):
            self._check(fn(self.h, *args, self._stream()))

    def _call_sync(self, fn, *args):
        """A synchronous entry point that takes no stream (irs_lookahead_expand / irs_lookahead_choose): the work on torch's
        current stream, which produced the inputs, is drained first; the outputs are complete when the call returns."""
        with torch.cuda.device(self.device):
            torch.cuda.current_stream(self.device).synchronize()
            self._check(fn(self.h, *args))

    def _call_null(self, fn, *args, tensors=()):
        """An entry point that takes no stream and enqueues on the null stream without waiting (irs_recommend, irs_recommend_take).
        On torch's default stream, which is the null stream, that is all.  On any other current stream the default stream waits
        for it first and it waits for the default stream afterwards -- two events, no host wait -- and `tensors` (everything the
        call reads or writes) are marked as used on the default stream."""
        with torch.cuda.device(self.device):
            cur, null = torch.cuda.current_stream(self.device), torch.cuda.default_stream(self.device)
            if cur != null:
                null.wait_stream(cur)
            self._check(fn(self.h, *args))
            if cur != null:
                cur.wait_stream(null)
                for t in tensors:
                    if t is not None:
                        t.record_stream(null)

    def _inplace(self, t: torch.Tensor, dtype, what: str) -> torch.Tensor:
        """A buffer the library updates in place: it must already be what the kernels assume (a copy would
        silently drop the update)."""
        if t.device != self.device or t.dtype != dtype or not t.is_contiguous():
            raise IrsError(f"{what}: need a contiguous {dtype} tensor on {self.device}, got {t.dtype} on {t.device}"
                           f"{'' if t.is_contiguous() else ' (non-contiguous)'}")
        return t

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, t: torch.Tensor, dtype) -> torch.Tensor:
        if t.device != self.device:
            raise IrsError(f"tensor on {t.device}, engine on {self.device}")
        if t.dtype != dtype:
            raise IrsError(f"tensor dtype {t.dtype}, expected {dtype}")
        return t.contiguous()

    # ------------------------------------------------------------------ weights
    def bind_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Bind every tensor of a reference-keyed state_dict.
        project.weight / project.bias may be given whole ([N, d] / [N]); the
        local shard rows are sliced here (a view, no copy)."""
        for name, t in sd.items():
            key = name[7:] if name.startswith("module.") else name
            if key.endswith("multihead_attn.in_proj_weight"):
                pass  # bound for the key-set contract; only its bias slice matters (zero memory)
            if key == "project.weight" and t.shape[0] == self.n_item and self.n_local != self.n_item:
                t = t[self.item_lo:self.item_hi]
            if key == "project.bias" and t.shape[0] == self.n_item and self.n_local != self.n_item:
                t = t[self.item_lo:self.item_hi]
            t = self._dev(t.detach(), torch.float32)
            self._weights[key] = t  # keep alive
            self._check(self.lib.irs_bind_weight(self.h, key.encode(), _ptr(t), t.numel()))
        self.finalize()

    def finalize(self):
        with torch.cuda.device(self.device):
            need = self.lib.irs_derived_bytes(self.h)
            if self._arena is None or self._arena.numel() < need:
                self._arena = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
            self._check(self.lib.irs_finalize_weights(self.h, _ptr(self._arena), self._arena.numel(), self._stream()))

    # ------------------------------------------------------------------ decoder
    def pif(self, users: torch.Tensor) -> torch.Tensor:
        users = self._dev(users, torch.int64)
        out = torch.empty(users.shape[0], dtype=torch.float32, device=self.device)
        self._call(self.lib.irs_pif, _ptr(users), users.shape[0], _ptr(out))
        return out

    def decode(self, seqs: torch.Tensor, users: Optional[torch.Tensor], *, want_x: bool = True,
               pos: Optional[torch.Tensor] = None, want_r_u: bool = False):
        """Returns (x[B,L,d] or None, xrows[B,d] or None, r_u[B] or None)."""
        seqs = self._dev(seqs, torch.int64)
        B, L = seqs.shape
        if L != self.L:
            raise IrsError(f"sequence length {L} != max_len {self.L}")
        if users is not None:
            users = self._dev(users, torch.int64)
        x = torch.empty((B, L, self.d), dtype=torch.float32, device=self.device) if want_x else None
        xr = None
        if pos is not None:
            pos = self._dev(pos, torch.int32)
            xr = torch.empty((B, self.d), dtype=torch.float32, device=self.device)
        ru = torch.empty(B, dtype=torch.float32, device=self.device) if want_r_u else None
        self._call(self.lib.irs_decode, _ptr(seqs), _ptr(users), B, _ptr(x), _ptr(pos), _ptr(xr), _ptr(ru))
        return x, xr, ru

    # ------------------------------------------------------------------ scoring
    def score_topk(self, xrows: torch.Tensor, k: int = 100, sweep: int = IRS_SWEEP_BF16, carry: bool = False):
        """(val[M,k] float32, ids0[M,k] int64 global 0-based, status[M] int32) of this shard.  carry: the rows are the previous
        call's rows one path-search step later -- irs_score_topk_carry reuses that call's emission thresholds (same exact results;
        unrelated rows only cost time)."""
        xrows = self._dev(xrows, torch.float32)
        M = xrows.shape[0]
        val = torch.empty((M, k), dtype=torch.float32, device=self.device)
        ids = torch.empty((M, k), dtype=torch.int64, device=self.device)
        st = torch.empty(M, dtype=torch.int32, device=self.device)
        fn = self.lib.irs_score_topk_carry if (carry and sweep == IRS_SWEEP_BF16) else self.lib.irs_score_topk
        self._call(fn, _ptr(xrows), M, k, sweep, _ptr(val), _ptr(ids), _ptr(st))
        return val, ids, st

    def score_topk_lse(self, xrows: torch.Tensor, k: int = 100, sweep: int = IRS_SWEEP_BF16):
        """score_topk and score_lse out of one call (one pass over the float32 catalog on the swept path):
        (val, ids0, status, max[M], sumexp[M]) of this shard."""
        xrows = self._dev(xrows, torch.float32)
        M = xrows.shape[0]
        val = torch.empty((M, k), dtype=torch.float32, device=self.device)
        ids = torch.empty((M, k), dtype=torch.int64, device=self.device)
        st = torch.empty(M, dtype=torch.int32, device=self.device)
        mx = torch.empty(M, dtype=torch.float32, device=self.device)
        sm = torch.empty(M, dtype=torch.float32, device=self.device)
        self._call(self.lib.irs_score_topk_lse, _ptr(xrows), M, k, sweep, _ptr(val), _ptr(ids), _ptr(st), _ptr(mx), _ptr(sm))
        return val, ids, st, mx, sm

    def score_gather(self, xrows: torch.Tensor, ids0: torch.Tensor) -> torch.Tensor:
        xrows = self._dev(xrows, torch.float32)
        ids0 = self._dev(ids0, torch.int64)
        M, g = ids0.shape
        out = torch.empty((M, g), dtype=torch.float32, device=self.device)
        self._call(self.lib.irs_score_gather, _ptr(xrows), M, _ptr(ids0), g, _ptr(out))
        return out

    def score_count_before(self, xrows, ref_score, ref_id0, excl_ids0: Optional[torch.Tensor]) -> torch.Tensor:
        xrows = self._dev(xrows, torch.float32)
        ref_score = self._dev(ref_score, torch.float32)
        ref_id0 = self._dev(ref_id0, torch.int64)
        M = xrows.shape[0]
        n_ex = 0
        if excl_ids0 is not None:
            excl_ids0 = self._dev(excl_ids0, torch.int64)
            n_ex = excl_ids0.shape[1]
        out = torch.empty(M, dtype=torch.int64, device=self.device)
        self._call(self.lib.irs_score_count_before, _ptr(xrows), M, _ptr(ref_score), _ptr(ref_id0),
                                                    _ptr(excl_ids0) if n_ex else None, n_ex, _ptr(out))
        return out

    def score_dense(self, xrows: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        xrows = self._dev(xrows, torch.float32)
        M = xrows.shape[0]
        if out is None:
            out = torch.empty((M, self.n_local), dtype=torch.float32, device=self.device)
        self._call(self.lib.irs_score_dense, _ptr(xrows), M, _ptr(out), out.stride(0))
        return out

    def score_lse(self, xrows: torch.Tensor):
        xrows = self._dev(xrows, torch.float32)
        M = xrows.shape[0]
        mx = torch.empty(M, dtype=torch.float32, device=self.device)
        sm = torch.empty(M, dtype=torch.float32, device=self.device)
        self._call(self.lib.irs_score_lse, _ptr(xrows), M, _ptr(mx), _ptr(sm))
        return mx, sm

    # ---- projection + cross entropy without the logits (training side)
    def ce_forward(self, xrows: torch.Tensor, labels0: torch.Tensor):
        """(lse[M] float32, label_score[M] float32, loss[3] float64 = {sum over valid rows of lse - label score,
        number of valid rows, number of labels >= n_item}); labels0 int64 0-based, -1 = row ignored."""
        xrows = self._dev(xrows, torch.float32)
        labels0 = self._dev(labels0, torch.int64)
        M = xrows.shape[0]
        lse = torch.empty(M, dtype=torch.float32, device=self.device)
        ls = torch.empty(M, dtype=torch.float32, device=self.device)
        loss = torch.empty(3, dtype=torch.float64, device=self.device)
        self._call(self.lib.irs_ce_forward, _ptr(xrows), _ptr(labels0), M, _ptr(lse), _ptr(ls), _ptr(loss))
        return lse, ls, loss

    def ce_grad_logits(self, xrows: torch.Tensor, labels0: torch.Tensor, lse: torch.Tensor, scale: float, out: torch.Tensor):
        """out[M, ld >= n_local] = scale * (softmax(logits) - onehot(label)); ignored rows 0.  Written in place."""
        xrows = self._dev(xrows, torch.float32)
        labels0 = self._dev(labels0, torch.int64)
        lse = self._dev(lse, torch.float32)
        M = xrows.shape[0]
        if out.dtype != torch.float32 or out.device != self.device or out.dim() != 2 or out.stride(1) != 1 \
                or out.shape[0] < M or out.shape[1] < self.n_local:
            raise IrsError("ce_grad_logits: out must be a float32 [>= M, >= n_local] row-major tensor on the engine's device")
        self._call(self.lib.irs_ce_grad_logits, _ptr(xrows), _ptr(labels0), _ptr(lse), M, float(scale), _ptr(out),
                   int(out.stride(0)))
        return out

    def ce_backward_scratch_bytes(self, M: int) -> int:
        n = self.lib.irs_ce_backward_scratch_bytes(self.h, M)
        if n == 0:
            raise IrsError(f"ce_backward: no scratch size for M={M} (need 1 <= M <= max_rows={self.max_rows})")
        return n

    def ce_backward(self, xrows: torch.Tensor, labels0: torch.Tensor, lse: torch.Tensor, scale: float, accumulate: bool,
                    dx: torch.Tensor, dw: torch.Tensor, db: torch.Tensor, scratch: torch.Tensor):
        """dx[M, d] = G W (overwritten), dw[n_local, d] (+)= G^T X, db[n_local] (+)= colsum G with
        G = scale * (softmax(logits) - onehot(label)), ignored rows 0, never stored (irs_ce_backward).  All three are
        written in place; scratch: uint8, at least ce_backward_scratch_bytes(M) bytes."""
        xrows = self._dev(xrows, torch.float32)
        labels0 = self._dev(labels0, torch.int64)
        lse = self._dev(lse, torch.float32)
        if xrows.dim() != 2 or xrows.shape[1] != self.d:
            raise IrsError(f"ce_backward: rows of shape {tuple(xrows.shape)}, expected [M, {self.d}]")
        M = xrows.shape[0]
        if tuple(labels0.shape) != (M,) or tuple(lse.shape) != (M,):
            raise IrsError(f"ce_backward: labels {tuple(labels0.shape)} / lse {tuple(lse.shape)}, expected [{M}]")
        dx = self._inplace(dx, torch.float32, "ce_backward dx")
        dw = self._inplace(dw, torch.float32, "ce_backward dw")
        db = self._inplace(db, torch.float32, "ce_backward db")
        scratch = self._inplace(scratch, torch.uint8, "ce_backward scratch")
        if tuple(dx.shape) != (M, self.d) or tuple(dw.shape) != (self.n_local, self.d) or tuple(db.shape) != (self.n_local,):
            raise IrsError(f"ce_backward: dx {tuple(dx.shape)} / dw {tuple(dw.shape)} / db {tuple(db.shape)}, expected "
                           f"{(M, self.d)} / {(self.n_local, self.d)} / {(self.n_local,)}")
        self._call(self.lib.irs_ce_backward, _ptr(xrows), _ptr(labels0), _ptr(lse), M, float(scale), 1 if accumulate else 0,
                   _ptr(dx), _ptr(dw), _ptr(db), _ptr(scratch), scratch.numel())
        return dx, dw, db

    # ------------------------------------------------------------------ native training trunk
    def train_saved_bytes(self, B: int, L: int) -> int:
        n = self.lib.irs_train_saved_bytes(self.h, B, L)
        if n == 0:
            raise IrsError(f"train trunk: no saved state for B={B}, L={L} (need 1 <= L <= max_len={self.L})")
        return n

    def train_grad_offset(self, name: str) -> int:
        """Float offset of state_dict key `name` in the gradient arena of train_backward, -1 if it is not a trunk parameter.
        The layout depends on the context's dims only: each name is asked of the library once per engine."""
        off = self._grad_off.get(name)
        if off is None:
            off = self._grad_off[name] = int(self.lib.irs_train_grad_offset(self.h, name.encode()))
        return off

    def train_forward(self, seqs: torch.Tensor, users: Optional[torch.Tensor], p: float, seed: int):
        """Trunk forward of a training step: (x float32 [B, L, d], saved uint8 tensor for train_backward)."""
        seqs = self._dev(seqs, torch.int64)
        users = self._dev(users, torch.int64) if users is not None else None
        B, L = seqs.shape
        saved = torch.empty(self.train_saved_bytes(B, L), dtype=torch.uint8, device=self.device)
        x = torch.empty((B, L, self.d), dtype=torch.float32, device=self.device)
        self._call(self.lib.irs_train_forward, _ptr(seqs), _ptr(users), B, L, float(p), int(seed) & (2 ** 64 - 1), _ptr(saved),
                   saved.numel(), _ptr(x))
        return x, saved

    def train_backward(self, seqs: torch.Tensor, users: Optional[torch.Tensor], p: float, seed: int, saved: torch.Tensor,
                       dx: torch.Tensor) -> torch.Tensor:
        """Every trunk parameter gradient for dL/dx, as one float32 arena (slice it with train_grad_offset)."""
        seqs = self._dev(seqs, torch.int64)
        users = self._dev(users, torch.int64) if users is not None else None
        dx = self._dev(dx, torch.float32)
        B, L = seqs.shape
        if tuple(dx.shape) != (B, L, self.d):
            raise IrsError(f"train_backward: dx shape {tuple(dx.shape)}, expected {(B, L, self.d)}")
        saved = self._inplace(saved, torch.uint8, "train_backward saved state")
        nb = self.lib.irs_train_grad_bytes(self.h)
        grads = torch.empty(nb // 4, dtype=torch.float32, device=self.device)
        self._call(self.lib.irs_train_backward, _ptr(seqs), _ptr(users), B, L, float(p), int(seed) & (2 ** 64 - 1),
                   _ptr(saved), saved.numel(), _ptr(dx), _ptr(grads), nb)
        return grads

    def merge_topk(self, val_in: torch.Tensor, ids_in: torch.Tensor):
        """[W, M, k] gathered per-shard lists -> global (val[M,k], ids0[M,k])."""
        val_in = self._dev(val_in, torch.float32)
        ids_in = self._dev(ids_in, torch.int64)
        W, M, k = val_in.shape
        val = torch.empty((M, k), dtype=torch.float32, device=self.device)
        ids = torch.empty((M, k), dtype=torch.int64, device=self.device)
        self._call(self.lib.irs_merge_topk, _ptr(val_in), _ptr(ids_in), W, M, k, _ptr(val), _ptr(ids))
        return val, ids

    def pack_topk(self, val: torch.Tensor, ids0: torch.Tensor) -> torch.Tensor:
        """(val, ids0) lists -> the exchange step's 64-bit keys (include/irs_hip.h), same shape, int64 storage."""
        val = self._dev(val, torch.float32)
        ids0 = self._dev(ids0, torch.int64)
        keys = torch.empty(val.shape, dtype=torch.int64, device=self.device)
        self._call(self.lib.irs_pack_topk, _ptr(val), _ptr(ids0), val.numel(), _ptr(keys))
        return keys

    def merge_topk_keys(self, keys_in: torch.Tensor):
        """[W, M, k] packed per-shard lists -> global (val[M,k], ids0[M,k])."""
        keys_in = self._dev(keys_in, torch.int64)
        W, M, k = keys_in.shape
        val = torch.empty((M, k), dtype=torch.float32, device=self.device)
        ids = torch.empty((M, k), dtype=torch.int64, device=self.device)
        self._call(self.lib.irs_merge_topk_keys, _ptr(keys_in), W, M, k, _ptr(val), _ptr(ids))
        return val, ids

    # ------------------------------------------------------------------ evaluation batch (device-side loader)
    def build_eval_batch(self, items: torch.Tensor, offsets: torch.Tensor, *, raw_len: int = 100, gap_len: int = 0,
                         targets: Optional[torch.Tensor] = None, pool: Optional[torch.Tensor] = None, seed: int = 0):
        """get_random_evaluate_data + DataLoaderEvalIRS._collate_fn on the device (data_provider.py:398-449,
        591-617).  `items` int64 [total] / `offsets` int64 [B+1]: every user's events, oldest first.
        Returns (seq[B,L], targets[B], labels[B], raw[B,raw_len] right-aligned, raw_n[B] int32, status[B] int32)."""
        items = self._dev(items, torch.int64)
        offsets = self._dev(offsets, torch.int64)
        B = offsets.shape[0] - 1
        if targets is not None:
            targets = self._dev(targets, torch.int64)
        if pool is not None:
            pool = self._dev(pool, torch.int64)
        seq = torch.empty((B, self.L), dtype=torch.int64, device=self.device)
        tgt = torch.empty(B, dtype=torch.int64, device=self.device)
        lab = torch.empty(B, dtype=torch.int64, device=self.device)
        raw = torch.empty((B, raw_len), dtype=torch.int64, device=self.device)
        raw_n = torch.empty(B, dtype=torch.int32, device=self.device)
        status = torch.zeros(B, dtype=torch.int32, device=self.device)
        self._call(self.lib.irs_build_eval_batch, _ptr(items), _ptr(offsets), B, raw_len, gap_len, _ptr(targets),
                                                  _ptr(pool), 0 if pool is None else pool.shape[0], seed & (2 ** 64 - 1),
                                                  _ptr(seq), _ptr(tgt), _ptr(lab), _ptr(raw), _ptr(raw_n), _ptr(status))
        return seq, tgt, lab, raw, raw_n, status

    # ------------------------------------------------------------------ exact candidates (survivors.hip)
    def survivor_scratch_bytes(self, rows: int, want: int) -> int:
        n = int(self.lib.irs_survivor_scratch_bytes(self.h, rows, want))
        if n == 0:
            raise IrsError(f"survivor_scratch_bytes: rows={rows} / want={want} (want in [1, 32])")
        return n

    def ensure_survivors(self, xrows: torch.Tensor, seqs: torch.Tensor, hep: torch.Tensor, val: torch.Tensor, ids0: torch.Tensor,
                         status: torch.Tensor, want: int = 1, rows_per_status: int = 1, cum: Optional[torch.Tensor] = None,
                         fin: Optional[torch.Tensor] = None, done: Optional[torch.Tensor] = None,
                         scratch: Optional[torch.Tensor] = None):
        """irs_topk_ensure_survivors: rows whose k candidates leave fewer than `want` survivors outside the window
        seqs[m, :hep[m] + 1] get the exact best `want` admissible items of the whole catalog (val / ids0 rewritten in place,
        IRS_ROW_RESCUED in status[m // rows_per_status]); other rows are not written.  Returns (val, ids0, status)."""
        xrows = self._dev(xrows, torch.float32)
        seqs, hep = self._dev(seqs, torch.int64), self._dev(hep, torch.int32)
        val = self._inplace(val, torch.float32, "ensure_survivors: val")
        ids0 = self._inplace(ids0, torch.int64, "ensure_survivors: ids0")
        status = self._inplace(status, torch.int32, "ensure_survivors: status")
        M = xrows.shape[0]
        if (xrows.shape[1] != self.d or seqs.shape != (M, self.L) or hep.numel() != M or val.shape != ids0.shape or val.shape[0] != M
                or rows_per_status < 1 or M % rows_per_status or status.numel() != M // rows_per_status):
            raise IrsError("ensure_survivors: inconsistent shapes")
        cum = None if cum is None else self._dev(cum, torch.float64)
        fin = None if fin is None else self._dev(fin, torch.int32)
        done = None if done is None else self._dev(done, torch.int32)
        if (cum is not None and cum.numel() != M) or (fin is not None and fin.numel() != M) or (
                done is not None and done.numel() != M // rows_per_status):
            raise IrsError("ensure_survivors: cum / fin are per row, done per status word")
        if scratch is None:
            scratch = torch.empty(self.survivor_scratch_bytes(M, want), dtype=torch.uint8, device=self.device)
        self._call(self.lib.irs_topk_ensure_survivors, _ptr(xrows), _ptr(seqs), _ptr(hep), M, rows_per_status, val.shape[1], want,
                   _ptr(cum), _ptr(fin), _ptr(done), _ptr(val), _ptr(ids0), _ptr(status), _ptr(scratch),
                   scratch.numel() * scratch.element_size())
        return val, ids0, status

    # ------------------------------------------------------------------ bound exclusions (irs_bind_exclusions)
    def exclusion_scratch_bytes(self, users: int, n_excl: int) -> int:
        n = int(self.lib.irs_exclusion_scratch_bytes(self.h, users, n_excl))
        if n == 0:
            raise IrsError(f"exclusion_scratch_bytes: users={users} / n_excl={n_excl} (users >= 1, n_excl in [0, 4096])")
        return n

    def bind_exclusions(self, excl_ids0: Optional[torch.Tensor], users: Optional[int] = None, no_repeat: bool = False,
                        scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
        """irs_bind_exclusions: excl_ids0 int64 [users, n_excl], global 0-based ids, -1 = unused slot (None: no_repeat only, for
        `users` users).  Until unbind_exclusions every step and loop entry point drops window + list (+ the path so far under
        no_repeat).  Returns the scratch, which the caller keeps alive while bound."""
        if excl_ids0 is not None:
            excl_ids0 = self._dev(excl_ids0, torch.int64)
            if excl_ids0.dim() != 2 or (users is not None and users != excl_ids0.shape[0]):
                raise IrsError("bind_exclusions: excl_ids0 must be [users, n_excl]")
            users, n_excl = excl_ids0.shape
            if n_excl == 0:
                excl_ids0 = None
        else:
            n_excl = 0
        if users is None:
            raise IrsError("bind_exclusions: users is needed without a list")
        if scratch is None:
            scratch = torch.empty(self.exclusion_scratch_bytes(users, n_excl), dtype=torch.uint8, device=self.device)
        self._call(self.lib.irs_bind_exclusions, _ptr(excl_ids0), users, n_excl, int(bool(no_repeat)), _ptr(scratch),
                   scratch.numel() * scratch.element_size())
        if excl_ids0 is not None:  # (the prepare launch reads the list on the stream; the caller's tensor need not outlive the call)
            excl_ids0.record_stream(torch.cuda.current_stream(self.device))
        return scratch

    def unbind_exclusions(self):
        self._call(self.lib.irs_bind_exclusions, None, 0, 0, 0, None, 0)

    # ------------------------------------------------------------------ offer set (irs_bind_offer_set)
    def offer_set_scratch_bytes(self, n_ids: int, rows: int) -> int:
        n = int(self.lib.irs_offer_set_scratch_bytes(self.h, n_ids, rows))
        if n == 0:
            raise IrsError(f"offer_set_scratch_bytes: n_ids={n_ids} / rows={rows} (n_ids in [1, n_item={self.n_item}], rows in "
                           f"[1, max_rows={self.max_rows}])")
        return n

    def bind_offer_set(self, ids0: torch.Tensor, rows: Optional[int] = None, *, prepared: bool = False) -> torch.Tensor:
        """irs_bind_offer_set: ids0 int64, global 0-based ids in any order (sorted and made unique on the device here).  Until
        unbind_offer_set the search loops, recommend and the survivor pass offer items of the set only; score_topk_offer ranks
        inside it.  rows: the rows of one pass of the scratch (default max_rows).  The hole count is read once -- the call's one
        host wait -- and an id outside [0, n_item) raises.  prepared: bind the array as it is (what the C caller does).
        Returns the scratch, which the engine also keeps alive while bound.  The binding's launch goes on the null stream,
        ordered against torch's current stream by events (_call_null)."""
        ids0 = self._dev(ids0, torch.int64).reshape(-1)
        if not prepared:
            ids0 = torch.unique(ids0, sorted=True)
        n = ids0.numel()
        rows = self.max_rows if rows is None else rows
        scratch = torch.empty(self.offer_set_scratch_bytes(n, rows), dtype=torch.uint8, device=self.device)
        self._call_null(self.lib.irs_bind_offer_set, _ptr(ids0), n, _ptr(scratch), scratch.numel(), tensors=(ids0, scratch))
        self._offer_scratch = scratch
        holes = int(scratch[:4].view(torch.int32).item())
        if holes:
            self.unbind_offer_set()
            raise IrsError(f"bind_offer_set: {holes} of {n} ids are outside [0, n_item={self.n_item}), repeated or not ascending")
        return scratch

    def unbind_offer_set(self):
        with torch.cuda.device(self.device):  # (no launch: nothing to order)
            self._check(self.lib.irs_bind_offer_set(self.h, None, 0, None, 0))
        self._offer_scratch = None

    def score_topk_offer(self, xrows: torch.Tensor, k: int = 100):
        """irs_score_topk_offer: (val[M,k] float32, ids0[M,k] int64 global 0-based, status[M] int32), the best k of the bound set.
        The work goes on the null stream, ordered against torch's current stream by events (_call_null)."""
        xrows = self._dev(xrows, torch.float32)
        M = xrows.shape[0]
        val = torch.empty((M, k), dtype=torch.float32, device=self.device)
        ids = torch.empty((M, k), dtype=torch.int64, device=self.device)
        st = torch.empty(M, dtype=torch.int32, device=self.device)
        self._call_null(self.lib.irs_score_topk_offer, _ptr(xrows), M, k, _ptr(val), _ptr(ids), _ptr(st),
                        tensors=(xrows, val, ids, st, getattr(self, "_offer_scratch", None)))
        return val, ids, st

    # ------------------------------------------------------------------ recommend (irs_recommend, irs_recommend_take)
    def recommend_scratch_bytes(self, rows: int, n: int, k: int) -> int:
        nb = int(self.lib.irs_recommend_scratch_bytes(self.h, rows, n, k))
        if nb == 0:
            raise IrsError(f"recommend_scratch_bytes: rows={rows} / n={n} / k={k} (rows in [1, max_rows={self.max_rows}], k in "
                           f"[1, max_k={self.max_k}], n in [1, min(k, {_lib.IRS_MAX_RECOMMEND})])")
        return nb

    def _window(self, what: str, seqs, hep, M: int):
        if (seqs is None) != (hep is None):
            raise IrsError(f"{what}: seqs and hep go together")
        if seqs is None:
            return None, None
        seqs, hep = self._dev(seqs, torch.int64), self._dev(hep, torch.int32)
        if tuple(seqs.shape) != (M, self.L) or hep.numel() != M:
            raise IrsError(f"{what}: seqs [M, max_len] and hep [M] for M = {M} rows")
        return seqs, hep

    def recommend(self, xrows: torch.Tensor, n: int, *, seqs: Optional[torch.Tensor] = None, hep: Optional[torch.Tensor] = None,
                  k: int = 100, sweep: int = IRS_SWEEP_BF16, log_probs: bool = True):
        """irs_recommend: per row the best n items of the whole catalog that are neither in the window seqs[m, :hep[m] + 1] (None:
        no window) nor in the bound user's exclusion list (bind_exclusions), exact whatever the window hides of the top k.
        Returns (val[M, n] float32, ids0[M, n] int64 0-based, lp[M, n] float32 or None, count[M] int32, status[M] int32); entries
        behind count[m] are (-inf, -1, -inf).  The scratch is the engine's, kept for the next call of the same shape.  The work goes on
        the null stream, ordered against torch's current stream by events (_call_null)."""
        xrows = self._dev(xrows, torch.float32)
        if xrows.dim() != 2 or xrows.shape[1] != self.d:
            raise IrsError("recommend: xrows [M, d]")
        M = xrows.shape[0]
        seqs, hep = self._window("recommend", seqs, hep, M)
        need = self.recommend_scratch_bytes(M, n, k)
        held = getattr(self, "_recommend_scratch", None)
        if held is None or held[0] != (M, n, k):
            held = ((M, n, k), torch.empty(need, dtype=torch.uint8, device=self.device))
            self._recommend_scratch = held
        scratch = held[1]
        val = torch.empty((M, n), dtype=torch.float32, device=self.device)
        ids = torch.empty((M, n), dtype=torch.int64, device=self.device)
        lp = torch.empty((M, n), dtype=torch.float32, device=self.device) if log_probs else None
        count = torch.empty(M, dtype=torch.int32, device=self.device)
        st = torch.empty(M, dtype=torch.int32, device=self.device)
        self._call_null(self.lib.irs_recommend, _ptr(xrows), _ptr(seqs), _ptr(hep), M, n, k, sweep, _ptr(val), _ptr(ids), _ptr(lp),
                        _ptr(count), _ptr(st), _ptr(scratch), scratch.numel(),
                        tensors=(xrows, seqs, hep, val, ids, lp, count, st, scratch))
        return val, ids, lp, count, st

    def recommend_take(self, val: torch.Tensor, ids0: torch.Tensor, n: int, *, seqs: Optional[torch.Tensor] = None,
                       hep: Optional[torch.Tensor] = None, lse: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """irs_recommend_take, the kernel alone: the first n admissible entries of the caller's ranked lists val / ids0 [M, k] (a
        list ends at its first negative id).  lse: the rows' (max, sumexp) for the log-probabilities (None: no lp).  Returns
        (val[M, n], ids0[M, n], lp[M, n] or None, count[M])."""
        val, ids0 = self._dev(val, torch.float32), self._dev(ids0, torch.int64)
        if val.dim() != 2 or val.shape != ids0.shape:
            raise IrsError("recommend_take: val and ids0 [M, k]")
        M, k = val.shape
        seqs, hep = self._window("recommend_take", seqs, hep, M)
        mx = sm = None
        if lse is not None:
            mx, sm = self._dev(lse[0], torch.float32), self._dev(lse[1], torch.float32)
            if mx.numel() != M or sm.numel() != M:
                raise IrsError("recommend_take: lse is (max[M], sumexp[M])")
        # (allocated with the shape the caller asked for even where the library is going to refuse it: its message is the answer)
        o_val = torch.empty((M, max(n, 0)), dtype=torch.float32, device=self.device)
        o_ids = torch.empty((M, max(n, 0)), dtype=torch.int64, device=self.device)
        o_lp = torch.empty((M, max(n, 0)), dtype=torch.float32, device=self.device) if lse is not None else None
        count = torch.empty(M, dtype=torch.int32, device=self.device)
        self._call_null(self.lib.irs_recommend_take, _ptr(seqs), _ptr(hep), M, _ptr(val), _ptr(ids0), k, _ptr(mx), _ptr(sm), n,
                        _ptr(o_val), _ptr(o_ids), _ptr(o_lp), _ptr(count),
                        tensors=(seqs, hep, val, ids0, mx, sm, o_val, o_ids, o_lp, count))
        return o_val, o_ids, o_lp, count

    # ------------------------------------------------------------------ path trace (irs_bind_path_trace)
    def path_trace_scratch_bytes(self, rows: int) -> int:
        n = int(self.lib.irs_path_trace_scratch_bytes(self.h, rows))
        if n == 0:
            raise IrsError(f"path_trace_scratch_bytes: rows={rows} (need 1 <= rows <= max_rows={self.max_rows})")
        return n

    def score_target_trace(self, xrows: torch.Tensor, seqs: torch.Tensor, hep: torch.Tensor,
                           scratch: Optional[torch.Tensor] = None):
        """irs_score_target_trace: how each row's target seqs[m, L - 1] stands in the row's softmax, out of one pass over the
        float32 catalog: (max[M], sumexp[M], target_score[M] float32, rank[M] int32).  The rank leaves out the non-pad items of
        the window seqs[m, :hep[m] + 1]; log p(target) = target_score - (max + log(sumexp)).  A row without a target (0) gets
        target_score -inf and rank 0."""
        xrows = self._dev(xrows, torch.float32)
        seqs, hep = self._dev(seqs, torch.int64), self._dev(hep, torch.int32)
        M = xrows.shape[0]
        if xrows.dim() != 2 or xrows.shape[1] != self.d or tuple(seqs.shape) != (M, self.L) or hep.numel() != M:
            raise IrsError("score_target_trace: xrows [M, d], seqs [M, max_len], hep [M]")
        if scratch is None:
            scratch = torch.empty(self.path_trace_scratch_bytes(M), dtype=torch.uint8, device=self.device)
        scratch = self._inplace(scratch, torch.uint8, "score_target_trace: scratch")
        mx, sm, ts = (torch.empty(M, dtype=torch.float32, device=self.device) for _ in range(3))
        rank = torch.empty(M, dtype=torch.int32, device=self.device)
        self._call(self.lib.irs_score_target_trace, _ptr(xrows), _ptr(seqs), _ptr(hep), M, _ptr(scratch), scratch.numel(),
                   _ptr(mx), _ptr(sm), _ptr(ts), _ptr(rank))
        scratch.record_stream(torch.cuda.current_stream(self.device))
        return mx, sm, ts, rank

    def bind_path_trace(self, users: int, ld: int):
        """irs_bind_path_trace: until unbind_path_trace the greedy / sampled loops record (lp_item, lp_target float32 [users, ld],
        rank_target int32 [users, ld]); the beam and the sharded loops refuse.  Returns (lp_item, lp_target, rank_target,
        scratch): the caller keeps all four alive while bound."""
        lp_item = torch.zeros((users, ld), dtype=torch.float32, device=self.device)
        lp_target = torch.zeros((users, ld), dtype=torch.float32, device=self.device)
        rank = torch.zeros((users, ld), dtype=torch.int32, device=self.device)
        scratch = torch.empty(self.path_trace_scratch_bytes(users), dtype=torch.uint8, device=self.device)
        self._check(self.lib.irs_bind_path_trace(self.h, _ptr(lp_item), _ptr(lp_target), _ptr(rank), users, ld, _ptr(scratch),
                                                 scratch.numel()))
        return lp_item, lp_target, rank, scratch

    def unbind_path_trace(self):
        self._check(self.lib.irs_bind_path_trace(self.h, None, None, None, 0, 0, None, 0))

    # ------------------------------------------------------------------ admissible rank (irs_bind_trace_admissible)
    def admissible_scratch_bytes(self, rows: int) -> int:
        n = int(self.lib.irs_admissible_scratch_bytes(self.h, rows))
        if n == 0:
            raise IrsError(f"admissible_scratch_bytes: rows={rows} (need 1 <= rows <= max_rows={self.max_rows})")
        return n

    def score_target_rank_admissible(self, xrows: torch.Tensor, seqs: torch.Tensor, hep: torch.Tensor,
                                     paths: Optional[torch.Tensor] = None, step: int = 0):
        """irs_score_target_rank_admissible: score_target_trace's four results and rank_adm int32 [M], the target's rank among
        what the window, the bound exclusion list of user m (bind_exclusions), the non-zero entries paths[m, :step] (float32
        [M, path_ld], optional) and a bound offer set (bind_offer_set) leave: (max, sumexp, target_score, rank, rank_adm).  Where
        the target is admissible its 0-based position in recommend()'s slate on the same rows and bindings is rank_adm - 1.
        The work goes on the null stream, ordered against torch's current stream by events (_call_null)."""
        xrows = self._dev(xrows, torch.float32)
        seqs, hep = self._dev(seqs, torch.int64), self._dev(hep, torch.int32)
        M = xrows.shape[0]
        if xrows.dim() != 2 or xrows.shape[1] != self.d or tuple(seqs.shape) != (M, self.L) or hep.numel() != M:
            raise IrsError("score_target_rank_admissible: xrows [M, d], seqs [M, max_len], hep [M]")
        if paths is not None:
            paths = self._dev(paths, torch.float32)
            if paths.dim() != 2 or paths.shape[0] != M:
                raise IrsError("score_target_rank_admissible: paths [M, path_ld]")
        t_scratch = torch.empty(self.path_trace_scratch_bytes(M), dtype=torch.uint8, device=self.device)
        scratch = torch.empty(self.admissible_scratch_bytes(M), dtype=torch.uint8, device=self.device)
        mx, sm, ts = (torch.empty(M, dtype=torch.float32, device=self.device) for _ in range(3))
        rank, rank_adm = (torch.empty(M, dtype=torch.int32, device=self.device) for _ in range(2))
        self._call_null(self.lib.irs_score_target_rank_admissible, _ptr(xrows), _ptr(seqs), _ptr(hep), M, _ptr(paths),
                        paths.shape[1] if paths is not None else 0, int(step), _ptr(t_scratch), t_scratch.numel(), _ptr(scratch),
                        scratch.numel(), _ptr(mx), _ptr(sm), _ptr(ts), _ptr(rank), _ptr(rank_adm),
                        tensors=(xrows, seqs, hep, paths, t_scratch, scratch, mx, sm, ts, rank, rank_adm,
                                 getattr(self, "_offer_scratch", None)))
        return mx, sm, ts, rank, rank_adm

    def bind_trace_admissible(self, users: int, ld: int):
        """irs_bind_trace_admissible: adds rank_adm int32 [users, ld] to the BOUND path trace (the same users and ld) until
        unbind_trace_admissible or the trace's own unbind / rebind.  Returns (rank_adm, scratch): the caller keeps both alive."""
        rank_adm = torch.zeros((users, ld), dtype=torch.int32, device=self.device)
        scratch = torch.empty(self.admissible_scratch_bytes(users), dtype=torch.uint8, device=self.device)
        self._check(self.lib.irs_bind_trace_admissible(self.h, _ptr(rank_adm), users, ld, _ptr(scratch), scratch.numel()))
        return rank_adm, scratch

    def unbind_trace_admissible(self):
        self._check(self.lib.irs_bind_trace_admissible(self.h, None, 0, 0, None, 0))

    # ------------------------------------------------------------------ beam trace (irs_bind_beam_trace)
    def beam_trace_scratch_bytes(self, users: int, W: int) -> int:
        n = int(self.lib.irs_beam_trace_scratch_bytes(self.h, users, W))
        if n == 0:
            raise IrsError(f"beam_trace_scratch_bytes: users={users}, W={W} (need users >= 1, 1 <= W <= 32 and users * W <= "
                           f"min(max_seqs={self.max_seqs}, max_rows={self.max_rows}))")
        return n

    def bind_beam_trace(self, users: int, W: int, ld: int):
        """irs_bind_beam_trace (opt-in, off by default): until unbind_beam_trace the two beam loops of width W record, per output
        beam, (lp_item, lp_target float32 [users, W, ld], rank_target int32 [users, W, ld]) -- the path trace's values along the
        beam's ancestors, in the beam order of paths / scores; every other search entry point refuses.  Returns (lp_item,
        lp_target, rank_target, scratch): the caller keeps all four alive while bound."""
        lp_item = torch.zeros((users, W, ld), dtype=torch.float32, device=self.device)
        lp_target = torch.zeros((users, W, ld), dtype=torch.float32, device=self.device)
        rank = torch.zeros((users, W, ld), dtype=torch.int32, device=self.device)
        scratch = torch.empty(self.beam_trace_scratch_bytes(users, W), dtype=torch.uint8, device=self.device)
        self._check(self.lib.irs_bind_beam_trace(self.h, _ptr(lp_item), _ptr(lp_target), _ptr(rank), users, W, ld, _ptr(scratch),
                                                 scratch.numel()))
        return lp_item, lp_target, rank, scratch

    def unbind_beam_trace(self):
        self._check(self.lib.irs_bind_beam_trace(self.h, None, None, None, 0, 0, 0, None, 0))

    def beam_step_linked(self, state_in, val, ids0, lse, step: int, state_out, status, *, done=None,
                         stop_rule: int = _lib.IRS_BEAM_STOP_BEST):
        """irs_beam_step_linked: beam_step (four-tensor states, done None) or beam_step_until (five-tensor states with fin, and
        done[B]) that also returns (link int32 [B, W], link_val float32 [B, W]): per output beam IRS_BEAM_LINK_DEAD, its parent
        p, or IRS_BEAM_LINK_COPY | p, and the list value of the candidate a child chose.  A synchronous call (_call_sync)."""
        kinds = (torch.int64, torch.int32, torch.float64, torch.float32, torch.int32)
        if len(state_in) != len(state_out) or (len(state_in) == 5) != (done is not None) or len(state_in) not in (4, 5):
            raise IrsError("beam_step_linked: four-tensor states without done, or five-tensor states (fin last) with done")
        s_in = [self._inplace(t, k, "beam_step_linked: state_in") for t, k in zip(state_in, kinds)] + [None]
        s_out = [self._inplace(t, k, "beam_step_linked: state_out") for t, k in zip(state_out, kinds)] + [None]
        if done is not None:
            done = self._inplace(done, torch.int32, "beam_step_linked: done")
        status = self._inplace(status, torch.int32, "beam_step_linked: status")
        val, ids0 = self._dev(val, torch.float32), self._dev(ids0, torch.int64)
        B, W, _ = s_in[0].shape
        lmax, lsum = lse if lse is not None else (None, None)
        if lmax is not None:
            lmax, lsum = self._dev(lmax, torch.float32), self._dev(lsum, torch.float32)
        link = torch.empty((B, W), dtype=torch.int32, device=self.device)
        link_val = torch.empty((B, W), dtype=torch.float32, device=self.device)
        self._call_sync(self.lib.irs_beam_step_linked, _ptr(s_in[0]), _ptr(s_in[1]), _ptr(s_in[2]), _ptr(s_in[3]), _ptr(s_in[4]),
                   _ptr(val), _ptr(ids0), _ptr(lmax), _ptr(lsum), B, W, val.shape[1], step, s_in[3].shape[2], int(stop_rule),
                   _ptr(s_out[0]), _ptr(s_out[1]), _ptr(s_out[2]), _ptr(s_out[3]), _ptr(s_out[4]), _ptr(done), _ptr(status),
                   _ptr(link), _ptr(link_val))
        return link, link_val

    def beam_trace_carry(self, link, link_val, mx, sm, ts, rank, step: int, lp_item, lp_target, rank_target, row_map=None):
        """irs_beam_trace_carry: applies a linked step's (link, link_val [B, W]) to the three [users, W, ld] arrays in place;
        (mx, sm, ts, rank) are score_target_trace's results on the step's B * W INPUT rows; row_map int32 [B] (None: the
        identity) names the user row of the arrays.  A synchronous call (_call_sync)."""
        link, link_val = self._dev(link, torch.int32), self._dev(link_val, torch.float32)
        mx, sm, ts = (self._dev(t, torch.float32) for t in (mx, sm, ts))
        rank = self._dev(rank, torch.int32)
        lp_item = self._inplace(lp_item, torch.float32, "beam_trace_carry: lp_item")
        lp_target = self._inplace(lp_target, torch.float32, "beam_trace_carry: lp_target")
        rank_target = self._inplace(rank_target, torch.int32, "beam_trace_carry: rank_target")
        B, W = link.shape
        users, ld = lp_item.shape[0], lp_item.shape[2]
        if link_val.shape != (B, W) or any(t.numel() != B * W for t in (mx, sm, ts, rank)) or lp_item.dim() != 3 or \
                lp_item.shape != (users, W, ld) or lp_target.shape != lp_item.shape or rank_target.shape != lp_item.shape:
            raise IrsError("beam_trace_carry: link / link_val [B, W], sweep rows [B * W], the three arrays [users, W, ld]")
        if row_map is not None:
            row_map = self._dev(row_map, torch.int32)
            if row_map.numel() != B:
                raise IrsError("beam_trace_carry: row_map [B]")
        elif B > users:
            raise IrsError(f"beam_trace_carry: {B} users, the arrays hold {users}")
        self._call_sync(self.lib.irs_beam_trace_carry, _ptr(link), _ptr(link_val), _ptr(mx), _ptr(sm), _ptr(ts), _ptr(rank), B, W, step,
                   _ptr(lp_item), _ptr(lp_target), _ptr(rank_target), ld, _ptr(row_map))

    # ------------------------------------------------------------------ beam rule (irs_set_beam_rule)
    def set_beam_rule(self, rank_max: Optional[int] = None, lp_min: Optional[float] = None, target_weight: float = 0.0):
        """irs_set_beam_rule (opt-in, off by default): until cleared (None, None, 0) the two beam loops, which then need a bound
        beam trace (trace=True), offer the target alone to a beam whose target stands at rank <= rank_max among what its window
        leaves, or at log-probability >= lp_min (IRS_ROW_OFFERED in the user's status word), and order the candidates of a step
        by score + target_weight * lp_target(parent); the returned scores stay acceptance sums.  Every other search entry point
        refuses while a rule is set."""
        self._check(self.lib.irs_set_beam_rule(self.h, 0 if rank_max is None else int(rank_max),
                                               float("nan") if lp_min is None else float(lp_min), float(target_weight)))

    def beam_step_ruled(self, state_in, val, ids0, lse, step: int, state_out, status, mx, sm, ts, rank, *, done=None,
                        stop_rule: int = _lib.IRS_BEAM_STOP_BEST, rank_max: Optional[int] = None, lp_min: Optional[float] = None,
                        target_weight: float = 0.0):
        """irs_beam_step_ruled: beam_step_linked under a rule given as arguments; (mx, sm, ts, rank) are score_target_trace's
        results on the step's B * W INPUT rows.  Returns (link, link_val) as beam_step_linked does.  A synchronous call."""
        kinds = (torch.int64, torch.int32, torch.float64, torch.float32, torch.int32)
        if len(state_in) != len(state_out) or (len(state_in) == 5) != (done is not None) or len(state_in) not in (4, 5):
            raise IrsError("beam_step_ruled: four-tensor states without done, or five-tensor states (fin last) with done")
        s_in = [self._inplace(t, k, "beam_step_ruled: state_in") for t, k in zip(state_in, kinds)] + [None]
        s_out = [self._inplace(t, k, "beam_step_ruled: state_out") for t, k in zip(state_out, kinds)] + [None]
        if done is not None:
            done = self._inplace(done, torch.int32, "beam_step_ruled: done")
        status = self._inplace(status, torch.int32, "beam_step_ruled: status")
        val, ids0 = self._dev(val, torch.float32), self._dev(ids0, torch.int64)
        mx, sm, ts = (self._dev(t, torch.float32) for t in (mx, sm, ts))
        rank = self._dev(rank, torch.int32)
        B, W, _ = s_in[0].shape
        if any(t.numel() != B * W for t in (mx, sm, ts, rank)):
            raise IrsError("beam_step_ruled: the sweep's rows [B * W]")
        lmax, lsum = lse if lse is not None else (None, None)
        if lmax is not None:
            lmax, lsum = self._dev(lmax, torch.float32), self._dev(lsum, torch.float32)
        link = torch.empty((B, W), dtype=torch.int32, device=self.device)
        link_val = torch.empty((B, W), dtype=torch.float32, device=self.device)
        self._call_sync(self.lib.irs_beam_step_ruled, _ptr(s_in[0]), _ptr(s_in[1]), _ptr(s_in[2]), _ptr(s_in[3]), _ptr(s_in[4]),
                        _ptr(val), _ptr(ids0), _ptr(lmax), _ptr(lsum), B, W, val.shape[1], step, s_in[3].shape[2], int(stop_rule),
                        _ptr(s_out[0]), _ptr(s_out[1]), _ptr(s_out[2]), _ptr(s_out[3]), _ptr(s_out[4]), _ptr(done), _ptr(status),
                        _ptr(link), _ptr(link_val), _ptr(mx), _ptr(sm), _ptr(ts), _ptr(rank), 0 if rank_max is None else int(rank_max),
                        float("nan") if lp_min is None else float(lp_min), float(target_weight))
        return link, link_val

    # ------------------------------------------------------------------ path replay (irs_replay_windows / irs_replay_paths)
    def replay_scratch_bytes(self, chunk: int) -> int:
        n = int(self.lib.irs_replay_scratch_bytes(self.h, chunk))
        if n == 0:
            raise IrsError(f"replay_scratch_bytes: chunk={chunk} (need 1 <= chunk <= min(max_rows, max_seqs) = "
                           f"{min(self.max_rows, self.max_seqs)})")
        return n

    def _replay_inputs(self, what: str, layout: int, seq0, paths, row_user, row_step, hep0, users, P):
        seq0, paths = self._dev(seq0, torch.int64), self._dev(paths, torch.int64)
        row_user, row_step = self._dev(row_user, torch.int32), self._dev(row_step, torch.int32)
        if seq0.dim() != 2 or seq0.shape[1] != self.L or paths.dim() != 2 or paths.shape[0] != seq0.shape[0] or \
                row_user.dim() != 1 or row_user.shape != row_step.shape or row_user.numel() < 1:
            raise IrsError(f"{what}: seq0 [B, max_len], paths [B, path_ld], row_user / row_step [R >= 1]")
        B = seq0.shape[0]
        hep0 = None if hep0 is None else self._dev(hep0, torch.int32)
        users = None if users is None else self._dev(users, torch.int64)
        if (hep0 is not None and hep0.numel() != B) or (users is not None and users.numel() != B):
            raise IrsError(f"{what}: hep0 / users are per user [B]")
        if layout == _lib.IRS_REPLAY_SLOT and hep0 is None:
            raise IrsError(f"{what}: the slot layout needs hep0")
        P = paths.shape[1] if P is None else int(P)
        return seq0, paths, row_user, row_step, hep0, users, B, P

    def replay_windows(self, layout: int, seq0, paths, row_user, row_step, *, hep0=None, users=None, P: Optional[int] = None):
        """irs_replay_windows: the teacher-forced window of every row (row_user[r], row_step[r]) -- the user's start window
        seq0[b] with paths[b, :i] applied by the layout's step rule (IRS_REPLAY_SLOT: the search loops', hep0 given;
        IRS_REPLAY_FULL: the evaluator's post-padded windows).  paths int64 [B, path_ld], P = path_ld unless given.
        Returns (seq [R, max_len] int64, hep [R] int32, users [R] int64 or None, status [R] int32)."""
        seq0, paths, row_user, row_step, hep0, users, B, P = self._replay_inputs("replay_windows", layout, seq0, paths, row_user,
                                                                                 row_step, hep0, users, P)
        R = row_user.numel()
        seq = torch.empty((R, self.L), dtype=torch.int64, device=self.device)
        hep = torch.empty(R, dtype=torch.int32, device=self.device)
        usr = torch.empty(R, dtype=torch.int64, device=self.device) if users is not None else None
        status = torch.empty(R, dtype=torch.int32, device=self.device)
        self._call(self.lib.irs_replay_windows, layout, _ptr(seq0), _ptr(hep0), _ptr(users), B, _ptr(paths), P, paths.shape[1],
                   _ptr(row_user), _ptr(row_step), R, _ptr(seq), _ptr(hep), _ptr(usr), _ptr(status))
        return seq, hep, usr, status

    def replay_paths(self, layout: int, seq0, paths, row_user, row_step, *, hep0=None, users=None, targets=None,
                     P: Optional[int] = None, chunk: Optional[int] = None, scratch: Optional[torch.Tensor] = None):
        """irs_replay_paths: the path trace's three values for every row (row_user[r], row_step[r]) of saved paths, in passes of
        `chunk` rows (default min(max_rows, max_seqs)): windows, one rows-only decode, one sweep of the float32 catalog per pass.
        targets int64 [B]: the evaluator's layout (IRS_REPLAY_FULL); the slot layout reads them from seq0[:, -1].
        Returns (lp_item [R], lp_target [R] float32, rank_target [R] int32, status [R] int32); an invalid row reads 0 / 0 / 0 and
        IRS_ROW_NO_CANDIDATE."""
        seq0, paths, row_user, row_step, hep0, users, B, P = self._replay_inputs("replay_paths", layout, seq0, paths, row_user,
                                                                                 row_step, hep0, users, P)
        targets = None if targets is None else self._dev(targets, torch.int64)
        if targets is not None and targets.numel() != B:
            raise IrsError("replay_paths: targets are per user [B]")
        R = row_user.numel()
        chunk = min(self.max_rows, self.max_seqs) if chunk is None else int(chunk)
        if scratch is None:
            scratch = torch.empty(self.replay_scratch_bytes(chunk), dtype=torch.uint8, device=self.device)
        scratch = self._inplace(scratch, torch.uint8, "replay_paths: scratch")
        lp_item, lp_target = (torch.empty(R, dtype=torch.float32, device=self.device) for _ in range(2))
        rank = torch.empty(R, dtype=torch.int32, device=self.device)
        status = torch.empty(R, dtype=torch.int32, device=self.device)
        self._call(self.lib.irs_replay_paths, layout, _ptr(seq0), _ptr(hep0), _ptr(users), _ptr(targets), B, _ptr(paths), P,
                   paths.shape[1], _ptr(row_user), _ptr(row_step), R, chunk, _ptr(scratch), scratch.numel(), _ptr(lp_item),
                   _ptr(lp_target), _ptr(rank), _ptr(status))
        for t in (scratch, seq0, paths, row_user, row_step, hep0, users, targets):  # (the passes only enqueue)
            if t is not None:
                t.record_stream(torch.cuda.current_stream(self.device))
        return lp_item, lp_target, rank, status

    # ------------------------------------------------------------------ bound guide (irs_bind_guide)
    def guide_scratch_bytes(self, kind: int, F: int) -> int:
        """irs_guide_scratch_bytes: the packed table of a binary guide; 0 for a float guide, which is read where it lies."""
        if kind == _lib.IRS_GUIDE_FLOAT and 1 <= F <= _lib.IRS_MAX_GUIDE_FLOATS:
            return 0
        n = int(self.lib.irs_guide_scratch_bytes(self.h, kind, F))
        if n == 0:
            raise IrsError(f"guide_scratch_bytes: kind={kind} / F={F} (binary: F in [1, {_lib.IRS_MAX_GUIDE_BITS}], float: F in "
                           f"[1, {_lib.IRS_MAX_GUIDE_FLOATS}])")
        return n

    def bind_guide(self, table: torch.Tensor, k_c: int = 5):
        """irs_bind_guide: table [n_item + 1, F], row i = the features of the 1-based item i (row 0 is never read).  bool / uint8 /
        any integer dtype: a binary guide (nonzero = 1, Hamming distance); floating: a float guide (converted to contiguous
        float32, squared Euclidean distance).  Until unbind_guide the greedy step and loops choose, among the first k_c
        admissible candidates, the one nearest to the target; the beam and the sharded loops refuse.  The engine holds the
        table and the scratch until unbound."""
        if not torch.is_tensor(table) or table.dim() != 2 or table.shape[0] != self.n_item + 1 or table.shape[1] < 1:
            raise IrsError(f"bind_guide: table must be [n_item + 1 = {self.n_item + 1}, F >= 1], got "
                           f"{tuple(table.shape) if torch.is_tensor(table) else type(table)}")
        if table.device != self.device:
            raise IrsError(f"bind_guide: table on {table.device}, engine on {self.device}")
        F = table.shape[1]
        if table.dtype.is_floating_point:
            kind, held, scratch = _lib.IRS_GUIDE_FLOAT, table.to(torch.float32).contiguous(), None
        elif table.dtype.is_complex:
            raise IrsError("bind_guide: a complex table has no distance here")
        else:
            kind, held = _lib.IRS_GUIDE_BINARY, table.ne(0).to(torch.uint8).contiguous()
            if F > _lib.IRS_MAX_GUIDE_BITS:
                raise IrsError(f"bind_guide: F={F} > {_lib.IRS_MAX_GUIDE_BITS} binary features")
            scratch = torch.empty(self.guide_scratch_bytes(kind, F), dtype=torch.uint8, device=self.device)
        self._call(self.lib.irs_bind_guide, kind, _ptr(held), F, k_c, _ptr(scratch), scratch.numel() if scratch is not None else 0)
        self._guide_held = (held, scratch)
        return held, scratch

    def unbind_guide(self):
        self._call(self.lib.irs_bind_guide, 0, None, 0, 0, None, 0)
        self._guide_held = None

    # ------------------------------------------------------------------ bound lookahead (irs_bind_lookahead)
    def lookahead_scratch_bytes(self, rows: int, k_c: int) -> int:
        n = int(self.lib.irs_lookahead_scratch_bytes(self.h, rows, k_c))
        if n == 0:
            raise IrsError(f"lookahead_scratch_bytes: rows={rows} / k_c={k_c} (rows >= 1, k_c in [1, {_lib.IRS_MAX_LOOKAHEAD_KC}])")
        return n

    def bind_lookahead(self, k_c: int, users: int, ld: int, record: bool = False):
        """irs_bind_lookahead: until unbind_lookahead a greedy step of generate_paths / generate_paths_until takes, among its
        first k_c admissible candidates, the one under which the target's log-probability at the NEXT step is highest (one
        decode of users * k_c child windows and one float32 catalog pass per step); the beam and the sharded loops refuse.
        record: the loops also write every live row's candidates and values, (items int32 [users, ld, k_c], 1-based, 0 = none;
        lp float32 [users, ld, k_c]).  Returns (items, lp) or None; the engine holds scratch and record until unbound."""
        k_c, users, ld = int(k_c), int(users), int(ld)
        # (an invalid k_c gets the library's message: the scratch is then only a placeholder)
        ok = 1 <= k_c <= _lib.IRS_MAX_LOOKAHEAD_KC and users >= 1
        nbytes = self.lookahead_scratch_bytes(users, k_c) if ok else 256
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        rec = None
        if record and ok and ld >= 1:
            rec = (torch.zeros((users, ld, k_c), dtype=torch.int32, device=self.device),
                   torch.zeros((users, ld, k_c), dtype=torch.float32, device=self.device))
        self._check(self.lib.irs_bind_lookahead(self.h, k_c, _ptr(scratch), scratch.numel(), _ptr(rec[0]) if rec else None,
                                                _ptr(rec[1]) if rec else None, users, ld))
        self._lookahead_held = (scratch, rec)
        return rec

    def unbind_lookahead(self):
        self._check(self.lib.irs_bind_lookahead(self.h, 0, None, 0, None, None, 0, 0))
        self._lookahead_held = None

    def lookahead_expand(self, seqs, hep, users, val, ids0, k_c: int, *, fin=None, paths=None, step: int = 0, row_map=None):
        """irs_lookahead_expand: the kernel alone, synchronously (the current stream is drained first).  Returns (child_seq [M * k_c, L] int64, child_hep [M * k_c] int32, child_user
        [M * k_c] int64, child_target0 [M * k_c] int64, cand_ids0 [M, k_c] int64, cand_val [M, k_c] float32)."""
        seqs, hep = self._dev(seqs, torch.int64), self._dev(hep, torch.int32)
        users = None if users is None else self._dev(users, torch.int64)
        val, ids0 = self._dev(val, torch.float32), self._dev(ids0, torch.int64)
        M = seqs.shape[0]
        if seqs.dim() != 2 or seqs.shape[1] != self.L or val.dim() != 2 or val.shape != ids0.shape or val.shape[0] != M or \
                hep.numel() != M or (users is not None and users.numel() != M):
            raise IrsError("lookahead_expand: seqs [M, max_len], val / ids0 [M, k], hep / users [M]")
        fin = None if fin is None else self._dev(fin, torch.int32)
        paths = None if paths is None else self._dev(paths, torch.float32)
        row_map = None if row_map is None else self._dev(row_map, torch.int32)
        if (fin is not None and fin.numel() != M) or (row_map is not None and row_map.numel() != M) or \
                (paths is not None and paths.dim() != 2):
            raise IrsError("lookahead_expand: fin / row_map [M], paths [rows, path_ld]")
        k_c = int(k_c)
        n = M * max(k_c, 1)
        c_seq = torch.empty((n, self.L), dtype=torch.int64, device=self.device)
        c_hep = torch.empty(n, dtype=torch.int32, device=self.device)
        c_user = torch.empty(n, dtype=torch.int64, device=self.device)
        c_tgt = torch.empty(n, dtype=torch.int64, device=self.device)
        c_ids = torch.empty((M, max(k_c, 1)), dtype=torch.int64, device=self.device)
        c_val = torch.empty((M, max(k_c, 1)), dtype=torch.float32, device=self.device)
        self._call_sync(self.lib.irs_lookahead_expand, _ptr(seqs), _ptr(hep), _ptr(users), M, _ptr(val), _ptr(ids0), val.shape[1], k_c,
                   _ptr(fin), _ptr(paths), paths.shape[1] if paths is not None else 0, step, _ptr(row_map), _ptr(c_seq), _ptr(c_hep),
                   _ptr(c_user), _ptr(c_tgt), _ptr(c_ids), _ptr(c_val))
        return c_seq, c_hep, c_user, c_tgt, c_ids, c_val

    def lookahead_choose(self, seqs, cand_ids0, cand_val, mx, sm, ts, val, ids0, *, fin=None):
        """irs_lookahead_choose: the kernel alone and synchronous like lookahead_expand, on expand's candidates and the children's (max, sumexp, target score), each
        [M, k_c] (or flat [M * k_c]); val / ids0 are rewritten in place.  Returns (lp [M, k_c] float32, choice [M] int32)."""
        seqs = self._dev(seqs, torch.int64)
        cand_ids0, cand_val = self._dev(cand_ids0, torch.int64), self._dev(cand_val, torch.float32)
        mx, sm, ts = (self._dev(t, torch.float32) for t in (mx, sm, ts))
        val = self._inplace(val, torch.float32, "lookahead_choose: val")
        ids0 = self._inplace(ids0, torch.int64, "lookahead_choose: ids0")
        M = seqs.shape[0]
        if seqs.dim() != 2 or seqs.shape[1] != self.L or cand_ids0.dim() != 2 or cand_ids0.shape[0] != M or \
                cand_val.shape != cand_ids0.shape or val.dim() != 2 or val.shape != ids0.shape or val.shape[0] != M or \
                any(t.numel() != cand_ids0.numel() for t in (mx, sm, ts)):
            raise IrsError("lookahead_choose: seqs [M, max_len], cand_ids0 / cand_val / mx / sm / ts [M, k_c], val / ids0 [M, k]")
        fin = None if fin is None else self._dev(fin, torch.int32)
        if fin is not None and fin.numel() != M:
            raise IrsError("lookahead_choose: fin [M]")
        k_c = cand_ids0.shape[1]
        lp = torch.empty((M, k_c), dtype=torch.float32, device=self.device)
        choice = torch.empty(M, dtype=torch.int32, device=self.device)
        self._call_sync(self.lib.irs_lookahead_choose, _ptr(seqs), M, k_c, _ptr(cand_ids0), _ptr(cand_val), _ptr(mx), _ptr(sm), _ptr(ts),
                   _ptr(fin), _ptr(val), _ptr(ids0), val.shape[1], _ptr(lp), _ptr(choice))
        return lp, choice

    # ------------------------------------------------------------------ bound sampler (irs_bind_sampler)
    def bind_sampler(self, top_k: int, temperature: float = 1.0, top_p: float = 1.0, users: int = 0, ld: int = 0, record: bool = False):
        """irs_bind_sampler: until unbind_sampler a step of generate_paths / generate_paths_until (called with sample=False) draws
        among its first top_k admissible candidates: weights exp((v - v_0) / temperature), the nucleus top_p, a draw keyed by
        (seed, the caller's row, the step); the beam and the sharded loops, a guide and a lookahead refuse.  record: the loops also
        write (u float32, lq float32, support int32), each [users, ld]: the draw, the chosen candidate's log-probability under
        the distribution it was drawn from, and the candidates the nucleus kept.  Returns the record or None; the engine holds it
        until unbound."""
        rec = None
        if record:
            if users < 1 or ld < 1:
                raise IrsError(f"bind_sampler: record=True needs users >= 1 and ld >= 1 (users={users}, ld={ld})")
            rec = (torch.zeros((users, ld), dtype=torch.float32, device=self.device),
                   torch.zeros((users, ld), dtype=torch.float32, device=self.device),
                   torch.zeros((users, ld), dtype=torch.int32, device=self.device))
        self._check(self.lib.irs_bind_sampler(self.h, int(top_k), float(temperature), float(top_p), _ptr(rec[0]) if rec else None,
                                              _ptr(rec[1]) if rec else None, _ptr(rec[2]) if rec else None, int(users), int(ld)))
        self._sampler_held = rec
        return rec

    def unbind_sampler(self):
        self._check(self.lib.irs_bind_sampler(self.h, 0, 1.0, 1.0, None, None, None, 0, 0))
        self._sampler_held = None

    def sampler_choose(self, seqs, hep, val, ids0, step: int, seed: int, status, *, row_ids=None, fin=None, paths=None):
        """irs_sampler_choose: the bound sampler's kernel alone on the caller's lists, synchronously (the current stream is drained
        first); val / ids0 are rewritten in place, the bound
        record (if any) is written at row row_ids[r] (None: r) and column step.  status is read only."""
        seqs, hep = self._dev(seqs, torch.int64), self._dev(hep, torch.int32)
        val = self._inplace(val, torch.float32, "sampler_choose: val")
        ids0 = self._inplace(ids0, torch.int64, "sampler_choose: ids0")
        status = self._dev(status, torch.int32)
        M = seqs.shape[0]
        if seqs.dim() != 2 or seqs.shape[1] != self.L or val.dim() != 2 or val.shape != ids0.shape or val.shape[0] != M or \
                hep.numel() != M or status.numel() != M:
            raise IrsError("sampler_choose: seqs [M, max_len], val / ids0 [M, k], hep / status [M]")
        row_ids = None if row_ids is None else self._dev(row_ids, torch.int32)
        fin = None if fin is None else self._dev(fin, torch.int32)
        paths = None if paths is None else self._dev(paths, torch.float32)
        if (fin is not None and fin.numel() != M) or (row_ids is not None and row_ids.numel() != M) or \
                (paths is not None and paths.dim() != 2):
            raise IrsError("sampler_choose: fin / row_ids [M], paths [rows, path_ld]")
        self._call_sync(self.lib.irs_sampler_choose, _ptr(seqs), _ptr(hep), M, _ptr(val), _ptr(ids0), val.shape[1], int(step), int(seed),
                   _ptr(row_ids), _ptr(status), _ptr(fin), _ptr(paths), paths.shape[1] if paths is not None else 0)

    # ------------------------------------------------------------------ arrival rule (irs_set_arrival_rule)
    def set_arrival_rule(self, rank_max: Optional[int] = None, lp_min: Optional[float] = None, among: str = "window"):
        """irs_set_arrival_rule[_ex]: until cleared (both None) a live row of the greedy / sampled loops whose target stands at rank
        <= rank_max among what the window leaves, or at log-probability >= lp_min, is offered the target alone
        (IRS_ROW_OFFERED).  The loops then need a bound path trace (trace=True).  among="admissible": the rank clause reads the
        admissible rank (IRS_RANK_ADMISSIBLE), and the loops need bind_trace_admissible as well (rank_admissible=True)."""
        kind = arrive_among_kind(among)
        rank_max, lp_min = 0 if rank_max is None else int(rank_max), float("nan") if lp_min is None else float(lp_min)
        if kind == _lib.IRS_RANK_WINDOW:
            self._check(self.lib.irs_set_arrival_rule(self.h, rank_max, lp_min))
        else:
            self._check(self.lib.irs_set_arrival_rule_ex(self.h, rank_max, lp_min, kind))

    def arrival_offer(self, seqs, hep, mx, sm, ts, rank, val, ids0, status, *, rank_max: Optional[int] = None,
                      lp_min: Optional[float] = None, fin=None, paths=None, step: int = 0, row_map=None):
        """irs_arrival_offer: the rule alone on the outputs of score_target_trace; val / ids0 / status are rewritten in place."""
        seqs, hep = self._dev(seqs, torch.int64), self._dev(hep, torch.int32)
        mx, sm, ts = (self._dev(t, torch.float32) for t in (mx, sm, ts))
        rank = self._dev(rank, torch.int32)
        val = self._inplace(val, torch.float32, "arrival_offer: val")
        ids0 = self._inplace(ids0, torch.int64, "arrival_offer: ids0")
        status = self._inplace(status, torch.int32, "arrival_offer: status")
        M = seqs.shape[0]
        if seqs.dim() != 2 or seqs.shape[1] != self.L or val.dim() != 2 or val.shape != ids0.shape or val.shape[0] != M or \
                any(t.numel() != M for t in (hep, mx, sm, ts, rank, status)):
            raise IrsError("arrival_offer: seqs [M, max_len], val / ids0 [M, k], the rest [M]")
        fin = None if fin is None else self._dev(fin, torch.int32)
        paths = None if paths is None else self._dev(paths, torch.float32)
        row_map = None if row_map is None else self._dev(row_map, torch.int32)
        if (fin is not None and fin.numel() != M) or (row_map is not None and row_map.numel() != M) or \
                (paths is not None and paths.dim() != 2):
            raise IrsError("arrival_offer: fin / row_map [M], paths [rows, path_ld]")
        self._call(self.lib.irs_arrival_offer, _ptr(seqs), _ptr(hep), M, _ptr(mx), _ptr(sm), _ptr(ts), _ptr(rank), _ptr(fin),
                   _ptr(val), _ptr(ids0), val.shape[1], 0 if rank_max is None else int(rank_max),
                   float("nan") if lp_min is None else float(lp_min), _ptr(paths), paths.shape[1] if paths is not None else 0,
                   step, _ptr(row_map), _ptr(status))

    # ------------------------------------------------------------------ the per-call keywords of the search methods
    @contextlib.contextmanager
    def _search_options(self, users: int, ld: int, beam: int = 0, sample=False, sample_k=3, graph: bool = False, *,
                        exact_candidates: bool = False, exclude: Optional[torch.Tensor] = None, no_repeat: bool = False, trace: bool = False,
                        guide: Optional[torch.Tensor] = None, guide_k: int = 5, arrive_rank: Optional[int] = None,
                        arrive_lp: Optional[float] = None, lookahead: Optional[int] = None, lookahead_record: bool = False,
                        beam_trace: bool = False, offer: Optional[torch.Tensor] = None, target_weight: float = 0.0,
                        rank_admissible: bool = False, arrive_among: str = "window", sampler: Optional[Sampler] = None):
        """While a search call runs with per-call keywords: what they ask for is bound before and unbound after.  Yields (the
        trace arrays (lp_item, lp_target, rank_target) or None, the lookahead record (items, lp) or None); beam_trace (the beam
        loops' trace=True) binds a beam trace for the call's width instead, whose [users, W, ld] arrays take the first place.
        offer (int64, 0-based ids, any order): an offer set is bound for the call (bind_offer_set), its scratch sized for the
        call's rows.  In a beam call (beam >= 1) arrive_rank / arrive_lp / target_weight set the BEAM rule (set_beam_rule).
        rank_admissible (with trace): an admissible rank is bound behind the trace (bind_trace_admissible) and the trace arrays
        grow a fourth, rank_adm; arrive_among="admissible" makes the arrival rule read it (ValueError without rank_admissible).
        users / ld: the call's users and path length; beam: its beam width, 0 for the greedy loops.  graph: the call replays
        a captured step -- the stream is drained once before the first unbind destroys it.
        sampler: a sampler is bound for the call (bind_sampler); its record (u, lq, support), or None, is the third member yielded.
        Every bind and unbind drops ALL captured steps of the context, so with a keyword set use_graph saves nothing: the step
        is captured again on every call, and steps captured by earlier calls are lost.  A caller that wants a captured step
        with an option inside binds it once itself (bind_* / set_arrival_rule) and calls without the keyword."""
        out = {}
        check_rank_options(trace, rank_admissible, arrive_among)

        def survivors():  # (for the call's rows and the candidates a step chooses among: csrc/irs_internal.h, irs_opt_choices)
            want = beam or (guide_k if guide is not None else (lookahead if lookahead is not None else (
                sampler.top_k if sampler is not None else (sample_k if sample else 1))))
            scratch = torch.empty(self.survivor_scratch_bytes(users * max(beam, 1), want), dtype=torch.uint8, device=self.device)
            self._check(self.lib.irs_bind_survivor_scratch(self.h, _ptr(scratch), scratch.numel()))
            return (scratch,)

        def exclusions():
            if exclude is not None and exclude.shape[0] != users:
                raise IrsError(f"exclude: {exclude.shape[0]} lists for {users} users")
            return (self.bind_exclusions(exclude, users, no_repeat),)

        def look():
            out["looked"] = self.bind_lookahead(lookahead, users, ld, lookahead_record)
            return self._lookahead_held[:1]

        def sampled():
            out["drawn"] = self.bind_sampler(sampler.top_k, sampler.temperature, sampler.top_p, users, ld, sampler.record)
            return out["drawn"] or ()

        def traced():
            lp_item, lp_target, rank, scratch = self.bind_path_trace(users, ld)
            out["traced"] = (lp_item, lp_target, rank)
            return (scratch,)

        def admissible():  # (behind the trace it belongs to; the trace's unbind, which runs later, would drop it as well)
            rank_adm, scratch = self.bind_trace_admissible(users, ld)
            out["traced"] = out["traced"] + (rank_adm,)
            return (scratch,)

        def beam_traced():
            lp_item, lp_target, rank, scratch = self.bind_beam_trace(users, beam, ld)
            out["traced"] = (lp_item, lp_target, rank)
            return (scratch,)

        # (asked for, bind -> the tensors it holds for the call, unbind), in bind order: irs_bind_lookahead refuses behind a
        # bound guide ("one choice rule at a time"), and a caller who asks for both gets that message
        arrive = arrive_rank is not None or arrive_lp is not None
        options = (
            (arrive and not beam, lambda: self.set_arrival_rule(arrive_rank, arrive_lp, arrive_among) or (),
             lambda: self.set_arrival_rule(None, None)),
            (bool(beam) and (arrive or target_weight != 0), lambda: self.set_beam_rule(arrive_rank, arrive_lp, target_weight) or (),
             lambda: self.set_beam_rule(None, None, 0.0)),
            (exact_candidates, survivors, lambda: self._check(self.lib.irs_bind_survivor_scratch(self.h, None, 0))),
            (exclude is not None or no_repeat, exclusions, self.unbind_exclusions),
            (guide is not None, lambda: self.bind_guide(guide, guide_k), self.unbind_guide),
            (lookahead is not None, look, self.unbind_lookahead),
            (sampler is not None, sampled, self.unbind_sampler),
            (trace, traced, self.unbind_path_trace),
            (trace and rank_admissible, admissible, self.unbind_trace_admissible),
            (beam_trace, beam_traced, self.unbind_beam_trace),
            (offer is not None, lambda: (self.bind_offer_set(offer, users * max(beam, 1)),), self.unbind_offer_set),
        )
        bound = []
        try:
            for asked, bind, unbind in options:
                if asked:
                    bound.append((bind(), unbind))
            yield out.get("traced"), out.get("looked"), out.get("drawn")
        finally:
            stream = torch.cuda.current_stream(self.device)
            if graph and bound:
                stream.synchronize()
            for held, unbind in reversed(bound):
                for t in held:  # (the loops only enqueue: scratch and table must outlive the work on the stream)
                    if t is not None:
                        t.record_stream(stream)
                unbind()

    def _greedy_call(self, what: str, seqs, users, hep, max_path_len: int, paths, status):
        """What generate_paths and generate_paths_until check and allocate alike: (seqs, users, hep, B, paths, status)."""
        seqs = self._inplace(seqs, torch.int64, f"{what}: seqs")
        hep = self._inplace(hep, torch.int32, f"{what}: hep")
        if users is not None:
            users = self._dev(users, torch.int64)
        B = seqs.shape[0]
        if seqs.shape[1] != self.L or hep.shape[0] != B or (users is not None and users.shape[0] != B):
            raise IrsError(f"{what}: inconsistent shapes")
        if paths is None:
            paths = torch.zeros((B, max_path_len), dtype=torch.float32, device=self.device)
        if status is None:
            status = torch.zeros(B, dtype=torch.int32, device=self.device)
        paths = self._inplace(paths, torch.float32, f"{what}: paths")
        status = self._inplace(status, torch.int32, f"{what}: status")
        if paths.shape != (B, max_path_len):
            raise IrsError(f"{what}: paths must be [B, max_path_len]")
        return seqs, users, hep, B, paths, status

    @staticmethod
    def _recorded(recorded, trace: bool, lookahead_record: bool):
        """The members a greedy loop's return value grows: the trace arrays, then the lookahead record, then the sampler's."""
        traced, looked, drawn = recorded
        return ((traced,) if trace else ()) + ((looked,) if lookahead_record else ()) + ((drawn,) if drawn is not None else ())

    # ------------------------------------------------------------------ path search
    def path_step(self, seqs, hep, val, ids0, step: int, paths, status, sample=False, sample_k=3, seed=0):
        seqs = self._inplace(seqs, torch.int64, "path_step: seqs")
        hep = self._inplace(hep, torch.int32, "path_step: hep")
        paths = self._inplace(paths, torch.float32, "path_step: paths")
        status = self._inplace(status, torch.int32, "path_step: status")
        val, ids0 = self._dev(val, torch.float32), self._dev(ids0, torch.int64)
        B = seqs.shape[0]
        if seqs.shape[1] != self.L or hep.shape[0] != B or val.shape != ids0.shape or val.shape[0] != B:
            raise IrsError("path_step: inconsistent shapes")
        self._call(self.lib.irs_path_step, _ptr(seqs), _ptr(hep), B, _ptr(val), _ptr(ids0), val.shape[1], step,
                                           _ptr(paths), paths.shape[1], int(sample), sample_k, seed, _ptr(status))

    def generate_paths(self, seqs: torch.Tensor, users: Optional[torch.Tensor], hep: torch.Tensor, max_path_len: int,
                       k: int = 100, sweep: int = IRS_SWEEP_BF16, sample=False, sample_k=3, seed=0,
                       use_graph: bool = False, paths: Optional[torch.Tensor] = None,
                       status: Optional[torch.Tensor] = None, exact_candidates: bool = False,
                       exclude: Optional[torch.Tensor] = None, no_repeat: bool = False, trace: bool = False,
                       guide: Optional[torch.Tensor] = None, guide_k: int = 5, arrive_rank: Optional[int] = None,
                       arrive_lp: Optional[float] = None, lookahead: Optional[int] = None, lookahead_record: bool = False,
                       offer: Optional[torch.Tensor] = None, rank_admissible: bool = False, arrive_among: str = "window",
                       sampler: Optional[Sampler] = None):
        """Runs the whole search loop on the device.  `seqs` and `hep` are the
        working window state and are modified in place.  exact_candidates: a row whose k candidates are hidden by its window
        chooses among the exact best admissible items of the catalog instead (IRS_ROW_RESCUED; the result of k = n_item).
        With a per-call keyword set use_graph saves nothing: the step is captured again on every call (_search_options).
        exclude (int64 [B, E], 0-based ids, -1 = unused) / no_repeat: bound for this call (irs_bind_exclusions): a step drops
        window + the user's list (+ its own path so far); the same holds in the three other loops.
        trace: a path trace is bound for this call (irs_bind_path_trace) and the return value grows a third member, (lp_item,
        lp_target float32 [B, max_path_len], rank_target int32 [B, max_path_len]): all columns are written; cut them where paths
        is cut.
        guide ([n_item + 1, F], see bind_guide) / guide_k: a guide is bound for this call (irs_bind_guide): a step takes, among
        its first guide_k admissible candidates, the one nearest to the target seqs[b, L - 1] (the Rec2Inf rule); greedy only.
        arrive_rank / arrive_lp: an arrival rule is set for this call (irs_set_arrival_rule; needs trace=True): a row whose
        target stands at rank <= arrive_rank among what its window leaves, or at log-probability >= arrive_lp, is offered the
        target at that step (IRS_ROW_OFFERED in its status word); this loop then searches on behind the arrival.
        lookahead (k_c in [1, 32]): a lookahead is bound for this call (irs_bind_lookahead): a step takes, among its first k_c
        admissible candidates, the one under which the target's next-step log-probability is highest; greedy only, not with
        guide.  lookahead_record: the return value grows a last member, (items int32 [B, max_path_len, k_c], lp float32 [B,
        max_path_len, k_c]): every step's candidates (1-based, 0 = none) and the values compared.
        offer (int64, 0-based ids): an offer set is bound for this call (irs_bind_offer_set): every step offers items of the set
        only; log-probabilities and target ranks stay statements about the whole catalog.  The same holds in the three other
        loops.
        rank_admissible (needs trace=True): the trace member grows a fourth array, rank_adm int32 [B, max_path_len]: the target's
        rank among what the window, exclude, no_repeat and offer leave (irs_bind_trace_admissible).  arrive_among="admissible"
        (needs rank_admissible=True): arrive_rank reads rank_adm instead of rank_target.  The same holds in
        generate_paths_until.
        sampler (Sampler(top_k, temperature, top_p, record)): a sampler is bound for this call (irs_bind_sampler); `seed` keys its
        draws and sample must be False; not with guide or lookahead.  record: the return value grows a last member, (u, lq
        float32 [B, max_path_len], support int32 [B, max_path_len])."""
        seqs, users, hep, B, paths, status = self._greedy_call("generate_paths", seqs, users, hep, max_path_len, paths, status)
        with self._search_options(B, max_path_len, 0, sample, sample_k, bool(use_graph), exact_candidates=exact_candidates, exclude=exclude,
                                  no_repeat=no_repeat, trace=trace, guide=guide, guide_k=guide_k, arrive_rank=arrive_rank,
                                  arrive_lp=arrive_lp, lookahead=lookahead, lookahead_record=lookahead_record, offer=offer,
                                  rank_admissible=rank_admissible, arrive_among=arrive_among, sampler=sampler) as recorded:
            self._call(self.lib.irs_generate_paths, _ptr(seqs), _ptr(users), _ptr(hep), B, max_path_len, k, sweep,
                                                    int(sample), sample_k, seed, int(use_graph), _ptr(paths), _ptr(status))
        return (paths, status) + self._recorded(recorded, trace, lookahead is not None and lookahead_record)

    def generate_paths_until(self, seqs: torch.Tensor, users: Optional[torch.Tensor], hep: torch.Tensor, max_path_len: int,
                             k: int = 100, sweep: int = IRS_SWEEP_BF16, sample=False, sample_k=3, seed=0,
                             check_every: int = 1, paths: Optional[torch.Tensor] = None,
                             status: Optional[torch.Tensor] = None, exact_candidates: bool = False,
                             exclude: Optional[torch.Tensor] = None, no_repeat: bool = False, trace: bool = False,
                             guide: Optional[torch.Tensor] = None, guide_k: int = 5, arrive_rank: Optional[int] = None,
                             arrive_lp: Optional[float] = None, lookahead: Optional[int] = None, lookahead_record: bool = False,
                             offer: Optional[torch.Tensor] = None, rank_admissible: bool = False, arrive_among: str = "window",
                             sampler: Optional[Sampler] = None):
        """generate_paths that stops a user at its target (seqs[b, L - 1]) and the call when nobody is left
        (irs_generate_paths_until): returns (paths, status, steps_run, row_steps).  Paths are zero behind the target.
        `seqs` and `hep` are working state: modified, and unspecified afterwards.  One host read of 4 bytes per check.
        trace: as in generate_paths, a fifth member (lp_item, lp_target, rank_target), exactly zero behind a user's arrival.
        guide / guide_k: as in generate_paths -- with the Rec2Inf rule this loop is the reference's get_path.
        arrive_rank / arrive_lp: as in generate_paths (needs trace=True) -- a user is retired at the step that offered it its
        target, so the search stops as soon as the rule allows.
        lookahead / lookahead_record: as in generate_paths; the record is the last member, exactly zero behind a user's arrival.
        sampler: as in generate_paths; for the same seed the draws u are those of generate_paths bit for bit, and the paths those of
        generate_paths cut at the target wherever the lists agree (include/irs_hip.h); the record (the last member) is exactly zero
        behind a user's arrival."""
        seqs, users, hep, B, paths, status = self._greedy_call("generate_paths_until", seqs, users, hep, max_path_len, paths, status)
        stats = (ctypes.c_int64 * 2)(0, 0)
        with self._search_options(B, max_path_len, 0, sample, sample_k, exact_candidates=exact_candidates, exclude=exclude,
                                  no_repeat=no_repeat, trace=trace, guide=guide, guide_k=guide_k, arrive_rank=arrive_rank,
                                  arrive_lp=arrive_lp, lookahead=lookahead, lookahead_record=lookahead_record, offer=offer,
                                  rank_admissible=rank_admissible, arrive_among=arrive_among, sampler=sampler) as recorded:
            self._call(self.lib.irs_generate_paths_until, _ptr(seqs), _ptr(users), _ptr(hep), B, max_path_len, k, sweep,
                                                          int(sample), sample_k, seed, check_every, _ptr(paths), _ptr(status), stats)
        return (paths, status, int(stats[0]), int(stats[1])) + self._recorded(recorded, trace, lookahead is not None and lookahead_record)

    # ------------------------------------------------------------------ beam search (build-defined extension)
    def beam_step(self, state_in, val, ids0, lse, step: int, state_out, status):
        """One beam step; state = (seq[B,W,L] i64, hep[B,W] i32, cum[B,W] f64, paths[B,W,P] f32)."""
        kinds = (torch.int64, torch.int32, torch.float64, torch.float32)
        seq_i, hep_i, cum_i, paths_i = (self._inplace(t, k, "beam_step: state_in") for t, k in zip(state_in, kinds))
        seq_o, hep_o, cum_o, paths_o = (self._inplace(t, k, "beam_step: state_out") for t, k in zip(state_out, kinds))
        status = self._inplace(status, torch.int32, "beam_step: status")
        val, ids0 = self._dev(val, torch.float32), self._dev(ids0, torch.int64)
        B, W, _ = seq_i.shape
        lmax, lsum = lse if lse is not None else (None, None)
        if lmax is not None:
            lmax, lsum = self._dev(lmax, torch.float32), self._dev(lsum, torch.float32)
        self._call(self.lib.irs_beam_step, _ptr(seq_i), _ptr(hep_i), _ptr(cum_i), _ptr(paths_i), _ptr(val),
                                           _ptr(ids0), _ptr(lmax), _ptr(lsum), B, W, val.shape[1], step,
                                           paths_i.shape[2], _ptr(seq_o), _ptr(hep_o), _ptr(cum_o), _ptr(paths_o),
                                           _ptr(status))

    def beam_search(self, seqs: torch.Tensor, users: Optional[torch.Tensor], hep: torch.Tensor, max_path_len: int,
                    beam: int, k: int = 100, sweep: int = IRS_SWEEP_BF16, use_graph: bool = False,
                    want_windows: bool = False, exact_candidates: bool = False, exclude: Optional[torch.Tensor] = None,
                    no_repeat: bool = False, trace: bool = False, offer: Optional[torch.Tensor] = None,
                    arrive_rank: Optional[int] = None, arrive_lp: Optional[float] = None, target_weight: float = 0.0):
        """(paths[B,W,P] f32, scores[B,W] f64, status[B] i32[, windows[B,W,L]]); beam 0 is the best.
        trace: a beam trace is bound for this call (irs_bind_beam_trace) and the return value grows a last member, (lp_item,
        lp_target float32 [B, W, P], rank_target int32 [B, W, P]): the path trace's values along each output beam's ancestors.
        arrive_rank / arrive_lp / target_weight: a beam rule is set for this call and cleared after it (set_beam_rule; needs
        trace=True); this loop searches on behind an arrival."""
        seqs = self._dev(seqs, torch.int64)
        hep = self._dev(hep, torch.int32)
        if users is not None:
            users = self._dev(users, torch.int64)
        B = seqs.shape[0]
        paths = torch.zeros((B, beam, max_path_len), dtype=torch.float32, device=self.device)
        scores = torch.zeros((B, beam), dtype=torch.float64, device=self.device)
        status = torch.zeros(B, dtype=torch.int32, device=self.device)
        fin = torch.empty((B, beam, self.L), dtype=torch.int64, device=self.device) if want_windows else None
        with self._search_options(B, max_path_len, beam, graph=bool(use_graph), exact_candidates=exact_candidates, exclude=exclude,
                                  no_repeat=no_repeat, beam_trace=trace, offer=offer, arrive_rank=arrive_rank, arrive_lp=arrive_lp,
                                  target_weight=target_weight) as recorded:
            self._call(self.lib.irs_beam_search, _ptr(seqs), _ptr(users), _ptr(hep), B, beam, max_path_len, k, sweep,
                                                 int(use_graph), _ptr(paths), _ptr(scores), _ptr(fin), _ptr(status))
        out = (paths, scores, status, fin) if want_windows else (paths, scores, status)
        return out + self._recorded(recorded, trace, False)

    def beam_step_until(self, state_in, val, ids0, lse, step: int, stop_rule: int, state_out, done, status):
        """One beam step with the end symbol (irs_beam_step_until); state = beam_step's four tensors plus fin[B,W] i32;
        done[B] i32 is read and written."""
        kinds = (torch.int64, torch.int32, torch.float64, torch.float32, torch.int32)
        seq_i, hep_i, cum_i, paths_i, fin_i = (self._inplace(t, k, "beam_step_until: state_in") for t, k in zip(state_in, kinds))
        seq_o, hep_o, cum_o, paths_o, fin_o = (self._inplace(t, k, "beam_step_until: state_out") for t, k in zip(state_out, kinds))
        done = self._inplace(done, torch.int32, "beam_step_until: done")
        status = self._inplace(status, torch.int32, "beam_step_until: status")
        val, ids0 = self._dev(val, torch.float32), self._dev(ids0, torch.int64)
        B, W, _ = seq_i.shape
        lmax, lsum = lse if lse is not None else (None, None)
        if lmax is not None:
            lmax, lsum = self._dev(lmax, torch.float32), self._dev(lsum, torch.float32)
        self._call(self.lib.irs_beam_step_until, _ptr(seq_i), _ptr(hep_i), _ptr(cum_i), _ptr(paths_i), _ptr(fin_i), _ptr(val),
                   _ptr(ids0), _ptr(lmax), _ptr(lsum), B, W, val.shape[1], step, paths_i.shape[2], int(stop_rule), _ptr(seq_o),
                   _ptr(hep_o), _ptr(cum_o), _ptr(paths_o), _ptr(fin_o), _ptr(done), _ptr(status))

    def beam_search_until(self, seqs: torch.Tensor, users: Optional[torch.Tensor], hep: torch.Tensor, max_path_len: int,
                          beam: int, k: int = 100, sweep: int = IRS_SWEEP_BF16, stop_rule: int = _lib.IRS_BEAM_STOP_BEST,
                          check_every: int = 1, want_windows: bool = False, paths: Optional[torch.Tensor] = None,
                          scores: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
                          fin: Optional[torch.Tensor] = None, exact_candidates: bool = False,
                          exclude: Optional[torch.Tensor] = None, no_repeat: bool = False, trace: bool = False,
                          offer: Optional[torch.Tensor] = None, arrive_rank: Optional[int] = None,
                          arrive_lp: Optional[float] = None, target_weight: float = 0.0):
        """Beam search that ends a beam at its target (seqs[b, L - 1]) and retires finished users (irs_beam_search_until):
        (paths[B,W,P] f32, scores[B,W] f64, status[B] i32, fin[B,W] i32, steps_run, window_steps[, windows[B,W,L]]); beam 0 is
        the best.  One host read of 4 bytes per check.
        trace: as in beam_search, the last member; a finished beam's columns are exactly zero behind its arrival.
        arrive_rank / arrive_lp / target_weight: as in beam_search; an offered beam is finished at its arrival."""
        seqs = self._dev(seqs, torch.int64)
        hep = self._dev(hep, torch.int32)
        if users is not None:
            users = self._dev(users, torch.int64)
        B = seqs.shape[0]
        if seqs.shape[1] != self.L or hep.shape[0] != B or (users is not None and users.shape[0] != B):
            raise IrsError("beam_search_until: inconsistent shapes")
        if paths is None:
            paths = torch.zeros((B, beam, max_path_len), dtype=torch.float32, device=self.device)
        if scores is None:
            scores = torch.zeros((B, beam), dtype=torch.float64, device=self.device)
        if status is None:
            status = torch.zeros(B, dtype=torch.int32, device=self.device)
        if fin is None:
            fin = torch.zeros((B, beam), dtype=torch.int32, device=self.device)
        paths = self._inplace(paths, torch.float32, "beam_search_until: paths")
        scores = self._inplace(scores, torch.float64, "beam_search_until: scores")
        status = self._inplace(status, torch.int32, "beam_search_until: status")
        fin = self._inplace(fin, torch.int32, "beam_search_until: fin")
        if paths.shape != (B, beam, max_path_len) or scores.shape != (B, beam) or fin.shape != (B, beam) or status.shape != (B,):
            raise IrsError("beam_search_until: paths [B, W, P], scores / fin [B, W], status [B]")
        win = torch.empty((B, beam, self.L), dtype=torch.int64, device=self.device) if want_windows else None
        stats = (ctypes.c_int64 * 2)(0, 0)
        with self._search_options(B, max_path_len, beam, exact_candidates=exact_candidates, exclude=exclude, no_repeat=no_repeat,
                                  beam_trace=trace, offer=offer, arrive_rank=arrive_rank, arrive_lp=arrive_lp,
                                  target_weight=target_weight) as recorded:
            self._call(self.lib.irs_beam_search_until, _ptr(seqs), _ptr(users), _ptr(hep), B, beam, max_path_len, k, sweep,
                       int(stop_rule), int(check_every), _ptr(paths), _ptr(scores), _ptr(fin), _ptr(win), _ptr(status), stats)
        out = (paths, scores, status, fin, int(stats[0]), int(stats[1]))
        return (out + (win,) if want_windows else out) + self._recorded(recorded, trace, False)

    # ------------------------------------------------------------------ item-sharded loops below the ABI (comm.hip)
    def allgather_rows(self, comm: "Comm", rows_local: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        rows_local = self._dev(rows_local, torch.float32)
        B = rows_local.shape[0]
        if out is None:
            out = torch.empty((comm.world * B, self.d), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.irs_allgather_rows(self.h, comm.h, _ptr(rows_local), B, _ptr(out), self._stream()))
        return out

    def exchange_topk(self, comm: "Comm", keys_send: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[world, B, k] packed lists of all rows (this shard) -> [world, B, k] the world's lists of this rank's rows."""
        keys_send = self._dev(keys_send, torch.int64)
        W, B, k = keys_send.shape
        if W != comm.world:
            raise IrsError("exchange_topk: keys must be [world, B, k]")
        if out is None:
            out = torch.empty_like(keys_send)
        with torch.cuda.device(self.device):
            self._check(self.lib.irs_exchange_topk(self.h, comm.h, _ptr(keys_send), _ptr(out), B, k, self._stream()))
        return out

    def generate_paths_sharded(self, comm: "Comm", seqs: torch.Tensor, users: Optional[torch.Tensor], hep: torch.Tensor,
                               max_path_len: int, k: int = 100, sweep: int = IRS_SWEEP_BF16, sample=False, sample_k=3, seed=0,
                               use_graph: bool = False, paths: Optional[torch.Tensor] = None,
                               status: Optional[torch.Tensor] = None):
        """generate_paths over the item-sharded catalog: this rank's B users; every rank calls it together."""
        seqs = self._inplace(seqs, torch.int64, "generate_paths_sharded: seqs")
        hep = self._inplace(hep, torch.int32, "generate_paths_sharded: hep")
        if users is not None:
            users = self._dev(users, torch.int64)
        B = seqs.shape[0]
        if seqs.shape[1] != self.L or hep.shape[0] != B or (users is not None and users.shape[0] != B):
            raise IrsError("generate_paths_sharded: inconsistent shapes")
        if paths is None:
            paths = torch.zeros((B, max_path_len), dtype=torch.float32, device=self.device)
        if status is None:
            status = torch.zeros(B, dtype=torch.int32, device=self.device)
        paths = self._inplace(paths, torch.float32, "generate_paths_sharded: paths")
        status = self._inplace(status, torch.int32, "generate_paths_sharded: status")
        if paths.shape != (B, max_path_len):
            raise IrsError("generate_paths_sharded: paths must be [B, max_path_len]")
        self._comm_ref = comm  # a captured step holds RCCL nodes of this communicator: it must outlive the context's graphs
        with torch.cuda.device(self.device):
            self._check(self.lib.irs_generate_paths_sharded(self.h, comm.h, _ptr(seqs), _ptr(users), _ptr(hep), B, max_path_len, k,
                                                            sweep, int(sample), sample_k, seed, int(use_graph), _ptr(paths),
                                                            _ptr(status), self._stream()))
        return paths, status

    def beam_search_sharded(self, comm: "Comm", seqs: torch.Tensor, users: Optional[torch.Tensor], hep: torch.Tensor,
                            max_path_len: int, beam: int, k: int = 100, sweep: int = IRS_SWEEP_BF16, split_decode: bool = False,
                            use_graph: bool = False, want_windows: bool = False):
        """beam_search over the item-sharded catalog.  split_decode=False: this rank's own B users; True: the SAME users on
        every rank, their B * beam windows decoded 1/world each (one user's beams spread over the node)."""
        seqs = self._dev(seqs, torch.int64)
        hep = self._dev(hep, torch.int32)
        if users is not None:
            users = self._dev(users, torch.int64)
        B = seqs.shape[0]
        paths = torch.zeros((B, beam, max_path_len), dtype=torch.float32, device=self.device)
        scores = torch.zeros((B, beam), dtype=torch.float64, device=self.device)
        # the status pointer is part of the captured step's reuse key (capi: sh_ptr): a buffer of the engine's own, so that
        # a replay does not depend on which address the allocator hands out; the caller receives a copy
        if getattr(self, "_beam_status", None) is None or self._beam_status.numel() < B:
            self._beam_status = torch.zeros(max(B, 64), dtype=torch.int32, device=self.device)
        status = self._beam_status[:B]
        status.zero_()
        fin = torch.empty((B, beam, self.L), dtype=torch.int64, device=self.device) if want_windows else None
        self._comm_ref = comm  # (see generate_paths_sharded)
        with torch.cuda.device(self.device):
            self._check(self.lib.irs_beam_search_sharded(self.h, comm.h, _ptr(seqs), _ptr(users), _ptr(hep), B, beam, max_path_len, k,
                                                         sweep, int(split_decode), int(use_graph), _ptr(paths), _ptr(scores),
                                                         _ptr(fin), _ptr(status), self._stream()))
        status = status.clone()
        return (paths, scores, status, fin) if want_windows else (paths, scores, status)

    # ---- projection + cross entropy over the item-sharded catalog (ce_sharded.hip); every rank calls them together
    def ce_forward_sharded(self, comm: "Comm", xrows: torch.Tensor, labels0: torch.Tensor):
        """ce_forward of this rank's B rows (the same B on every rank; labels0 global 0-based, -1 = ignored) against the
        WHOLE catalog: (lse[B], label_score[B], loss[3] float64 over the rows of the whole world, identical on every rank)."""
        xrows = self._dev(xrows, torch.float32)
        labels0 = self._dev(labels0, torch.int64)
        if xrows.dim() != 2 or xrows.shape[1] != self.d or tuple(labels0.shape) != (xrows.shape[0],):
            raise IrsError(f"ce_forward_sharded: rows {tuple(xrows.shape)} / labels {tuple(labels0.shape)}, expected "
                           f"[B, {self.d}] / [B]")
        B = xrows.shape[0]
        lse = torch.empty(B, dtype=torch.float32, device=self.device)
        ls = torch.empty(B, dtype=torch.float32, device=self.device)
        loss = torch.empty(3, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.irs_ce_forward_sharded(self.h, comm.h, _ptr(xrows), _ptr(labels0), B, _ptr(lse), _ptr(ls),
                                                        _ptr(loss), self._stream()))
        return lse, ls, loss

    def ce_backward_sharded_scratch_bytes(self, B: int) -> int:
        n = self.lib.irs_ce_backward_sharded_scratch_bytes(self.h, B)
        if n == 0:
            raise IrsError(f"ce_backward_sharded: no scratch size for B={B} (need 1 <= world * B <= max_rows={self.max_rows})")
        return n

    def ce_backward_sharded(self, comm: "Comm", xrows: torch.Tensor, labels0: torch.Tensor, lse: torch.Tensor, scale: float,
                            accumulate: bool, dx: torch.Tensor, dw: torch.Tensor, db: torch.Tensor, scratch: torch.Tensor):
        """ce_backward over the item-sharded catalog (irs_ce_backward_sharded): dx[B, d] of this rank's rows (overwritten),
        dw[n_local, d] / db[n_local] of this rank's shard (+)= over the rows of the whole world.  lse: ce_forward_sharded's.
        scratch: uint8, at least ce_backward_sharded_scratch_bytes(B) bytes."""
        xrows = self._dev(xrows, torch.float32)
        labels0 = self._dev(labels0, torch.int64)
        lse = self._dev(lse, torch.float32)
        if xrows.dim() != 2 or xrows.shape[1] != self.d:
            raise IrsError(f"ce_backward_sharded: rows of shape {tuple(xrows.shape)}, expected [B, {self.d}]")
        B = xrows.shape[0]
        if tuple(labels0.shape) != (B,) or tuple(lse.shape) != (B,):
            raise IrsError(f"ce_backward_sharded: labels {tuple(labels0.shape)} / lse {tuple(lse.shape)}, expected [{B}]")
        dx = self._inplace(dx, torch.float32, "ce_backward_sharded dx")
        dw = self._inplace(dw, torch.float32, "ce_backward_sharded dw")
        db = self._inplace(db, torch.float32, "ce_backward_sharded db")
        scratch = self._inplace(scratch, torch.uint8, "ce_backward_sharded scratch")
        if tuple(dx.shape) != (B, self.d) or tuple(dw.shape) != (self.n_local, self.d) or tuple(db.shape) != (self.n_local,):
            raise IrsError(f"ce_backward_sharded: dx {tuple(dx.shape)} / dw {tuple(dw.shape)} / db {tuple(db.shape)}, expected "
                           f"{(B, self.d)} / {(self.n_local, self.d)} / {(self.n_local,)}")
        with torch.cuda.device(self.device):
            self._check(self.lib.irs_ce_backward_sharded(self.h, comm.h, _ptr(xrows), _ptr(labels0), _ptr(lse), B, float(scale),
                                                         1 if accumulate else 0, _ptr(dx), _ptr(dw), _ptr(db), _ptr(scratch),
                                                         scratch.numel(), self._stream()))
        return dx, dw, db

    # ------------------------------------------------------------------ decoder GEMM arithmetic
    @property
    def decoder_gemm(self) -> int:
        """IRS_GEMM_H3 (split-float16 MFMAs, the default), IRS_GEMM_X6 (split-bf16 MFMAs) or IRS_GEMM_F32 (float32 MFMAs):
        include/irs_hip.h.  The SELECTED mode (get / set round trips restore it); `decoder_gemm_effective` is what runs."""
        return int(self.lib.irs_get_decoder_gemm(self.h))

    @property
    def decoder_gemm_effective(self) -> int:
        """The arithmetic that runs: IRS_GEMM_X6 where IRS_GEMM_H3 is selected and the weights fail the float16 range bound."""
        return int(self.lib.irs_get_decoder_gemm_effective(self.h))

    @decoder_gemm.setter
    def decoder_gemm(self, mode: int):
        self._check(self.lib.irs_set_decoder_gemm(self.h, int(mode)))

    def debug_buffer(self, which: int, numel: int, dtype: torch.dtype) -> torch.Tensor:
        """(tests / lab) a view of one of the decoder's workspace buffers (irs_debug_ptr): what the last decode left behind."""
        p = self.lib.irs_debug_ptr(self.h, int(which))
        if not p:
            raise IrsError(f"irs_debug_ptr({which}) is null")
        off = int(p) - self._ws.data_ptr()
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        assert 0 <= off and off + nbytes <= self._ws.numel()
        return self._ws[off:off + nbytes].view(dtype)

    @property
    def decoder_seq(self) -> int:
        """Sequence-resident decoder (irs_set_decoder_seq, include/irs_hip.h): 0 off, 1 on, 2 auto (default: from 384 sequences
        per call up).  The setter takes False / True / None (= auto) or the numbers."""
        return int(self.lib.irs_get_decoder_seq(self.h))

    @decoder_seq.setter
    def decoder_seq(self, mode):
        self._check(self.lib.irs_set_decoder_seq(self.h, 2 if mode is None else int(mode)))

    @property
    def decoder_seq_last(self) -> bool:
        """True when the last decode took the sequence-resident path."""
        return bool(self.lib.irs_decoder_seq_last(self.h))

    @property
    def topk_dense(self) -> int:
        """Dense form of the swept top-k on small catalogs (irs_set_topk_dense, include/irs_hip.h): 0 never, 1 wherever the form
        is eligible, 2 auto (default).  The setter takes False / True / None (= auto) or the numbers."""
        return int(self.lib.irs_get_topk_dense(self.h))

    @topk_dense.setter
    def topk_dense(self, mode):
        self._check(self.lib.irs_set_topk_dense(self.h, 2 if mode is None else int(mode)))

    @property
    def topk_dense_last(self) -> bool:
        """True when the last top-k launch (score_topk, or the last step of a search loop run without a graph) took the dense form."""
        return bool(self.lib.irs_topk_dense_last(self.h))

    @property
    def decoder_route_last(self) -> Dict[str, object]:
        """(tests) The kernel route the last decode took (irs_decoder_route_last): plan / embed / layer / tail as their enum
        names (_lib.ROUTE_NAMES), the flags as bools, npl / nt as ints."""
        n = len(_lib.ROUTE_FIELDS)
        buf = (ctypes.c_int32 * n)()
        got = self.lib.irs_decoder_route_last(self.h, buf, n)
        if got < 0:
            raise IrsError(f"irs_decoder_route_last failed ({got}): no decode has run on this engine yet")
        if got != n:
            raise IrsError(f"irs_decoder_route_last wrote {got} fields, expected {n}")
        out: Dict[str, object] = {}
        for name, v in zip(_lib.ROUTE_FIELDS, buf):
            out[name] = _lib.ROUTE_NAMES[name][v] if name in _lib.ROUTE_NAMES else (int(v) if name in ("npl", "nt") else bool(v))
        return out

    @property
    def sharded_overlap(self) -> bool:
        """irs_set_sharded_overlap: generate_paths_sharded runs two user micro-batches per step with the collectives on a side
        stream (greedy choice; same results).  Off by default."""
        return bool(self.lib.irs_get_sharded_overlap(self.h))

    @sharded_overlap.setter
    def sharded_overlap(self, on: bool):
        self._check(self.lib.irs_set_sharded_overlap(self.h, 1 if on else 0))

    @property
    def h3_range_bound(self) -> float:
        """Largest operand magnitude the bound weights allow in the float16-plane kernels (irs_h3_range_bound; -1 before the
        weights are finalised).  At 32752 or more IRS_GEMM_H3 runs as IRS_GEMM_X6 and `decoder_gemm_effective` reports that."""
        return float(self.lib.irs_h3_range_bound(self.h))

    # ------------------------------------------------------------------ measurement
    def prof_enable(self, family: int):
        with torch.cuda.device(self.device):
            self._check(self.lib.irs_prof_enable(self.h, family))

    def prof_read(self):
        n = ctypes.c_int32()
        ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        with torch.cuda.device(self.device):
            self._check(self.lib.irs_prof_read(self.h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)))
        return n.value, ms.value, fl.value, by.value


class Comm:
    """irs_comm handle (include/irs_hip.h, multi-GPU section): the collectives of the item-sharded loops, enqueued on the
    engine's stream BELOW the C ABI.  With torch.distributed's "nccl" backend it is an RCCL communicator of its own
    (ncclCommInitRank over a unique id that rank 0 draws and the process group broadcasts); with "gloo" (the CPU
    rehearsal backend: several ranks, possibly on ONE GPU) the library calls back into gloo through the host.  world == 1
    without a process group gives a one-rank RCCL communicator (the single-GPU anchor runs the same code path)."""

    def __init__(self, device: torch.device, group=None, backend: Optional[str] = None):
        import torch.distributed as dist
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.group = group
        inited = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if inited else 1
        self.rank = dist.get_rank(group) if inited else 0
        if backend is None:
            backend = dist.get_backend(group) if inited else "nccl"
        self.backend = backend
        h = ctypes.c_void_p()
        if backend == "nccl":
            buf = ctypes.create_string_buffer(_lib.IRS_COMM_ID_BYTES)
            if self.rank == 0:
                if self.lib.irs_comm_unique_id(buf) != 0:
                    raise IrsError(f"irs_comm_unique_id: {self.lib.irs_comm_last_error().decode()}")
            if self.world > 1:
                box = [bytes(buf.raw)]
                dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
                buf = ctypes.create_string_buffer(box[0], _lib.IRS_COMM_ID_BYTES)
            with torch.cuda.device(self.device):
                rc = self.lib.irs_comm_init_rccl(ctypes.byref(h), buf, self.rank, self.world)
            if rc != 0:
                raise IrsError(f"irs_comm_init_rccl: {self.lib.irs_comm_last_error().decode()}")
        else:
            self._make_callbacks()
            rc = self.lib.irs_comm_init_callbacks(ctypes.byref(h), self.rank, self.world, None,
                                                  ctypes.cast(self._cb[0], ctypes.c_void_p), ctypes.cast(self._cb[1], ctypes.c_void_p),
                                                  ctypes.cast(self._cb[2], ctypes.c_void_p))
            if rc != 0:
                raise IrsError(f"irs_comm_init_callbacks: {self.lib.irs_comm_last_error().decode()}")
        self.h = h

    def __del__(self):
        try:
            import sys
            if sys.is_finalizing():
                return  # interpreter shutdown: the HIP runtime may already be going down under ncclCommDestroy (observed: a hang)
            if getattr(self, "h", None):
                self.lib.irs_comm_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @property
    def is_rccl(self) -> bool:
        return bool(self.lib.irs_comm_is_rccl(self.h))

    def _make_callbacks(self):
        """gloo through the host: wait for the stream, stage the payload in host memory, run the collective, copy back.
        (Not capturable, not fast: it exists so that the N > 1 code path runs where no second GPU does.)"""
        import numpy as np
        import torch.distributed as dist
        hip = ctypes.CDLL("libamdhip64.so")  # the copy torch has already loaded
        hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        D2H, H2D = 2, 1
        world, group, dev = self.world, self.group, self.device

        def fetch(ptr, n, stream):
            with torch.cuda.device(dev):
                if hip.hipStreamSynchronize(stream) != 0:
                    raise RuntimeError("hipStreamSynchronize")
                h = np.empty(n, dtype=np.uint8)
                if hip.hipMemcpy(h.ctypes.data, ptr, n, D2H) != 0:
                    raise RuntimeError("hipMemcpy D2H")
            return torch.from_numpy(h)

        def store(ptr, t):
            with torch.cuda.device(dev):
                if hip.hipMemcpy(ptr, t.data_ptr(), t.numel() * t.element_size(), H2D) != 0:
                    raise RuntimeError("hipMemcpy H2D")

        def allgather(user, send, recv, nbytes, stream):
            try:
                h = fetch(send, nbytes, stream)
                out = torch.empty(world * nbytes, dtype=torch.uint8)
                dist.all_gather_into_tensor(out, h, group=group)
                store(recv, out)
                return 0
            except Exception:  # noqa: BLE001 -- reported through the C return code
                return 1

        def alltoall(user, send, recv, nbytes, stream):
            try:
                h = fetch(send, world * nbytes, stream)
                out = torch.empty_like(h)
                dist.all_to_all_single(out, h, group=group)
                store(recv, out)
                return 0
            except Exception:  # noqa: BLE001
                return 1

        def allreduce(user, buf, count, op, stream):
            try:
                h = fetch(buf, 4 * count, stream).view(torch.float32)
                dist.all_reduce(h, op=dist.ReduceOp.MAX if op == 1 else dist.ReduceOp.SUM, group=group)
                store(buf, h)
                return 0
            except Exception:  # noqa: BLE001
                return 1

        self._cb = (_lib.ALLGATHER_FN(allgather), _lib.ALLTOALL_FN(alltoall), _lib.ALLREDUCE_F32_FN(allreduce))  # kept alive
