"""Helpers shared by the -m gpu tests: build an Engine from synthetic weights."""
import contextlib
import os

import numpy as np
import torch

from influentialrs_amd import synth
from influentialrs_amd.engine import Engine
from influentialrs_amd._lib import IRS_MASK_CAUSAL, IRS_MASK_IRN


@contextlib.contextmanager
def _attn_env(attn):
    if attn is None:
        yield
        return
    old = os.environ.pop("IRS_ATTN_GEMM", None)
    try:
        if attn != "h3":
            os.environ["IRS_ATTN_GEMM"] = attn
        yield
    finally:
        os.environ.pop("IRS_ATTN_GEMM", None)
        if old is not None:
            os.environ["IRS_ATTN_GEMM"] = old


def make_engine(cfg, sd_np, *, evaluator=False, max_rows=64, max_seqs=0, rank=0, world=1, max_k=100, device="cuda:0", attn=None,
                arena_fill=None):
    """attn: IRS_ATTN_GEMM while the context is created ("f32"; "h3": unset, the default; None: the environment as it is).
    arena_fill: the derived arena exists before the first finalisation, every byte = arena_fill (otherwise finalize() allocates
    it uninitialised)."""
    dev = torch.device(device)
    with _attn_env(attn):
        eng = Engine(n_item=cfg.n_item, n_user=(0 if evaluator else cfg.n_user), d=cfg.emb_dim, max_len=cfg.max_len,
                     n_heads=cfg.n_heads, ffn_dim=cfg.ffn_dim, n_layers=cfg.n_layers,
                     u_dim=(0 if evaluator else cfg.u_emb_dim),
                     mask_mode=(IRS_MASK_CAUSAL if evaluator else IRS_MASK_IRN), device=dev, max_rows=max_rows,
                     max_seqs=max_seqs, max_k=max_k, rank=rank, world=world)
    if arena_fill is not None:
        eng._arena = torch.full((int(eng.lib.irs_derived_bytes(eng.h)) + 256,), arena_fill, dtype=torch.uint8, device=dev)
    # (a value may already be a tensor on the device: upload_state_dict's, shared by many engines)
    sd = {k: (v if torch.is_tensor(v) else torch.from_numpy(v)).to(dev) for k, v in sd_np.items()}
    eng.bind_state_dict(sd)
    return eng


def upload_state_dict(sd_np, device="cuda:0"):
    """A state dict on the device, once, for tests that build many engines on the same weights (an engine reads the bound
    tensors where they lie and never writes them)."""
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(torch.device(device)) for k, v in sd_np.items()}


def path_only_engine(max_len, *, n_item=64, max_k=128, device="cuda:0"):
    """Engine with a 1-layer dummy decoder and the window length a case needs, for tests of the path-search kernels
    alone (path / beam step, pack / merge, evaluation batch): they take their inputs from the caller, not from a model."""
    cfg = synth.make_config("tiny", n_item=n_item, emb_dim=16, n_heads=2, n_layers=1, max_len=max_len, ffn_dim=8, n_user=2)
    return make_engine(cfg, synth.irn_state_dict(cfg, seed=1), max_rows=64, max_seqs=1, max_k=max_k, device=device)


def _scoring_only(n_item, d, W, b):
    nh = d // 32 if d % 32 == 0 else 1
    cfg = synth.make_config("tiny", n_item=n_item, emb_dim=d, n_heads=nh, n_layers=1, max_len=4, ffn_dim=8, n_user=2)
    sd = synth.irn_state_dict(cfg, seed=1)
    sd["project.weight"] = W
    sd["project.bias"] = b
    return cfg, sd


def scoring_only_engine(n_item, d, W, b, *, max_rows=64, rank=0, world=1, max_k=100, device="cuda:0"):
    """Engine with a 1-layer dummy decoder, for tests of the scoring kernels alone."""
    cfg, sd = _scoring_only(n_item, d, W, b)
    return make_engine(cfg, sd, max_rows=max_rows, max_seqs=1, rank=rank, world=world, max_k=max_k, device=device)


def scoring_only_engines(n_item, d, W, b, *, max_rows=64, max_k=100, device="cuda:0"):
    """scoring_only_engine over and over on one catalog: the weights are generated and uploaded once, every call of the
    returned function builds a new engine (context, workspace, derived catalog) on them."""
    cfg, sd = _scoring_only(n_item, d, W, b)
    sd = upload_state_dict(sd, device)
    return lambda: make_engine(cfg, sd, max_rows=max_rows, max_seqs=1, max_k=max_k, device=device)
