"""The decoder's kernel routes as a table of cases (test infrastructure, shared by tests/test_decoder_routes.py on the CPU and
tests/test_gpu_decoder_routes.py on the GPU).

decode_route() in influentialrs_amd/csrc/decoder.hip picks the kernels of one irs_decode; irs_decoder_route_last reports the
choice (include/irs_hip.h).  Every case below names a decode -- config, batch, rows-only or full, arithmetic, sequence-resident
mode, attention arithmetic, IRN or evaluator -- and the WHOLE route it must take.  Cases come in pairs across each threshold of
decode_route (rows = B x L of the synthetic configs, influentialrs_amd/synth.py), so that moving a threshold, or a refactor that
changes a predicate, fails a named case instead of silently decoding through another kernel.

Attention variants are not route fields; the table reaches them through its head dims: 5 (default, not float4-aligned), 8 (c1 with
8 heads), 16 (c1), 32 (c2, c4d) and 64 (c2 with 2 heads)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict

from influentialrs_amd import synth
from influentialrs_amd._lib import ROUTE_FIELDS

FLAGS = ("rows_only", "small_plan", "frag", "seq", "kv_planes", "att_fused", "kv_only", "x6")


def R(plan: str, embed: str, layer: str, tail: str, flags: str = "", npl: int = 2, nt: int = 4) -> Dict[str, object]:
    """A whole route: the enum fields by name, `flags` = the flags that are on (every other flag is off)."""
    on = flags.split()
    assert set(on) <= set(FLAGS), on
    r = dict(plan=plan, embed=embed, layer=layer, tail=tail, npl=npl, nt=nt, **{f: f in on for f in FLAGS})
    assert set(r) == set(ROUTE_FIELDS)
    return r


@dataclass(frozen=True)
class Case:
    id: str
    cfg: str                    # synth config name
    B: int
    route: Dict[str, object]    # the expected irs_decoder_route_last, every field
    over: Dict[str, int] = field(default_factory=dict)  # config overrides
    rows_only: bool = True      # decode(want_x=False, pos=...); False: the full window (want_x=True, pos=...)
    gemm: str = "h3"            # irs_set_decoder_gemm: h3 / x6 / f32
    seq: object = "auto"        # irs_set_decoder_seq: 0 / 1 / "auto"
    attn: str = "h3"            # IRS_ATTN_GEMM at engine creation: h3 (the default) / f32
    evaluator: bool = False     # SampleNet (causal mask, post-padded windows, no user factor)
    full_check: bool = True     # rows-only: decode the full window too and compare the consumed rows over the whole batch

    def config(self):
        base = dict(self.over)
        if self.evaluator:
            base.setdefault("n_user", 0)
        return synth.make_config(self.cfg, **base)

    def engine_key(self):
        """Cases that may share one engine (the workspace is sized for the largest B of the group)."""
        return (self.cfg, tuple(sorted(self.over.items())), self.evaluator, self.attn)


SM16 = ("SMALL16_QKV", "SMALL16", "SMALL16")
FUSED = ("FRAG_QKV", "FRAG_FUSED", "SMALL16")
SEQ = ("SEQ", "FRAG_FUSED", "SMALL16")

CASES = [
    # ---- plan: the single-workgroup plan up to 64 sequences (irs_small_plan); one sequence plans inside the embed kernel when the
    #      layer kernel also runs the attention (att_fused: d = 128, 4 heads) or the generic small kernel serves the shape
    Case("c2_b1_att_fused", "c2", 1, R("IN_EMBED", *SM16, "rows_only small_plan att_fused x6")),
    Case("c2_b2", "c2", 2, R("SMALL", *SM16, "rows_only small_plan x6")),
    Case("c2_b64", "c2", 64, R("SMALL", *SM16, "rows_only small_plan x6")),
    Case("c2_b65", "c2", 65, R("MULTI", *SM16, "rows_only x6")),
    Case("default_b1_any", "default", 1, R("IN_EMBED", "ANY_QKV", "ANY", "ANY", "rows_only small_plan")),
    Case("c4d_b1", "c4d", 1, R("SMALL", "PACKED", "WIDE", "WIDE", "rows_only small_plan x6")),
    Case("c2_nl1_b1", "c2", 1, R("SMALL", "PACKED", "SMALL16", "SMALL16", "rows_only small_plan"), over=dict(n_layers=1)),
    # rows-only needs L >= 4: shorter windows decode in full and gather the consumed rows
    Case("tiny_L2", "tiny", 5, R("NONE", "FULL", "ANY", "ANY"), over=dict(max_len=2)),
    Case("tiny_L3", "tiny", 5, R("NONE", "FULL", "ANY", "ANY"), over=dict(max_len=3)),
    Case("tiny_L4", "tiny", 5, R("SMALL", "ANY_QKV", "ANY", "ANY", "rows_only small_plan"), over=dict(max_len=4)),
    # ---- the 16-token layer kernel (d = 128, ffn 256) up to SMALL_ROWS_MAX = 32768 rows, then the fragment-major fused kernel;
    #      32 tokens per workgroup beyond SMALL_MT2_ROWS = 8192 rows (c2: 40 / 41 sequences)
    Case("c2_b40", "c2", 40, R("SMALL", *SM16, "rows_only small_plan x6")),
    Case("c2_b41", "c2", 41, R("SMALL", *SM16, "rows_only small_plan x6")),
    Case("c2_b163", "c2", 163, R("MULTI", *SM16, "rows_only x6")),
    Case("c2_b164", "c2", 164, R("MULTI", *FUSED, "rows_only frag kv_planes kv_only x6")),
    Case("c2_L256_b128", "c2", 128, R("MULTI", *SM16, "rows_only x6"), over=dict(max_len=256)),
    Case("c2_L256_b129", "c2", 129, R("MULTI", *FUSED, "rows_only frag kv_planes kv_only x6"), over=dict(max_len=256)),
    # ---- the generic small kernel (d <= 96) up to 65536 rows; its rows-only last layer up to 2048 sequences
    Case("default_b1092", "default", 1092, R("MULTI", "ANY_QKV", "ANY", "ANY", "rows_only")),
    Case("default_b1093", "default", 1093, R("MULTI", "PACKED", "GEMM_LN", "ANY", "rows_only")),
    Case("default_b2048", "default", 2048, R("MULTI", "PACKED", "GEMM_LN", "ANY", "rows_only")),
    Case("default_b2049", "default", 2049, R("MULTI", "PACKED", "GEMM_LN", "GEMM_LN", "rows_only")),
    Case("c1_b1310", "c1", 1310, R("MULTI", "ANY_QKV", "ANY", "ANY", "rows_only")),
    Case("c1_b1311", "c1", 1311, R("MULTI", "FRAG", "FRAG_GEMM", "GEMM_LN", "rows_only frag")),
    # ---- fragment-major families: FRAG_BLOCK where the fused block's head-dim-32 attention is out (8 heads: hd 16; 2 heads: hd
    #      64), FRAG_GEMM for other widths; fragment-major from 2048 rows (c2 with ffn 128: 10 / 11 sequences)
    Case("c2_h8_b72", "c2", 72, R("MULTI", *SM16, "rows_only"), over=dict(n_heads=8)),
    Case("c2_h8_b176", "c2", 176, R("MULTI", "FRAG_QKV", "FRAG_BLOCK", "SMALL16", "rows_only frag kv_only"), over=dict(n_heads=8)),
    Case("c2_h2_b72", "c2", 72, R("MULTI", *SM16, "rows_only"), over=dict(n_heads=2)),
    Case("c2_h2_b176", "c2", 176, R("MULTI", "FRAG_QKV", "FRAG_BLOCK", "SMALL16", "rows_only frag kv_only"), over=dict(n_heads=2)),
    Case("c2_f128_b10", "c2", 10, R("SMALL", "PACKED", "GEMM_LN", "GEMM_LN", "rows_only small_plan"), over=dict(ffn_dim=128)),
    Case("c2_f128_b11", "c2", 11, R("SMALL", "FRAG_QKV", "FRAG_GEMM", "GEMM_LN", "rows_only small_plan frag"), over=dict(ffn_dim=128)),
    Case("c1_h8_b72", "c1", 72, R("MULTI", "ANY_QKV", "ANY", "ANY", "rows_only"), over=dict(n_heads=8)),
    # ---- d = 256: the 16-token wide kernel below 32768 rows; from there the split-precision fused kernel at 8 accumulator tiles
    #      (x6d: rows-only, h3 / x6 arithmetic) or the LN-fused per-GEMM kernels (f32, full decodes); other d > 128 shapes: GEMM
    Case("c4d_b163", "c4d", 163, R("MULTI", "PACKED", "WIDE", "WIDE", "rows_only x6")),
    Case("c4d_b164", "c4d", 164, R("MULTI", "FRAG_QKV", "FRAG_FUSED", "GEMM", "rows_only frag kv_planes kv_only x6", nt=8)),
    Case("c4d_b163_f32", "c4d", 163, R("MULTI", "PACKED", "WIDE", "WIDE", "rows_only", npl=3), gemm="f32"),
    Case("c4d_b164_f32", "c4d", 164, R("MULTI", "PACKED", "GEMM_LN", "WIDE", "rows_only", npl=3), gemm="f32"),
    Case("c4d_full_b163", "c4d", 163, R("NONE", "FULL", "WIDE", "WIDE", "x6"), rows_only=False),
    Case("c4d_full_b164", "c4d", 164, R("NONE", "FULL", "GEMM_LN", "WIDE", "x6"), rows_only=False),
    Case("c4d_f128_b16", "c4d", 16, R("SMALL", "PACKED", "GEMM", "GEMM", "rows_only small_plan"), over=dict(ffn_dim=128)),
    Case("d192_b16", "c2", 16, R("SMALL", "PACKED", "GEMM", "GEMM", "rows_only small_plan"),
         over=dict(emb_dim=192, n_heads=6, ffn_dim=200)),
    Case("d192_b168", "c2", 168, R("MULTI", "PACKED", "GEMM_LN", "GEMM", "rows_only"), over=dict(emb_dim=192, n_heads=6, ffn_dim=200)),
    # ---- flags: float16 K / V planes off through IRS_ATTN_GEMM=f32, the float32 mode and a single layer; three bf16 planes (x6)
    Case("c2_b164_attn_f32", "c2", 164, R("MULTI", *FUSED, "rows_only frag kv_only x6"), attn="f32"),
    Case("c2_b164_f32", "c2", 164, R("MULTI", *FUSED, "rows_only frag kv_only", npl=3), gemm="f32"),
    Case("c2_nl1_b164", "c2", 164, R("MULTI", "FRAG", "FRAG_FUSED", "SMALL16", "rows_only frag"), over=dict(n_layers=1)),
    Case("c2_b600_x6", "c2", 600, R("MULTI", *FUSED, "rows_only frag kv_planes kv_only x6", npl=3), gemm="x6"),
    # ---- full decodes (plan NONE)
    Case("c2_full_b8", "c2", 8, R("NONE", "FULL", "SMALL16", "SMALL16", "x6"), rows_only=False),
    Case("c2_full_b164", "c2", 164, R("NONE", "FRAG_QKV", "FRAG_FUSED", "SMALL16", "frag kv_planes x6"), rows_only=False),
    Case("default_full_b8", "default", 8, R("NONE", "FULL", "ANY", "ANY"), rows_only=False),
    # ---- the sequence-resident launch: automatic from SEQ_AUTO_MIN_SEQS = 384 sequences, forced from any fused shape, bounded by
    #      its plan kernel at 8192 sequences; not in x6 mode; a shorter window at the 32768-row edge (64 tokens: 512 / 513)
    Case("c2_b383", "c2", 383, R("MULTI", *FUSED, "rows_only frag kv_planes kv_only x6")),
    Case("c2_b384", "c2", 384, R("MULTI", *SEQ, "rows_only frag seq kv_planes kv_only x6")),
    Case("c2_b164_seq1", "c2", 164, R("MULTI", *SEQ, "rows_only frag seq kv_planes kv_only x6"), seq=1),
    Case("c2_b8192_seq1", "c2", 8192, R("MULTI", *SEQ, "rows_only frag seq kv_planes kv_only x6"), seq=1, full_check=False),
    Case("c2_b8193_seq1", "c2", 8193, R("MULTI", *FUSED, "rows_only frag kv_planes kv_only x6"), seq=1, full_check=False),
    Case("c2_L64_b512_seq1", "c2", 512, R("MULTI", *SM16, "rows_only x6"), over=dict(max_len=64), seq=1),
    Case("c2_L64_b513_seq1", "c2", 513, R("MULTI", *SEQ, "rows_only frag seq kv_planes kv_only x6"), over=dict(max_len=64), seq=1),
    # ---- the evaluator (causal mask, post-padded windows)
    Case("eval_c2_b16", "c2", 16, R("SMALL", *SM16, "rows_only small_plan x6"), evaluator=True),
    Case("eval_c2_b600", "c2", 600, R("MULTI", *SEQ, "rows_only frag seq kv_planes kv_only x6"), evaluator=True),
    Case("eval_default_b40", "eval_default", 40, R("SMALL", "ANY_QKV", "ANY", "ANY", "rows_only small_plan"), evaluator=True),
]

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "duplicate case ids"

# Values decode_route never assigns to a field, with the reason (the coverage test accepts exactly these as unreached).
UNREACHABLE = {
    ("tail", "FRAG_GEMM"): "the rows-only last layer works on B gathered row-major rows: only GEMM / GEMM_LN / SMALL16 / WIDE / ANY",
    ("tail", "FRAG_BLOCK"): "as FRAG_GEMM",
    ("tail", "FRAG_FUSED"): "as FRAG_GEMM",
}


def split_precision(c: Case) -> bool:
    """The consumed rows went through the split-precision kernels (k_block_x6 and its embed prologue, or the sequence-resident
    launch): X_TOL_X6 is their bar.  r.x6 alone says only that the mode and the weight streams exist."""
    r = c.route
    return bool(r["x6"]) and r["layer"] == "FRAG_FUSED"


def max_seqs(key) -> int:
    return max(c.B for c in CASES if c.engine_key() == key)

