"""Decodes behind long windows (256 < max_len <= 1024, irs_create_ex with IRS_CREATE_LONG_WINDOWS) as a table of cases, in the form
of tests/decoder_route_cases.py: config, batch, and the WHOLE route the decode must take (test infrastructure of
tests/test_gpu_long_window_decoder.py).

Above 256 tokens decode_route never takes att_fused, plan IN_EMBED, the sequence-resident launch, float16 K / V planes or the
FRAG_FUSED family (every predicate of theirs holds L <= 256, directly or through attn16_ok): one sequence plans with k_plan_small,
35200 rows of c2 run the fragment-major family WITHOUT the fused block (FRAG_BLOCK, float32, kv_only), d = 256 stays on the wide
16-token kernel.  The attention behind every one of them is k_attn_long (all rows) and k_attn_row_long (the consumed row); they
are not route fields, the table reaches their forms through its head dims: 5 (unaligned), 8, 16, 32 and 64.

Every case has n_layers = 2: the second layer reads what the first one's attention wrote."""
from decoder_route_cases import Case, R

ANY = R("SMALL", "ANY_QKV", "ANY", "ANY", "rows_only small_plan")
SM16_X6 = R("SMALL", "SMALL16_QKV", "SMALL16", "SMALL16", "rows_only small_plan x6")


def _c(id_, cfg, L, B, route, evaluator=False, **over):
    return Case(id_, cfg, B, route, over=dict(max_len=L, n_layers=2, **over), evaluator=evaluator)


CASES = [
    _c("tiny_L257_b5", "tiny", 257, 5, ANY),                   # head dim 8; one token beyond the old limit
    _c("tiny_L1024_b3", "tiny", 1024, 3, ANY),                 # the maximum length
    _c("default_L272_b9", "default", 272, 9, ANY),             # d = 30, head dim 5: the unaligned forms
    _c("c1_L320_b7", "c1", 320, 7, ANY),                       # head dim 16
    _c("c2_L320_b1", "c2", 320, 1, SM16_X6),                   # one sequence: no att_fused, no IN_EMBED plan
    _c("c2_L320_b40", "c2", 320, 40, SM16_X6),                 # the 16-token layer kernel
    # 35200 rows: fragment-major without the fused block; layer 0's q | k | v come from the float32 embed kernel
    _c("c2_L320_b110", "c2", 320, 110, R("MULTI", "FRAG_QKV", "FRAG_BLOCK", "SMALL16", "rows_only frag kv_only x6")),
    _c("c2_h2_L288_b6", "c2", 288, 6, R("SMALL", "SMALL16_QKV", "SMALL16", "SMALL16", "rows_only small_plan"), n_heads=2),  # head dim 64
    _c("c4d_L320_b4", "c4d", 320, 4, R("SMALL", "PACKED", "WIDE", "WIDE", "rows_only small_plan x6")),  # the wide 16-token kernel
    _c("eval_c2_L320_b6", "c2", 320, 6, SM16_X6, evaluator=True),             # causal mask, post-padded
    _c("eval_default_L300_b6", "eval_default", 300, 6, ANY, evaluator=True),  # causal mask at small d
]

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "duplicate case ids"

# the cases on whose engine (and route: at most 64 sequences, the same as the case's own) the batch of special windows runs too
CONTENT_CASES = ("tiny_L257_b5", "tiny_L1024_b3", "default_L272_b9", "c2_L320_b40", "c2_h2_L288_b6", "eval_c2_L320_b6")
N_CONTENT = 10  # sequences of that batch (test_gpu_long_window_decoder.py: _content_batch)


def max_seqs(key) -> int:
    return max([c.B for c in CASES if c.engine_key() == key] + [N_CONTENT])
