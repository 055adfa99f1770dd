/*
 * irs_hip.h -- C ABI of libirs_hip.so: the MI355X (gfx950) implementation of
 * InfluentialRS's sequential next-item scoring and persuasion-path search.
 *
 * The reference (JackShDr/InfluentialRS) has NO native/FFI interface for this
 * path: its boundary is the Python class API of model/influentialRS.py
 * (SURVEY.md section 8b, row B1).  This ABI is therefore NEW and sits below
 * that class API; each entry point names the reference call site whose
 * arithmetic it replaces.  The Python front-end (influentialrs_amd/model/)
 * keeps the reference's class/method signatures and calls these through
 * ctypes; INTEGRATION.md shows the binding a maintainer of the reference
 * would add.
 *
 * Conventions
 *  - every function returns 0 on success, a negative IRS_E_* code otherwise;
 *    no C++ exception crosses the ABI; irs_last_error() gives the message.
 *  - every pointer marked "dev" is a device (HBM) pointer owned by the caller
 *    (e.g. torch.Tensor.data_ptr()); the library never frees it.
 *  - nothing is allocated after irs_create(): scratch lives in a caller-owned
 *    workspace sized by irs_workspace_bytes() and bound by irs_bind_workspace().
 *  - all work is enqueued on the caller's stream (a hipStream_t passed as
 *    void*); no call synchronises the device unless documented.
 *  - one context <-> one device, one stream at a time (not re-entrant).  Kernels
 *    are launched on the CURRENT HIP device: the caller makes the device that
 *    owns the context's pointers current around every call (the Python engine
 *    does: influentialrs_amd/engine.py Engine._call).
 *  - item ids crossing the ABI in "ids0" arguments are 0-based GLOBAL catalog
 *    positions (reference item id = ids0 + 1, influentialRS.py:376,422;
 *    0 is the pad id in sequences, which carry 1-based ids like the reference).
 *  - total order used by every selection: score descending, then id
 *    ascending (torch's own tie order is unspecified).
 *  - indices are the caller's responsibility, as with any device gather: sequence entries in [0, n_item]
 *    (0 = pad), user ids in [0, n_user), label / candidate ids0 in [0, n_item) or negative where documented;
 *    nn.Embedding's IndexError has no device-side counterpart here.  Shapes and buffer sizes ARE checked
 *    (IRS_E_INVALID).
 */
#ifndef IRS_HIP_H
#define IRS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRS_ABI_VERSION 1

/* error codes */
#define IRS_OK 0
#define IRS_E_INVALID (-1)     /* bad argument / shape */
#define IRS_E_STATE (-2)       /* weights or workspace not bound */
#define IRS_E_HIP (-3)         /* HIP runtime error (message has the hipError) */
#define IRS_E_UNSUPPORTED (-4) /* shape outside the kernels' envelope */

/* attention mask flavours */
#define IRS_MASK_IRN 0    /* InfluentialNet as called: allowed = r_u[b], last column = 1.0
                             (_generate_square_subsequent_mask, influentialRS.py:120-155,
                             called at :183-184) + key padding (:171) */
#define IRS_MASK_CAUSAL 1 /* SampleNet: 0 / -inf causal (uRS.py:47-50) + key padding (:53) */

/* scoring precision of the catalog sweep */
#define IRS_SWEEP_BF16 0 /* bf16 MFMA filter with a proven error bound, then exact fp32
                            re-scoring of the survivors: results identical to IRS_SWEEP_F32 */
#define IRS_SWEEP_F32 1  /* fp32 MFMA sweep (exact k-ordered fma chain) */
#define IRS_SWEEP_EXHAUSTIVE 2 /* irs_score_topk only: every item through the exact VALU chain,
                                  one workgroup per row (fallback kernel; yard-stick in tests) */

/* per-row status bits written by the selection kernels */
#define IRS_ROW_OK 0
#define IRS_ROW_FALLBACK 1     /* candidate buffers overflowed; row was re-done by the exhaustive exact kernel
                                  (dense form, irs_set_topk_dense: more than 1024 items within the filter's error of the k-th) */
#define IRS_ROW_NO_CANDIDATE 2 /* every one of the k candidates is in the window
                                  (the reference raises IndexError at influentialRS.py:429) */
#define IRS_ROW_FEWER_THAN_K 4 /* catalog shard has fewer than k items; tail filled with (-inf, -1) */
#define IRS_ROW_RESCUED 8      /* the window hid the row's top-k list; irs_topk_ensure_survivors replaced it by the exact
                                  best items outside the window */
#define IRS_ROW_OFFERED 16     /* an arrival rule fired for the row (irs_set_arrival_rule): its list was rewritten to the
                                  target alone */

#define IRS_MAX_SAMPLE_K 8 /* sampled path steps draw among at most this many survivors (reference default: 3);
                              larger sample_k -> IRS_E_UNSUPPORTED */

typedef struct irs_ctx irs_ctx;

typedef struct irs_dims {
    int64_t n_item;   /* catalog size N (global) */
    int64_t n_user;   /* rows of user_embedder (0 for SampleNet) */
    int32_t d;        /* emb_dim (even, <= 256) */
    int32_t max_len;  /* L (<= 256; <= IRS_MAX_LEN_LONG through irs_create_ex with IRS_CREATE_LONG_WINDOWS) */
    int32_t n_heads;  /* H, divides d; d / H <= 64 */
    int32_t ffn_dim;  /* F */
    int32_t n_layers;
    int32_t u_dim;    /* u_emb_dim (0 for SampleNet) */
    int32_t mask_mode;/* IRS_MASK_* */
    int32_t max_rows; /* upper bound on scored rows per call */
    int32_t max_k;    /* upper bound on k of irs_score_topk (reference: 100) */
    int32_t max_seqs; /* upper bound on sequences per irs_decode call (0 -> max_rows) */
} irs_dims;

/* item-dimension shard held by this context: rows
 * [item_lo, item_hi) of project.weight / project.bias. */
typedef struct irs_shard {
    int32_t rank;
    int32_t world;
    int64_t item_lo;
    int64_t item_hi;
} irs_shard;

int irs_abi_version(void);
const char *irs_last_error(const irs_ctx *ctx); /* ctx may be NULL: last create() error */

int irs_create(irs_ctx **out, const irs_dims *dims, const irs_shard *shard);
/* irs_create with flags.  flags == 0 is irs_create exactly (max_len in [2, 256]).  IRS_CREATE_LONG_WINDOWS admits max_len in
 * [2, IRS_MAX_LEN_LONG]; every other check is unchanged, and a context with max_len <= 256 is the one irs_create gives (same
 * kernels, same routes, same bytes).  An unknown flag bit -> IRS_E_INVALID with a message (irs_last_error(NULL)).
 * Above 256 the decoder's all-rows attention streams K / V through LDS in key chunks (k_attn_long) and the last layer's row
 * walks key chunks of 256; the split-precision fused routes (sequence-resident launch, float16 K / V planes, the fused block
 * and the attention inside the 16-token kernel) are never taken.  The bound of 1024 is what the search kernels pay per window:
 * 16 window registers (64-bit) per lane in the path / beam / survivor-flag steps, a 32-word key bitmask in the attention, an
 * 8 KB (16 KB with path entries) sort buffer in the survivor strips, and 2 x max_seqs x (8 L + 20) bytes of compaction copies
 * in the _until loops. */
#define IRS_CREATE_LONG_WINDOWS 1u
#define IRS_MAX_LEN_LONG 1024
int irs_create_ex(irs_ctx **out, const irs_dims *dims, const irs_shard *shard, uint32_t flags);
void irs_destroy(irs_ctx *ctx);

/* ---- weights -----------------------------------------------------------
 * Bind one float32 device tensor by its reference state_dict key
 * (item_embedder.weight | word_embedder.weight,
 * user_embedder.weight, pos_embedder.pe, user_mask_layer.{weight,bias},
 * project.{weight,bias}, decoder.layers.<l>.{self_attn,multihead_attn}.
 * {in_proj_weight,in_proj_bias,out_proj.weight,out_proj.bias},
 * decoder.layers.<l>.linear{1,2}.{weight,bias}, decoder.layers.<l>.norm{1,2,3}.
 * {weight,bias}); a leading "module." (nn.DataParallel, pipeline.py:43-44) is
 * accepted.  project.weight / project.bias are the LOCAL shard rows
 * ([item_hi-item_lo, d] / [item_hi-item_lo]).  numel is checked. */
int irs_bind_weight(irs_ctx *ctx, const char *name, const float *dev_ptr, int64_t numel);

/* Bytes of the derived-weight arena (bf16 MFMA-fragment-packed copy of the
 * project shard, padded bias, per-layer cross-attention constants). */
size_t irs_derived_bytes(const irs_ctx *ctx);
/* Build the derived weights into the caller's arena (async on stream).
 * Must be called after all weights are bound and again after any weight
 * changes in place. */
int irs_finalize_weights(irs_ctx *ctx, void *dev_arena, size_t bytes, void *stream);

size_t irs_workspace_bytes(const irs_ctx *ctx);
int irs_bind_workspace(irs_ctx *ctx, void *dev_ws, size_t bytes);
/* Calls on one context, in any order (tests/test_gpu_engine_state.py holds the three statements below):
 *  - The caller orders them: all on one stream, or with events between streams.  Every entry point works on the stream it is
 *    given and nowhere else, so other streams of the process, the null stream included, and other contexts may run beside it.
 *  - Between calls the workspace's contents belong to the library.  The memory needs no initialisation before the bind, and
 *    binding the same or other memory again at any time (with no call of the context in flight) starts from a clean state.
 *  - A call's results do not depend on the calls before it: other entry points, other shapes, other bindings since unbound.  The
 *    one exception is documented where it lives: bit 0 (IRS_ROW_FALLBACK) of irs_score_topk_carry's status words. */

/* ---- decoder (replaces InfluentialNet.decoding, influentialRS.py:157-200;
 *      SampleNet.decoding, uRS.py:52-64) --------------------------------- */

/* r_u[b] = user_mask_layer(user_embedder(user[b]))  (influentialRS.py:180). */
int irs_pif(irs_ctx *ctx, const int64_t *dev_user, int32_t B, float *dev_r_u, void *stream);

/* Full decoder over B sequences.
 *  dev_seq   int64 [B, L] row-major, 1-based item ids, 0 = pad (not modified)
 *  dev_user  int64 [B] (ignored for IRS_MASK_CAUSAL, may be NULL)
 *  dev_x     float [B, L, d] out, may be NULL
 *  dev_pos   int32 [B] row to extract per sequence, may be NULL
 *  dev_xrows float [B, d] out: x[b, pos[b], :], may be NULL (with dev_pos)
 *  dev_r_u   float [B] out, may be NULL */
int irs_decode(irs_ctx *ctx, const int64_t *dev_seq, const int64_t *dev_user, int32_t B, float *dev_x,
               const int32_t *dev_pos, float *dev_xrows, float *dev_r_u, void *stream);

/* ---- scoring against the catalog shard (replaces `project`,
 *      influentialRS.py:83/214, uRS.py:45/68, and the selections on it) ---
 * Exact score of row m and local item j:
 *   e = fmaf(x[d-1], W[j][d-1], ... fmaf(x[0], W[j][0], b[j]))   (float32, k ascending)
 * identical bit for bit to oracle/oracle_score.c. */

/* top-k per row (replaces softmax + topk(100), influentialRS.py:418-421; the
 * softmax is monotone, so ids follow the logits).
 *  dev_xrows float [M, d]
 *  dev_val   float [M, k] out, exact scores, descending
 *  dev_ids0  int64 [M, k] out, global 0-based ids (-1 where the shard has < k items)
 *  dev_status int32 [M] out, IRS_ROW_* bits */
int irs_score_topk(irs_ctx *ctx, const float *dev_xrows, int32_t M, int32_t k, int32_t sweep, float *dev_val,
                   int64_t *dev_ids0, int32_t *dev_status, void *stream);
/* The same call for rows that are the PREVIOUS irs_score_topk[_carry] call's rows one path-search step later (same M, k, IRS_SWEEP_BF16):
 * the pre-pass over the catalog sample and the per-row threshold selection are skipped and the previous call's emission thresholds
 * reused (refreshed every IRS_THR_CARRY-th call, default 8); irs_generate_paths[_sharded] do this between their own steps.  Results are
 * exact whatever the rows are: a threshold that no longer fits is detected by the same validation as always and that row takes the
 * exhaustive path (IRS_ROW_FALLBACK) -- rows unrelated to the previous call's only cost time. */
int irs_score_topk_carry(irs_ctx *ctx, const float *dev_xrows, int32_t M, int32_t k, int32_t sweep, float *dev_val,
                         int64_t *dev_ids0, int32_t *dev_status, void *stream);

/* Exact scores at chosen items (replaces prob_dict[j][end][item-1],
 * evaluator.py:203-205, and the label lookup of influentialRS.py:386-388).
 *  dev_ids0 int64 [M, g] global 0-based ids; entries outside this shard (or <0)
 *  produce -inf so that an elementwise max over shards assembles the answer. */
int irs_score_gather(irs_ctx *ctx, const float *dev_xrows, int32_t M, const int64_t *dev_ids0, int32_t g,
                     float *dev_out, void *stream);

/* count[m] = #{ local j not in excl[m] : (e_j, j) ranks before (ref_score[m], ref_id0[m]) }
 * (replaces sort + history filter + nonzero, influentialRS.py:375-389,
 * evaluator.py:121-131,266-286; rank = 1 + sum of count over shards).
 *  dev_excl_ids0 int64 [M, n_excl] global 0-based ids, -1 = unused slot; duplicates allowed. */
int irs_score_count_before(irs_ctx *ctx, const float *dev_xrows, int32_t M, const float *dev_ref_score,
                           const int64_t *dev_ref_id0, const int64_t *dev_excl_ids0, int32_t n_excl,
                           int64_t *dev_count, void *stream);

/* Dense logits of the shard: out[m, j] for j in [0, n_local) with leading
 * dimension ld (>= n_local); the API-compatible `forward()` output
 * (influentialRS.py:214).  HBM-write bound by construction. */
int irs_score_dense(irs_ctx *ctx, const float *dev_xrows, int32_t M, float *dev_out, int64_t ld, void *stream);

/* Row-wise (max, sum exp(e - max)) over the shard (replaces Softmax /
 * LogSoftmax over N, influentialRS.py:418, evaluator.py:195, and
 * CrossEntropyLoss, evaluator.py:321).  Combine shards on the host side
 * (max of maxes, rescaled sum).  max is the maximum of the shard's chain
 * scores, bit for bit; the sum is a float32 sum in no fixed order. */
int irs_score_lse(irs_ctx *ctx, const float *dev_xrows, int32_t M, float *dev_max, float *dev_sumexp, void *stream);

/* irs_score_topk and irs_score_lse of the same rows out of ONE call: what a beam-search step needs (candidates +
 * the log-softmax normaliser, influentialRS.py:418-421 with LogSoftmax instead of Softmax).  On the swept path
 * with IRS_SWEEP_BF16 the threshold still comes from the bf16 pre-pass, but candidates and (max, sum exp) come
 * out of a single pass over the float32 catalog; results equal the two separate calls' (ids and values bit for
 * bit; the pair (max, sum) to float32 rounding). */
int irs_score_topk_lse(irs_ctx *ctx, const float *dev_xrows, int32_t M, int32_t k, int32_t sweep, float *dev_val,
                       int64_t *dev_ids0, int32_t *dev_status, float *dev_max, float *dev_sumexp, void *stream);

/* Training side: CrossEntropyLoss(project(x)[valid], label - 1) of IRSNN.train_batch /
 * get_loss_on_eval_data (influentialRS.py:252-310) and Evaluator.train_batch (evaluator.py:53-92) WITHOUT the
 * [M, n_item] logits the reference materialises.  One device holds the whole catalog (IRS_E_UNSUPPORTED otherwise; an item-sharded
 * catalog: irs_ce_forward_sharded / irs_ce_backward_sharded, multi-GPU section).  project.weight / bias are
 * read where they were bound: an optimizer step that updates them in place needs no re-finalisation for these two.
 * They do mark the context's derived catalog (bf16 copy, filter norms) as possibly stale: the entry points that
 * filter through it (irs_score_topk / _topk_lse with IRS_SWEEP_BF16, irs_generate_paths, irs_beam_search) return
 * IRS_E_STATE until irs_finalize_weights has run again.
 *  irs_ce_forward:  dev_labels0 int64 [M] 0-based, -1 = row ignored (a pad target);
 *                   dev_lse float [M] = log sum_j exp(logit_mj); dev_label_score float [M];
 *                   dev_loss double [3] = { sum over valid rows of (lse - label score), number of valid rows,
 *                   number of labels >= n_item (nn.CrossEntropyLoss raises on those; they count in neither sum) }.
 *  irs_ce_grad_logits: dL/dlogits of rows [0, M) (a chunk the caller sizes: M x ld floats), written ONCE by the
 *                   fp32-MFMA sweep's epilogue: scale * (exp(logit - lse) - [item == label]); ignored rows 0.
 *                   The caller finishes with two plain GEMMs (dX = G W, dW = G^T X) and a column sum (db). */
int irs_ce_forward(irs_ctx *ctx, const float *dev_xrows, const int64_t *dev_labels0, int32_t M, float *dev_lse,
                   float *dev_label_score, double *dev_loss, void *stream);
int irs_ce_grad_logits(irs_ctx *ctx, const float *dev_xrows, const int64_t *dev_labels0, const float *dev_lse, int32_t M,
                       float scale, float *dev_out, int64_t ld, void *stream);

/* The whole backward of projection + cross entropy WITHOUT dL/dlogits (opt-in; replaces the autograd of nn.Linear +
 * nn.CrossEntropyLoss as the reference runs it in IRSNN.train_batch, influentialRS.py:278-310, and Evaluator.train_batch,
 * evaluator.py:53-68 -- and this library's own irs_ce_grad_logits + two GEMMs + column sum per row chunk).  With
 *   G[m][j] = scale * (exp(logit_mj - lse[m]) - [j == label[m]]),   G[m][:] = 0 for ignored rows (label < 0):
 *   dev_dx float [M, d]        = G W              always overwritten; an ignored row is exactly zero
 *   dev_dw float [n_local, d]  (+)= G^T X         overwritten (accumulate == 0) or added to (accumulate != 0)
 *   dev_db float [n_local]     (+)= colsum G      likewise
 * G is never stored: an item-owned pass (dw, db) and a row-owned pass (dx) each recompute the logits tiles they need on the
 * float32 matrix pipe and consume G from registers -- four GEMM-sized products where the chunked route has three, and no
 * M x n_item traffic.  Labels >= n_item match no column, as in irs_ce_grad_logits.  dev_lse is irs_ce_forward's.
 * `accumulate` lets a caller walk M > max_rows in row blocks and still write dw / db in place, once per block.
 * project.weight / project.bias are read where they were bound (no finalisation, no workspace needed); the derived bf16
 * catalog is marked stale exactly as irs_ce_forward / irs_ce_grad_logits do.  One device holds the whole catalog
 * (IRS_E_UNSUPPORTED otherwise).  M > max_rows, null pointers, rows not 8-byte aligned and a scratch smaller than
 * irs_ce_backward_scratch_bytes(M) (or not 16-byte aligned) return IRS_E_INVALID before any launch.
 * dev_scratch is caller-owned, like the trunk's `saved` arena: it holds the partial outputs of a pass whose owned side has
 * too few tiles to fill the device (small catalogs: dw / db partials per row group; few rows: dx partials per catalog
 * group), never anything of order M x n_item: at most 64 MiB + 4 (M d + n_local d) bytes (not monotone in M: a caller
 * that walks row blocks of several sizes asks for each).  The number of groups is a
 * function of (M, n_local, d) alone and partials are added in group order; there are no float atomics: two identical calls
 * give identical bits.  Nothing is allocated; all work goes on the caller's stream. */
size_t irs_ce_backward_scratch_bytes(const irs_ctx *ctx, int32_t M); /* 0 for an invalid M */
int irs_ce_backward(irs_ctx *ctx, const float *dev_xrows, const int64_t *dev_labels0, const float *dev_lse, int32_t M,
                    float scale, int32_t accumulate, float *dev_dx, float *dev_dw, float *dev_db, void *dev_scratch,
                    size_t scratch_bytes, void *stream);

/* ---- native decoder trunk for training (opt-in; replaces the train-mode nn.TransformerDecoder autograd of
 *      InfluentialNet._decoding_autograd, influentialRS.py:157-200 as called by IRSNN.train_batch :278-310, and of
 *      SampleNet.decoding, uRS.py:52-64, as called by Evaluator.train_batch, evaluator.py:53-92) ------------------
 * irs_train_forward runs embedding -> n_layers post-norm decoder layers over sequences of length L <= max_len (the
 * cross-attention memory is the all-zero [max_len, B, d] tensor of the reference) and keeps in `saved` what
 * irs_train_backward needs; irs_train_backward takes dL/dx and writes every trunk parameter gradient into `grads`.
 * Both read the LIVE bound float32 weights (an optimizer step in place needs no re-binding or re-finalisation; the
 * cross-attention constant is recomputed from multihead_attn.in_proj_bias on every call).  Neither needs
 * irs_finalize_weights or a workspace; they do not touch the inference state.
 *  dev_seq int64 [B, L] 1-based ids, 0 = pad; dev_user int64 [B] (IRN mask; may be NULL for IRS_MASK_CAUSAL)
 *  p dropout probability in [0, 1), seed the step's 64-bit dropout key; backward takes the same B, L, p, seed and saved
 *  dev_saved >= irs_train_saved_bytes(B, L) bytes, 256-byte aligned: written by the forward, read (never modified
 *            outside its scratch tail) by the backward, so the backward can be repeated with identical results
 *  dev_x_out float [B, L, d] out; dev_dx float [B, L, d] in
 *  dev_grads >= irs_train_grad_bytes() bytes, 256-byte aligned, fully overwritten: the gradient of state_dict key
 *            `name` starts at float offset irs_train_grad_offset(name) (same names as irs_bind_weight; -1 = not a trunk
 *            parameter).  Row 0 of the embedding gradient (padding_idx) is 0.  multihead_attn.in_proj_weight and
 *            multihead_attn.in_proj_bias[0 : 2d] get exact zeros: with a zero memory they cannot change any output.
 * Dropout (train-mode torch sites): masks come from Philox4x32-10 with key {lo32(seed), hi32(seed)}; element e of
 * (site, layer) is word (e & 3) of the block for counter {lo32(e >> 2), hi32(e >> 2), layer, site} and is kept iff
 * (word >> 8) >= ceil(p * 2^24); kept values are scaled by 1 / (1 - p).  Sites and flat element indices (m = b L + i):
 *   0 embedding            m d + c            (layer 0)
 *   1 self-attention probs ((b H + h) L + i) L + j
 *   2 dropout1             m d + c
 *   3 cross-attention probs ((b H + h) L + i) max_len + j
 *   4 dropout2             m d + c
 *   5 feed-forward hidden  m ffn_dim + f
 *   6 dropout3             m d + c
 * Gradients are reduced in a fixed order: two identical calls give identical bits.  B * L <= IRS_TRAIN_MAX_TOKENS. */
#define IRS_TRAIN_MAX_TOKENS (1 << 22)
size_t irs_train_saved_bytes(const irs_ctx *ctx, int32_t B, int32_t L); /* 0 for an invalid shape */
size_t irs_train_grad_bytes(const irs_ctx *ctx);
int64_t irs_train_grad_offset(const irs_ctx *ctx, const char *name);
int irs_train_forward(irs_ctx *ctx, const int64_t *dev_seq, const int64_t *dev_user, int32_t B, int32_t L, float p,
                      uint64_t seed, void *dev_saved, size_t saved_bytes, float *dev_x_out, void *stream);
int irs_train_backward(irs_ctx *ctx, const int64_t *dev_seq, const int64_t *dev_user, int32_t B, int32_t L, float p,
                       uint64_t seed, void *dev_saved, size_t saved_bytes, const float *dev_dx, float *dev_grads,
                       size_t grad_bytes, void *stream);

/* Merge W per-shard top-k lists (after the RCCL all-gather) into
 * the global top-k with the same total order.
 *  dev_val_in float [W, M, k], dev_ids_in int64 [W, M, k] (ids -1 ignored) */
int irs_merge_topk(irs_ctx *ctx, const float *dev_val_in, const int64_t *dev_ids_in, int32_t W, int32_t M, int32_t k,
                   float *dev_val, int64_t *dev_ids0, void *stream);

/* Wire format of a per-shard list for the exchange step (SURVEY 8e budgets 8 bytes per entry): ONE unsigned 64-bit
 * key per entry = (order key of the float32 score << 32) | (0xFFFFFFFF - global id0); 0 = no entry (id -1).
 * Unsigned key order IS the selection order (score descending, id ascending), so a merge is a sort of keys.
 * irs_pack_topk: n = M * k entries -> dev_keys uint64 [n].
 * irs_merge_topk_keys: dev_keys_in uint64 [W, M, k] (what an all-gather / all-to-all of packed lists delivers)
 *                      -> the merged top-k as (dev_val float [M, k], dev_ids0 int64 [M, k]); W * k <= 2048. */
int irs_pack_topk(irs_ctx *ctx, const float *dev_val, const int64_t *dev_ids0, int64_t n, uint64_t *dev_keys, void *stream);
int irs_merge_topk_keys(irs_ctx *ctx, const uint64_t *dev_keys_in, int32_t W, int32_t M, int32_t k, float *dev_val,
                        int64_t *dev_ids0, void *stream);

/* ---- evaluation batch construction on the device (replaces the per-user Python of
 *      DataProvider.get_random_evaluate_data, data_provider.py:398-449, and
 *      DataLoaderEvalIRS._collate_fn, data_provider.py:591-617) -------------
 * User b's events are dev_items[dev_offsets[b] .. dev_offsets[b+1]) (1-based ids, oldest first).
 *   label[b]  = the last event; history = all events before it; raw window = its last raw_len items
 *   target[b] = dev_targets_in[b] when given, else a uniformly random member of [1, n_item] (or of
 *               dev_pool[0 .. n_pool), the reference's `popular_item` restriction) that is absent from the raw
 *               window -- device counter RNG keyed by (seed, b): distributional parity with random.sample
 *   seq[b]    = [0 .. 0, last (L - gap_len - 1) raw items, gap_len zeros, target],  L = max_len
 *  dev_seq int64 [B, L], dev_target / dev_label int64 [B] out
 *  dev_raw int64 [B, raw_len] out, right-aligned zero-padded raw windows, dev_raw_n int32 [B] their lengths (both may be NULL)
 *  dev_status int32 [B] in/out (may be NULL): IRS_ROW_NO_CANDIDATE is OR-ed in when no target was found
 *               (the catalog or the pool is contained in the raw window); target[b] is then 0
 * A user without events has label 0 and an empty raw window; a user with one event has that label and an empty window.
 * Needs L - gap_len - 1 >= 1 (the reference's slice arithmetic is only meaningful there). */
int irs_build_eval_batch(irs_ctx *ctx, const int64_t *dev_items, const int64_t *dev_offsets, int32_t B, int32_t raw_len,
                         int32_t gap_len, const int64_t *dev_targets_in, const int64_t *dev_pool, int64_t n_pool,
                         uint64_t seed, int64_t *dev_seq, int64_t *dev_target, int64_t *dev_label, int64_t *dev_raw,
                         int32_t *dev_raw_n, int32_t *dev_status, void *stream);

/* ---- one step of the persuasion-path search (replaces the per-row body of
 *      IRSNN.get_seq_in_batch, influentialRS.py:419-450) ------------------
 * For each row: drop candidates present in seq[b, :hep[b]+1], take the first
 * survivor (greedy) or draw one of the first sample_k survivors with
 * probability proportional to exp(val) (sample != 0; device counter RNG,
 * distributional parity only), record it in paths[b, step], then grow the
 * window (hep < L-2) or shift it left keeping the target at [L-1].
 *  dev_seq  int64 [B, L] in/out     dev_hep int32 [B] in/out
 *  dev_val  float [B, k], dev_ids0 int64 [B, k]: merged top-k (descending)
 *  dev_paths float [B, path_ld] out (ids stored as float32 like the reference, :407)
 *  dev_status int32 [B] in/out: IRS_ROW_NO_CANDIDATE is OR-ed in
 * The list of a row ends at its first negative id0.  A row without a survivor (IRS_ROW_NO_CANDIDATE) gets
 * paths[b, step] = 0 and keeps its window, its hep and its earlier path entries.  Other rows, other columns of
 * dev_paths, dev_val and dev_ids0 are not written.  step >= path_ld, k < 1, B < 1 and null pointers return
 * IRS_E_INVALID, sample != 0 with sample_k outside [1, IRS_MAX_SAMPLE_K] IRS_E_UNSUPPORTED, all before any launch. */
int irs_path_step(irs_ctx *ctx, int64_t *dev_seq, int32_t *dev_hep, int32_t B, const float *dev_val,
                  const int64_t *dev_ids0, int32_t k, int32_t step, float *dev_paths, int32_t path_ld, int32_t sample,
                  int32_t sample_k, uint64_t seed, int32_t *dev_status, void *stream);

/* Whole greedy/sampled path generation on ONE device holding the full catalog
 * (world == 1): max_path_len x { decode, top-k, path step } enqueued on the
 * stream; with use_graph != 0 one step is captured once into a hipGraph and
 * replayed (while a profiling family is enabled, irs_prof_enable, every search
 * loop runs on the stream and records its brackets: same paths and status).
 * dev_seq is the working window (modified); dev_hep int32 [B]
 * initial history end positions (L - gap_len - 2, per row). */
int irs_generate_paths(irs_ctx *ctx, int64_t *dev_seq, const int64_t *dev_user, int32_t *dev_hep, int32_t B,
                       int32_t max_path_len, int32_t k, int32_t sweep, int32_t sample, int32_t sample_k,
                       uint64_t seed, int32_t use_graph, float *dev_paths, int32_t *dev_status, void *stream);

/* irs_generate_paths that stops where it has arrived (the reference never does: "the tail is zeroed afterwards",
 * influentialRS.py:459-467, after every user has been decoded and scored max_path_len times).  A user's target is
 * seq[b][L-1]; the user is FINISHED after the first step whose chosen item equals it.  dev_paths [B, max_path_len] holds the
 * chosen items up to and including the target and exact 0.0f after it: what irs_generate_paths followed by the reference's
 * host zeroing produces, id for id.  A user who never reaches its target gets the row irs_generate_paths writes.  dev_status
 * keeps the bits of a row's live steps.
 * The steps run on the caller's stream.  After every check_every-th step (>= 1) the live users are compacted on the device
 * (stable order, an index map back to the caller's rows; compacted seq / user / hep live in the bound workspace, nothing is
 * allocated) and the live count comes to the host in ONE 4-byte asynchronous copy followed by a wait for the stream: that
 * host read per check is the price of deciding the next step's batch size, and the reason this loop is never replayed from a
 * hipGraph (no use_graph).  The following steps decode, score and step the live rows only; the call returns as soon as none
 * is left.  Between two checks a finished user may still be stepped; its path tail stays zero.  The first step after a
 * compaction that removed rows selects its top-k thresholds afresh (irs_score_topk, not _carry).
 *  dev_seq / dev_hep: the working state, modified; the rows of FINISHED users are unspecified afterwards (and once rows have
 *            been removed, the rows of the others stop where the compaction left them): pass a copy.
 *  host_stats int64 [2], HOST memory, may be NULL: { steps_run, row_steps }, row_steps = the sum over the steps run of the
 *            rows decoded in that step (irs_generate_paths: max_path_len and B * max_path_len).
 * Checks, before any launch: those of irs_generate_paths; check_every < 1 -> IRS_E_INVALID; world != 1 and
 * max_path_len > 64 (the staging rows of the workspace) -> IRS_E_UNSUPPORTED.
 * On any other error (a HIP error inside the loop) the call returns at once: host_stats is not written and dev_paths, dev_status,
 * dev_seq and dev_hep hold the steps enqueued so far -- treat all of them as unspecified.
 * sample != 0 is allowed and deterministic (two identical calls give identical paths), but a user's draws are NOT those of
 * irs_generate_paths for the same seed: the counter RNG is keyed by the launch row, and compaction changes launch rows.
 * Sampled mode is distribution-level parity either way. */
int irs_generate_paths_until(irs_ctx *ctx, int64_t *dev_seq, const int64_t *dev_user, int32_t *dev_hep, int32_t B,
                             int32_t max_path_len, int32_t k, int32_t sweep, int32_t sample, int32_t sample_k, uint64_t seed,
                             int32_t check_every, float *dev_paths, int32_t *dev_status, int64_t *host_stats, void *stream);

/* ---- beam search over persuasion paths (BUILD-DEFINED: the reference has no beam
 *      search -- SURVEY fact 4; BASELINE.json config 5).  Beam width W <= 32, path
 *      length P <= 64.  W == 1 is the greedy search of irs_generate_paths id for id, for every row that has a
 *      candidate at every step.  The two differ on a row that runs out of candidates (IRS_ROW_NO_CANDIDATE on both
 *      sides; the reference raises IndexError there, so nothing downstream may rely on either): irs_path_step /
 *      irs_generate_paths keep the earlier path entries and write 0 at the failed step, window and hep unchanged;
 *      the beam step turns the only beam into a dead beam (below): the whole path is zeroed and its score is -inf.
 * One step for B users x W beams given each beam row's merged top-k (descending) and,
 * for W > 1, its row-wise (max, sum exp) over the whole catalog:
 *   candidates = first W window-survivors of every live beam, scored
 *   cum + (val - max - log(sumexp)); best W by (score desc, parent asc, rank asc) survive.
 * State is ping-ponged: *_in -> *_out ([B, W, ...] row-major; cum = -inf marks a dead beam).
 * A beam's list ends at its first negative id0.  Dead input beams contribute nothing, whatever their lists hold.
 * When a user has fewer than W candidates in all, its trailing output beams are dead: cum = -inf, an all-zero path,
 * and the window and hep of that user's INPUT beam 0 (a well-formed window to decode; never selected again).
 * A live output beam copies paths_in[parent, 0 .. step) and writes the item at [step] and 0 after it, so whatever
 * paths_in holds at and beyond `step` is dropped.
 * dev_status int32 [B] in/out: IRS_ROW_NO_CANDIDATE is OR-ed into a user's word when ANY live input beam of that user
 * has no survivor, even if the user's other beams still fill all W output beams; a dead input beam never sets it.
 * W < 1, k < 1, step >= P, null pointers and W > 1 without dev_lse_max / dev_lse_sum return IRS_E_INVALID, W > 32
 * IRS_E_UNSUPPORTED, all before any launch. */
int irs_beam_step(irs_ctx *ctx, const int64_t *dev_seq_in, const int32_t *dev_hep_in, const double *dev_cum_in,
                  const float *dev_paths_in, const float *dev_val, const int64_t *dev_ids0, const float *dev_lse_max,
                  const float *dev_lse_sum, int32_t B, int32_t W, int32_t k, int32_t step, int32_t P,
                  int64_t *dev_seq_out, int32_t *dev_hep_out, double *dev_cum_out, float *dev_paths_out,
                  int32_t *dev_status, void *stream);

/* Whole beam search on ONE device holding the full catalog: P x { decode B*W windows, top-k,
 * log-sum-exp, beam step } on the stream; use_graph != 0 captures a two-step hipGraph once and
 * replays it.  Needs max_seqs >= B*W and max_rows >= B*W.
 *  dev_seq0 int64 [B, L], dev_user int64 [B], dev_hep0 int32 [B]  (not modified)
 *  dev_paths float [B, W, P] out (beam 0 = best), dev_scores double [B, W] out,
 *  dev_seq_final int64 [B, W, L] out (may be NULL), dev_status int32 [B] out */
int irs_beam_search(irs_ctx *ctx, const int64_t *dev_seq0, const int64_t *dev_user, const int32_t *dev_hep0, int32_t B,
                    int32_t W, int32_t P, int32_t k, int32_t sweep, int32_t use_graph, float *dev_paths,
                    double *dev_scores, int64_t *dev_seq_final, int32_t *dev_status, void *stream);

/* ---- beam search with an end symbol (BUILD-DEFINED like the beam search itself; W == 1 is pinned to the reference through
 *      irs_generate_paths_until).  The end symbol of a window is its target, seq[L-1].  A beam that has just chosen it is
 *      FINISHED (fin = 1): it is not expanded again and competes with its final score.  A user is DONE once nothing is left
 *      to decide for it; done users are skipped by the step and retired by the loop. */
#define IRS_BEAM_STOP_ALL 0  /* done: no output beam is both live (cum > -inf) and unfinished */
#define IRS_BEAM_STOP_BEST 1 /* done also as soon as output beam 0 is finished */
/* irs_beam_step with the flags: per beam dev_fin_in / dev_fin_out int32 [B, W], per user dev_done int32 [B] in/out.
 * A user whose done is 0 on entry:
 *   a live unfinished beam (cum > -inf, fin 0) contributes its first W window-survivors exactly as in irs_beam_step: score
 *     cum + (val - max - log(sumexp)), index parent * W + rank;
 *   a finished beam (fin 1) contributes ONE candidate, itself: score cum, unchanged, index parent * W + 0.  Its rows of
 *     dev_val / dev_ids0 / dev_lse_* are never read (NaNs and negative ids there do not matter) and it never sets
 *     IRS_ROW_NO_CANDIDATE.  (fin 1 with cum -inf is not a state the step produces: such a beam contributes nothing.)
 *   the best W candidates by (score desc, index asc) become the output beams.  A surviving finished beam is copied whole:
 *     window, hep, cum, all P path entries, fin 1.  A new beam is built as in irs_beam_step and gets fin 1 exactly when its
 *     item equals the PARENT window's seq[L-1].  Dead output beams are irs_beam_step's, with fin 0.
 *   done becomes 1 under the stop rule above, else 0.
 * A user whose done is 1 on entry: all W beams are copied from in to out unchanged (window, hep, cum, P path entries, fin);
 *   status and done are not written.  The result of a search therefore does not depend on how often the host looks.
 * IRS_BEAM_STOP_BEST is sound because a step adds a log-probability <= 0 to an unfinished beam and a finished beam 0 wins
 * every tie by index (it re-enters as index 0): later steps could only lower the others.  Float caveat: val, max and sumexp
 * are float32 results of separate reductions; where max is not the exact maximum of the scores val was taken from, an
 * increment can exceed 0 by an ulp, so ALL and BEST may differ for an unfinished beam within that ulp of beam 0.
 * With every fin_in 0, done 0 and no chosen item equal to its target the outputs equal irs_beam_step's bit for bit (fin_out
 * and done 0); with W == 1 the path is irs_generate_paths_until's: the target, then exact zeros.
 * Checks, before any launch: those of irs_beam_step; null dev_fin_in / dev_fin_out / dev_done, stop_rule outside {0, 1} ->
 * IRS_E_INVALID.  Like irs_beam_step it works on the caller's lists, whatever shard the context holds. */
int irs_beam_step_until(irs_ctx *ctx, const int64_t *dev_seq_in, const int32_t *dev_hep_in, const double *dev_cum_in,
                        const float *dev_paths_in, const int32_t *dev_fin_in, const float *dev_val, const int64_t *dev_ids0,
                        const float *dev_lse_max, const float *dev_lse_sum, int32_t B, int32_t W, int32_t k, int32_t step,
                        int32_t P, int32_t stop_rule, int64_t *dev_seq_out, int32_t *dev_hep_out, double *dev_cum_out,
                        float *dev_paths_out, int32_t *dev_fin_out, int32_t *dev_done, int32_t *dev_status, void *stream);

/* irs_beam_search with the end symbol, on ONE device holding the full catalog: beam init (fin 0, done 0), then per step
 * { decode live * W windows, top-k with the row log-sum-exp, irs_beam_step_until } on the users that are still live.  After
 * every check_every-th step except the last, `done` is scanned on the device and the live count comes to the host in ONE
 * 4-byte asynchronous copy followed by a wait for the stream (the stream drains once per check); when users are done, their
 * beams are written to the caller's rows and the live users are compacted (stable order, an index map back to the caller's
 * rows, never in place: into the step's free input set of the workspace).  The call returns when nobody is left; after the
 * last step the remaining users are written out through the map.  Every caller row is written exactly once.  The loop is
 * never replayed from a hipGraph (the batch size of a step is decided on the host: no use_graph), and it leaves the
 * captured steps of the other loops valid.
 *  inputs as irs_beam_search; dev_paths float [B, W, P], dev_scores double [B, W] out (beam 0 = best; W == 1 takes no
 *  log-sum-exp, as in irs_beam_search: the one score is then a sum of raw scores, not of log-probabilities, and may be > 0);
 *  dev_fin int32 [B, W] out, may be NULL; dev_seq_final int64 [B, W, L] out, may be NULL; dev_status int32 [B] out;
 *  host_stats int64 [2], HOST memory, may be NULL: { steps_run, window_steps }, window_steps = the sum over the steps run
 *            of the live * W windows decoded in that step (irs_beam_search: P and B * W * P).
 * Checks, before any launch: those of irs_beam_search; stop_rule outside {0, 1} and check_every < 1 -> IRS_E_INVALID;
 * world != 1 -> IRS_E_UNSUPPORTED.  A live count outside [0, live] returns IRS_E_STATE without launching anything further.
 * On a HIP error inside the loop the call returns at once: host_stats is not written, the outputs are unspecified. */
int irs_beam_search_until(irs_ctx *ctx, const int64_t *dev_seq0, const int64_t *dev_user, const int32_t *dev_hep0, int32_t B,
                          int32_t W, int32_t P, int32_t k, int32_t sweep, int32_t stop_rule, int32_t check_every,
                          float *dev_paths, double *dev_scores, int32_t *dev_fin, int64_t *dev_seq_final,
                          int32_t *dev_status, int64_t *host_stats, void *stream);

/* ---- exact candidates when the window hides the top-k (opt-in; BUILD-DEFINED: the reference raises IndexError at
 *      influentialRS.py:429 for one user, and has no beam search to starve) -------------------------------------------
 * Every search step chooses among the k best items of the catalog after dropping those in the row's window
 * seq[m, 0 .. hep[m]]; nothing guarantees that any of them survives.  irs_topk_ensure_survivors repairs such rows
 * exactly, so that a step on its lists returns what the same step would return with k = n_item.
 * A row's list is val[m, 0 .. k) / ids0[m, 0 .. k); it ends at the first negative id.  A SURVIVOR is an entry whose item
 * ids0 + 1 does not occur in seq[m, 0 .. hep[m]] (the path step's own test: positions beyond hep[m] do not count).  A row
 * is STARVED when its list has k valid entries (a list that ended early already is the whole catalog), fewer than `want`
 * of them survive, and the row is not skipped: cum[m] == -inf (a dead beam), fin[m] != 0 (a finished beam) or
 * done[m / rows_per_status] != 0 (a finished user) skip it; each of the three pointers may be NULL.
 * For the starved rows only, the exact best items of the whole catalog outside the window are computed -- float32 chain of
 * irs_score_topk bit for bit, the library's total order -- and the list is rewritten: with n = min(want, catalog items
 * outside the window), entries [0, n) are those items with their exact scores, descending; if n < k, entry n is
 * (-inf, -1), so the list ends there; IRS_ROW_RESCUED is OR-ed into dev_status[m / rows_per_status] (several beams of a
 * user may set it).  n == 0 leaves an empty list: the unchanged step then sets IRS_ROW_NO_CANDIDATE, which with this pass
 * means what it says -- no item of the catalog lies outside the window.  Rows that are not starved are not written.
 * Launches: a 4-byte memset, a flag pass (one wave per row) and two kernels that return at once when no row is starved;
 * otherwise one pass over the float32 catalog, cut into item strips, serves all starved rows together (any number of
 * them), and an item is tested against the window only after its score has beaten the row's running threshold.  No float
 * atomics: two identical calls give identical bits.  Nothing is allocated; all work goes on the caller's stream.
 *  dev_xrows float [M, d] the rows the lists were scored from; dev_seq int64 [M, L]; dev_hep int32 [M]
 *  dev_cum double [M], dev_fin int32 [M], dev_done int32 [M / rows_per_status]: may be NULL
 *  dev_val float [M, k], dev_ids0 int64 [M, k], dev_status int32 [M / rows_per_status]: in / out
 *  dev_scratch: caller-owned like irs_ce_backward's, >= irs_survivor_scratch_bytes(M, want) bytes, 16-byte aligned.  It holds
 *            the count and the list of the starved rows and the per-strip keys, never anything of order rows x n_item:
 *            256 + 4 rows (rounded up to 16) + 8 rows strips want bytes, strips = the largest power of two <= min(256,
 *            n_local / 128) (at least 1), halved while strips > 1 and rows x strips x want > 2^21.  Bound: 272 + 4 rows +
 *            8 max(2^21, rows x want) bytes, i.e. 16 MiB + 4 rows until rows x want exceeds 2^21.
 * Checks, all before any launch: null required pointers, M < 1, k outside [1, max_k], want outside [1, min(k, 32)],
 * rows_per_status < 1 or not dividing M, a scratch too small or not 16-byte aligned -> IRS_E_INVALID; world != 1 (the pass
 * needs the whole catalog) -> IRS_E_UNSUPPORTED; weights or workspace unbound -> IRS_E_STATE.
 *
 * irs_bind_survivor_scratch makes the four single-device loops do this themselves (NULL / 0 unbinds; a non-null scratch
 * must be 16-byte aligned).  While a scratch is bound, irs_generate_paths, irs_generate_paths_until, irs_beam_search and
 * irs_beam_search_until enqueue the pass between their top-k and their step, with want = 1 (greedy), sample_k (sampled)
 * or W (beam; the beam loops pass their cum / fin / done), so that their result is what the same loop returns with
 * k = n_item.  In sampled mode a row with at least sample_k survivors is untouched and draws as it does unbound for the
 * same seed; a starved row draws among the exact best sample_k admissible items.  A bound scratch smaller than
 * irs_survivor_scratch_bytes(rows of the call, want) returns IRS_E_INVALID before any launch.  The route where one
 * workgroup ranks and steps a row is not taken while a scratch is bound (top-k, pass and step are separate launches).
 * Binding or unbinding drops the captured steps; a captured step replays the pass like any other launch.  With nothing
 * bound every entry point launches exactly what it launched before this pass existed.
 * The sharded loops return IRS_E_UNSUPPORTED while a scratch is bound: a shard can only rescue a row against its own
 * items, and the exact answer needs the other shards' items outside the window as well. */
size_t irs_survivor_scratch_bytes(const irs_ctx *ctx, int32_t rows, int32_t want); /* 0 for invalid arguments */
int irs_topk_ensure_survivors(irs_ctx *ctx, const float *dev_xrows, const int64_t *dev_seq, const int32_t *dev_hep, int32_t M,
                              int32_t rows_per_status, int32_t k, int32_t want, const double *dev_cum, const int32_t *dev_fin,
                              const int32_t *dev_done, float *dev_val, int64_t *dev_ids0, int32_t *dev_status,
                              void *dev_scratch, size_t scratch_bytes, void *stream);
int irs_bind_survivor_scratch(irs_ctx *ctx, void *dev_scratch, size_t bytes);

/* ---- bound exclusions: never offer an item the user has already seen (opt-in; BUILD-DEFINED: the reference's search filters
 *      only the window, influentialRS.py:423-427, while its ranking metric filters the full raw history, :372-379) -------
 * A context can hold a bound EXCLUSION SET.  While it does, every place that drops "the items in the row's window" drops
 *   the window seq[row, 0 .. hep[row]], the row's user's exclusion list and, if no_repeat is on, the row's own non-zero
 *   path entries paths[row, 0 .. step) (for a beam: the path of the input beam, i.e. of the parent of what it becomes)
 * instead.  Everything else is as documented at the entry points: the order (score desc, id asc), greedy = the first
 * survivor, sampled = the first sample_k survivors, beams = the first W survivors of every live beam, grow / shift of the
 * window, the status bits, and IRS_ROW_NO_CANDIDATE when nothing survives (window, hep and path are then untouched); a
 * finished beam of the until forms still contributes only itself, and its lists are not read.  With exact candidates bound
 * as well (irs_bind_survivor_scratch), a row is starved when fewer than `want` entries of its list survive THIS test, and
 * the pass returns the exact best items outside window + list (+ path).
 *  dev_excl_ids0 int64 [users, n_excl], global 0-based ids, the format of irs_score_count_before's dev_excl_ids0: -1 marks
 *            an unused slot (anywhere), duplicates are allowed, ids >= n_item never match.  n_excl in [0, 4096];
 *            n_excl == 0 with a NULL list is legal together with no_repeat != 0 and means "no_repeat only".
 *  no_repeat != 0 switches the path test on.  It needs the path in one wave: while it is bound, a call with a path length
 *            (irs_path_step: a step index) above 64 returns IRS_E_UNSUPPORTED.
 *  dev_scratch: caller-owned, >= irs_exclusion_scratch_bytes(users, n_excl) bytes = 4 users (rounded up to 16) + 8 users
 *            stride, stride = n_excl rounded up to a power of two (0 for 0); 16-byte aligned.
 * Binding enqueues ONE launch on `stream`, one workgroup per user: the row's valid ids (0 <= id < n_item) are sorted
 * ascending in LDS and written to the scratch, followed by INT64_MAX up to `stride`, with the row's valid count.  The
 * caller's list need not outlive the call; the scratch must stay valid, and untouched, until the unbind.  Every later
 * membership test is a binary search in that sorted row (at most 13 probes), one candidate per lane, 64 per round.
 * irs_bind_exclusions(ctx, NULL, 0, 0, 0, NULL, 0, stream) unbinds.  A second bind replaces the first.  Bind and unbind
 * drop the captured steps of the context, as irs_bind_survivor_scratch does.
 * Which list a row reads: irs_path_step, irs_generate_paths: row b's; irs_beam_step[_until], irs_beam_search[_until]: row /
 * W; irs_topk_ensure_survivors: row / rows_per_status (it has no path argument and honours the list only);
 * irs_generate_paths_until and irs_beam_search_until: the caller's original row, through the compaction map the loops keep
 * -- a user keeps its own list after any number of compactions, and under no_repeat the greedy loop reads the path so far
 * from the caller's dev_paths row through the same map.
 * Refused before any launch: n_excl > 4096 and world != 1 -> IRS_E_UNSUPPORTED (the sharded loops return it too should a
 * binding exist); n_excl < 0, users < 1, a list without n_excl >= 1 or n_excl >= 1 without a list, n_excl == 0 without
 * no_repeat, a scratch that is NULL, too small or not 16-byte aligned -> IRS_E_INVALID.  While bound, a step or loop call
 * with more users than were bound (B; M / rows_per_status) returns IRS_E_INVALID before any launch.
 * The list is honoured by EVERY step and loop entry point while bound, the standalone steps included: unbind before an
 * unrelated search.  The route where one workgroup ranks and steps a row is not taken while bound.  With nothing bound
 * every entry point launches the kernels it launched before exclusions existed, and computes the same bits. */
size_t irs_exclusion_scratch_bytes(const irs_ctx *ctx, int32_t users, int32_t n_excl); /* 0 for invalid arguments */
int irs_bind_exclusions(irs_ctx *ctx, const int64_t *dev_excl_ids0, int32_t users, int32_t n_excl, int32_t no_repeat,
                        void *dev_scratch, size_t bytes, void *stream);

/* ---- offer set: search and recommend inside a bound subset of the catalog (opt-in; BUILD-DEFINED: the reference always offers
 *      the whole catalog) -------------------------------------------------------------------------------------------------
 * An OFFER SET is a strictly ascending array of C distinct 0-based item ids, 1 <= C <= n_item, bound to a context and shared
 * by all rows.  While it is bound, "the catalog" reads "the set" wherever a search or a slate decides what to OFFER:
 *   - the ranked list a step of irs_generate_paths[_until] / irs_beam_search[_until] or a slate of irs_recommend starts from
 *     is the best k items of the set in the library's total order (irs_fkey of the score descending, then id ascending);
 *   - its scores are the exact float32 chain (bias-seeded, k-ascending fma): bit for bit irs_score_gather's value for that
 *     row and item (one corner: a chain that ends at exactly -0 is returned as +0; the order folds the two anyway);
 *   - a list with C < k ends in (-inf, -1) and carries IRS_ROW_FEWER_THAN_K, which every consumer already reads as "the
 *     whole catalog was shown";
 *   - exact candidates (irs_bind_survivor_scratch), irs_recommend's repair and irs_topk_ensure_survivors repair a starved
 *     row FROM THE SET; irs_recommend's count is the number of admissible items of the set, cut at n;
 *   - the arrival rule (irs_set_arrival_rule, irs_arrival_offer) never offers a target that is not in the set, exactly like
 *     an excluded one; a caller who wants the target offerable puts it in the set.
 * What describes the user's MODEL stays a statement about the whole catalog: log-probabilities (irs_recommend's out_lp, the
 * traces' lp_item / lp_target, the lookahead's), the log-sum-exp behind a beam's cumulative score, rank_target of the two
 * traces, and the values the arrival rule compares.  The set restricts offers, not the softmax.  Guide, lookahead,
 * exclusions, no_repeat, both traces, both _until loops and long windows read the list and need nothing else.
 * irs_path_step, irs_beam_step[_until|_linked], irs_recommend_take and the lookahead kernels alone are kernels on the
 * caller's lists: they do not look at the binding.
 *  dev_ids0  int64 [n_ids].  The binding enqueues ONE launch that copies it into the scratch: an entry outside
 *            [0, n_item) or not greater than its predecessor in the caller's array becomes a HOLE (-1), and the number of
 *            holes goes to int32 word 0 of the scratch.  That launch compares integers only, and no later kernel indexes
 *            project.* with anything but a sanitised id: a hole is never scored into a list and never offered.  A set with
 *            holes is not a valid set (its sanitised ids need not ascend): read word 0 once after binding and rebind a
 *            repaired array if it is not 0.  The caller's array may be freed once the launch has run.
 *  dev_scratch  caller-owned, 16-byte aligned, >= irs_offer_set_scratch_bytes(n_ids, rows) = 256 + 8 C_pad (rounded up to
 *            256) + 4 rows C_pad bytes, C_pad = n_ids rounded up to 64: the header, the sanitised ids, and the float32
 *            scores of one PASS of `rows` rows.  The binding takes rows = what `bytes` holds, at most max_rows.  It must stay
 *            valid, and untouched, until the unbind.  Nothing of project.* is copied: the kernels read the weights where
 *            they lie, so an in-place weight update followed by irs_finalize_weights needs no rebinding.
 * irs_bind_offer_set(ctx, NULL, 0, NULL, 0) unbinds.  A second bind replaces the first.  Bind and unbind drop the
 * captured steps of the context.  Refused before any launch: world != 1 -> IRS_E_UNSUPPORTED (the sharded loops return it too
 * should a binding exist); an array without n_ids >= 1, n_ids outside [1, n_item], a scratch that is NULL, too small for one
 * row or not 16-byte aligned -> IRS_E_INVALID.  While bound, a loop or irs_recommend call with more rows (B; B * W) than
 * one pass holds returns IRS_E_INVALID before any launch, and the route where one workgroup ranks and steps a row is not
 * taken.  With nothing bound every entry point launches exactly what it launched before offer sets existed.
 * irs_score_topk_offer is the ranking alone: dev_val / dev_ids0 [M, k] and dev_status [M] in irs_score_topk's format, k in
 * [1, max_k], M in [1, max_rows]; it walks M in passes of the bound rows (two launches per pass: the scores on float32 MFMAs,
 * one selection workgroup per row).  No float atomics: two identical calls give identical bits.  IRS_E_STATE with no set
 * bound.
 * Neither entry point takes a stream, like irs_recommend: the work is enqueued on the null stream and the call returns without
 * waiting, so the scratch and the outputs are complete in null-stream order.  Blocking streams are ordered against it by the
 * runtime; a non-blocking stream needs an event on either side; not for use inside a stream capture.  Inside the loops the
 * same launchers run on the loop's stream, captured or not.
 * irs_score_topk_offer checks its arguments before the context's readiness: a NULL row pointer, M outside [1, max_rows], k
 * outside [1, max_k] or a NULL output -> IRS_E_INVALID; then weights / workspace, then the binding -> IRS_E_STATE. */
size_t irs_offer_set_scratch_bytes(const irs_ctx *ctx, int64_t n_ids, int32_t rows); /* 0 for invalid arguments */
int irs_bind_offer_set(irs_ctx *ctx, const int64_t *dev_ids0, int64_t n_ids, void *dev_scratch, size_t bytes);
int irs_score_topk_offer(irs_ctx *ctx, const float *dev_xrows, int32_t M, int32_t k, float *dev_val, int64_t *dev_ids0,
                         int32_t *dev_status);

/* ---- recommend: the exact top-n unseen items of every row (opt-in; replaces sort + history filter + cut of top_k_items,
 *      IRSNN.get_accuracy_metrics_in_batch, influentialRS.py:375-383; the baselines' predict_next(seqs, users, top_k, use_h),
 *      sas.py:357-388; the list Rec2Inf's get_path is built on, main_baselines.py:104) ---------------------------------------
 * For row m, a catalog item j (0-based global id) is ADMISSIBLE when both hold:
 *   item j + 1 does not occur in seq[m, 0 .. hep[m]] -- the path step's own test; dev_seq == NULL, or hep[m] < 0, is an empty window;
 *   if an exclusion set is bound (irs_bind_exclusions), j is not in the list of bound user m.  A bound no_repeat has nothing to
 *   read here -- there is no path -- and is ignored.
 * The row's SLATE is the best n admissible items of the whole catalog in the library's total order (score descending, id
 * ascending); scores are the exact float32 chain of irs_score_topk, bit for bit.  Per row:
 *   count[m] = min(n, admissible items of the catalog); entries [count, n) are (-inf, -1), and lp = -inf there;
 *   lp[m, i] = (float)((double)val - ((double)max + log((double)sumexp))): the expression the path trace stores, so a slate's
 *   log-probabilities equal the trace's.
 * irs_recommend_take is the kernel alone, on the caller's lists: a list val[m, 0 .. k) / ids0[m, 0 .. k) ends at its first negative
 *   id, and its first n admissible entries are copied in order.  It works on whatever shard the context holds, as irs_beam_step
 *   does, needs neither weights nor workspace, and writes nothing but its four outputs.  One wave per row, 64 entries per round
 *   (one per lane), the window held once per wave in LDS; no scratch, no atomics.
 *    dev_seq int64 [M, L] / dev_hep int32 [M] (both NULL: no window); dev_val float [M, k], dev_ids0 int64 [M, k]
 *    dev_lse_max / dev_lse_sum float [M]: the row's (max, sum exp) -- irs_score_lse / irs_score_topk_lse; NULL with out_lp NULL
 *    out_val float [M, n], out_ids0 int64 [M, n], out_lp float [M, n] (may be NULL), out_count int32 [M]
 * irs_recommend is the whole call on ONE device holding the catalog:
 *   1. irs_score_topk_lse of the rows at list length k into the scratch (out_lp NULL: irs_score_topk, no log-sum-exp);
 *   2. the exact repair of SHORT rows -- a list that shows all k valid entries and fewer than n admissible ones -- with want = n:
 *      the flag, strips and merge launches of irs_topk_ensure_survivors, which return at once when no row is short;
 *   3. the take kernel.
 *   The result is what the same call returns with k = n_item.  dev_status gets the top-k's bits, plus IRS_ROW_RESCUED on the
 *   repaired rows; a row with fewer than n admissible items in the whole catalog is reported through out_count, not by a
 *   status bit.
 *   Context state: it counts as one irs_score_topk_lse call of the same rows and nothing more.  It drops no captured step and
 *   reads and writes no search binding except the exclusion set and a bound offer set (irs_bind_offer_set: "the whole catalog"
 *   then reads "the set" in all of the above, and (max, sum exp) come from irs_score_lse over the whole catalog); no search option
 *   refuses it (guide, lookahead, path trace, beam trace, arrival rule, survivor scratch).  Nothing is allocated,
 *   irs_workspace_bytes does not change.  No float atomics: two identical calls give identical bits in val, ids0, count and
 *   status; lp inherits the unordered float32 sum of irs_score_lse.
 *    dev_scratch: caller-owned, >= irs_recommend_scratch_bytes(M, n, k) bytes, 16-byte aligned: the ranked lists (ids, then
 *            values: 12 M k bytes), the (max, sum exp) pairs, M empty windows for a call without dev_seq, and irs_survivor_scratch_bytes'
 *            layout for want = n (not monotone in M: a caller that walks row blocks of several sizes asks for each).
 *    Without dev_seq and without a bound list every entry is admissible and the repair is not launched; without dev_seq and
 *    with a list it runs on empty windows (one 4 M-byte memset more).
 * Checks, all before any launch: null required pointers (one of dev_seq / dev_hep without the other), M < 1, M > max_rows, k
 * outside [1, max_k], n outside [1, min(k, IRS_MAX_RECOMMEND)], out_lp without dev_lse_max / dev_lse_sum (take), a scratch too
 * small or not 16-byte aligned, more rows than the users of a bound exclusion LIST (a binding of no_repeat alone holds nothing
 * this call reads: it is ignored, its user count included) -> IRS_E_INVALID; world != 1 (irs_recommend only) ->
 * IRS_E_UNSUPPORTED; weights, derived weights or workspace unbound (irs_recommend only) -> IRS_E_STATE.
 * Neither entry point takes a stream.  All their work is ENQUEUED ON THE NULL STREAM (the legacy default stream) and the call
 * returns without waiting, like every entry point that takes one: the outputs are complete in null-stream order.  A caller that
 * works on the null stream -- torch's default -- needs nothing more.  A blocking stream is ordered against the null stream by the
 * runtime in both directions.  A stream created non-blocking is not: its owner puts an event between the work that produced the
 * inputs and this call, and another between this call and whatever reads the outputs (the Python engine does, with
 * wait_stream both ways; no host wait).  Not for use inside a stream capture.
 * IRS_MAX_RECOMMEND: the strip selection of the repair holds 512 keys and compacts to `want` whenever more than 256 are held. */
#define IRS_MAX_RECOMMEND 128
size_t irs_recommend_scratch_bytes(const irs_ctx *ctx, int32_t rows, int32_t n, int32_t k); /* 0 for invalid arguments */
int irs_recommend_take(irs_ctx *ctx, const int64_t *dev_seq, const int32_t *dev_hep, int32_t M, const float *dev_val,
                       const int64_t *dev_ids0, int32_t k, const float *dev_lse_max, const float *dev_lse_sum, int32_t n,
                       float *out_val, int64_t *out_ids0, float *out_lp, int32_t *out_count);
int irs_recommend(irs_ctx *ctx, const float *dev_xrows, const int64_t *dev_seq, const int32_t *dev_hep, int32_t M, int32_t n,
                  int32_t k, int32_t sweep, float *out_val, int64_t *out_ids0, float *out_lp, int32_t *out_count,
                  int32_t *dev_status, void *dev_scratch, size_t scratch_bytes);

/* ---- path trace: how the target stands at every step of a greedy / sampled search (opt-in; replaces the saved-path round trip
 *      through Evaluator.get_grad_in_batch -- t_probs, p_probs, IoI, mean path log-probability, evaluator.py:195-205 -- and
 *      get_rr_increase_in_batch's rank before and after, evaluator.py:266-286, with their Python loop of decode + LogSoftmax +
 *      gather per step) ----------------------------------------------------------------------------------------------------
 * For row b at step i, measured BEFORE the step chooses: the window w = seq[b][0 .. hep[b]], the target t = seq[b][L-1], x the
 * decoder row the step scores, e_j the exact float32 chain of x against item j (0-based) of the catalog (top of this section).
 *   lse                = log sum_j exp(e_j) over the WHOLE catalog, window items included: the softmax of influentialRS.py:418.
 *   lp_target[b][i]    = e_{t-1} - lse.
 *   rank_target[b][i]  = 1 + #{ j : j+1 is not a non-pad entry of w, and (e_j, j) ranks before (e_{t-1}, t-1) } in the library's
 *                        total order: score descending, id ascending, -0 folded onto +0.  Duplicates in the window count once; the
 *                        target in its own window still has a rank.  A bound exclusion list and no_repeat do NOT enter the rank:
 *                        it is the rank among what the window leaves, whatever else the step may drop (the rank among what
 *                        they leave as well is rank_adm: "admissible rank" below).
 *   lp_item[b][i]      = e_{c-1} - lse for the item c the step chose; 0 where it chose nothing (IRS_ROW_NO_CANDIDATE).
 *   t == 0 (or t outside the catalog): lp_target = 0 and rank_target = 0.
 * The values are formed as (double)e - ((double)max + log((double)sumexp)) from the float32 pair (max, sumexp = sum exp(e_j -
 * max)) and rounded to float32 once; rank_target is int32.
 * irs_score_target_trace is the sweep alone: ONE pass over the float32 catalog in chain order gives the (max, sumexp) partials
 * (the partial slots of irs_score_lse, reduced in slot order) and the number of items ranked before (e_{t-1}, t-1); e_{t-1} is
 * taken first, with irs_score_gather's arithmetic, and the window correction reads dev_seq / dev_hep where they lie (no [M, L]
 * copy of ids is made; any max_len).  No float atomics (integer ones count): two identical calls give identical bits.
 *  dev_xrows float [M, d], dev_seq int64 [M, L], dev_hep int32 [M]
 *  dev_max / dev_sumexp / dev_target_score float [M] out (target_score -inf without a target), dev_rank int32 [M] out
 *  dev_scratch: caller-owned, >= irs_path_trace_scratch_bytes(M) bytes (16 rows + 16 rows, each of six arrays rounded up to 256),
 *            16-byte aligned.  Null pointers, M outside [1, max_rows], a scratch too small or misaligned -> IRS_E_INVALID; world != 1
 *            -> IRS_E_UNSUPPORTED; all before any launch.
 * irs_bind_path_trace makes the greedy / sampled loops record the three values: dev_lp_item / dev_lp_target float [users, ld],
 * dev_rank_target int32 [users, ld], caller-owned; the scratch (>= irs_path_trace_scratch_bytes(users)) is caller-owned like
 * irs_bind_survivor_scratch's and must stay valid until the unbind; irs_workspace_bytes does not change.  All three arrays NULL
 * unbinds.  While bound:
 *   irs_generate_paths (stream launches and the captured step alike) runs the sweep between its top-k and its step and a record
 *     kernel after the step, and writes all max_path_len columns of rows [0, B); a caller cuts them after the arrival as it cuts
 *     dev_paths.  irs_generate_paths_until zeroes rows [0, B) of the three arrays at entry and writes only the steps up to and
 *     including the one that chose the target, at the caller's row (through its compaction map); a finished user that is still
 *     stepped until the next compaction writes nothing.
 *   the route where one workgroup ranks and steps a row is not taken (as under exclusions);
 *   B > users or max_path_len > ld -> IRS_E_INVALID before any launch;
 *   irs_beam_step[_until], irs_beam_search[_until] and the two _sharded loops return IRS_E_UNSUPPORTED (no trace is carried through
 *     beam state, and a shard sees only its own items); a context with world != 1 refuses the binding itself.
 * Binding and unbinding drop the captured steps; the bound pointers are part of a captured step's key.  With nothing bound every
 * entry point launches exactly what it launched before. */
size_t irs_path_trace_scratch_bytes(const irs_ctx *ctx, int32_t rows); /* 0 for invalid arguments */
int irs_score_target_trace(irs_ctx *ctx, const float *dev_xrows, const int64_t *dev_seq, const int32_t *dev_hep, int32_t M,
                           void *dev_scratch, size_t scratch_bytes, float *dev_max, float *dev_sumexp, float *dev_target_score,
                           int32_t *dev_rank, void *stream);
int irs_bind_path_trace(irs_ctx *ctx, float *dev_lp_item, float *dev_lp_target, int32_t *dev_rank_target, int32_t users, int32_t ld,
                        void *dev_scratch, size_t bytes);

/* ---- beam trace: the path trace of every beam, carried through beam state (opt-in, off by default; BUILD-DEFINED like the beam
 *      search itself; replaces an irs_replay_paths pass over all B * W * P windows behind the search, which decodes every one of
 *      them a second time) ------------------------------------------------------------------------------------------------------
 * A separate binding from the path trace above: what irs_bind_path_trace admits and refuses is unchanged.
 * For output beam j of user b after the last step, and column i < P: the three values are those of the row the beam's ANCESTOR
 * was at step i, measured BEFORE step i chose, with exactly the path trace's definitions -- lse over the whole catalog,
 * lp_target = e_{t-1} - lse, rank_target among what the ancestor's window leaves (exclusions and no_repeat do not enter),
 * lp_item = e_{c-1} - lse for the item c that step appended to this beam -- and its arithmetic: (double)e - ((double)max +
 * log((double)sumexp)) from the float32 results of the trace sweep (irs_score_target_trace) on that step's input row, rounded to
 * float32 once; lp_target and rank_target are 0 when the row has no target.
 *   e_{c-1} is the LIST value the beam step read for the chosen candidate (dev_val / the loop's ranked list); where the survivor
 *     pass rewrote the list (irs_bind_survivor_scratch), it is the rewritten value.
 *   lp_item is NOT the term the step added to the beam's score: the score uses the (max, sumexp) pair of the top-k call, the
 *     trace the sweep's own, and for W == 1 the score takes no log-sum-exp at all (irs_beam_search).
 *   A finished beam (the _until forms) keeps its columns up to and including the step that chose its target; later columns stay
 *     0; when it survives a step it is copied whole, possibly into another slot.  A user that is done on entry to a step is
 *     not written.  A dead output beam (score -inf) reads 0 in every column.
 *   On return the beam order is that of dev_paths / dev_scores.
 * The arrays are the caller's, float dev_lp_item / dev_lp_target [users, W, ld], int32 dev_rank_target [users, W, ld], addressed
 * by the CALLER's user row: irs_beam_search_until goes through its compaction map, and nothing of the trace is compacted.
 *
 * irs_bind_beam_trace binds them (all three NULL unbinds; no launch, no stream).  dev_scratch: caller-owned, >=
 * irs_beam_trace_scratch_bytes(users, W) bytes -- irs_path_trace_scratch_bytes(users * W) plus one link word and one float per
 * beam row, each array rounded up to 256 -- 16-byte aligned, valid until the unbind.  Checks, before anything else: world != 1 ->
 * IRS_E_UNSUPPORTED; the three arrays not all given, W outside [1, 32], users < 1, users * W above max_seqs or max_rows, ld
 * outside [1, 64], a scratch too small or misaligned -> IRS_E_INVALID.  Binding and unbinding drop the captured steps.
 * While bound:
 *   irs_beam_search (stream launches and the two captured ping-pong steps alike) and irs_beam_search_until zero rows [0, B) of
 *     the three arrays at entry and run, per step: decode, top-k (+ lse), the survivor pass if bound, the trace sweep over the
 *     live * W rows of the step's input state, the linked beam step, the carry, the step counter.  Paths, scores, status and fin
 *     are those of the unbound search.  B > users, W different from the bound W, P > ld -> IRS_E_INVALID before any launch.
 *   every other search entry point -- irs_generate_paths[_until], irs_path_step, irs_beam_step[_until] and the two _sharded
 *     loops -- returns IRS_E_UNSUPPORTED with a message that names the binding: it is never silently ignored.
 * With nothing bound every entry point checks and launches exactly what it did before this binding existed.
 *
 * The two kernels alone, so that a loop can be composed from public calls (the step honours and refuses the other bindings as
 * irs_beam_step does -- exclusions honoured; path trace, guide, lookahead refused -- and neither looks at a bound beam trace).
 * Like irs_lookahead_expand / irs_lookahead_choose they are SYNCHRONOUS and take no stream: the kernel is launched on the null
 * stream and the call returns when it has finished; a caller whose inputs were produced on another stream waits for that stream
 * first, and the outputs are complete on return:
 * irs_beam_step_linked is irs_beam_step when dev_fin_in, dev_fin_out and dev_done are all NULL (stop_rule is then ignored), and
 *   irs_beam_step_until when all three are given (one or two of them: IRS_E_INVALID); checks and outputs are theirs.  Besides,
 *   per output beam row b * W + j: dev_link int32 [B, W] and dev_link_val float [B, W] --
 *     IRS_BEAM_LINK_DEAD                      a dead beam                                              (value 0)
 *     p in [0, W)                             a child of input beam p: column `step` is new            (the candidate's list value)
 *     IRS_BEAM_LINK_COPY | p                  input beam p whole: a surviving finished beam, or beam p = j of a done user  (0)
 * irs_beam_trace_carry applies the links to the three arrays IN PLACE, one workgroup per user: every input row is read first
 *   (columns [0, step), all ld columns of a row that is copied whole), then every output slot is written in all ld columns -- the
 *   parent's columns [0, step), then column `step` formed as above from dev_max / dev_sumexp / dev_target_score / dev_rank of the
 *   PARENT's row (the sweep on the step's input state) and dev_link_val of the output row, then zeros; or the parent's whole
 *   row; or zeros.  A slot that is a whole copy of itself is not written.  dev_row_map int32 [B] (may be NULL: the identity):
 *   launch user -> the user row of the three arrays.  No atomics, no float reductions: identical calls give identical bits.
 *   Null pointers, B < 1, W outside [1, 32], ld outside [1, 64], step outside [0, ld) -> IRS_E_INVALID before the launch. */
#define IRS_BEAM_LINK_DEAD (-1)
#define IRS_BEAM_LINK_COPY 256
size_t irs_beam_trace_scratch_bytes(const irs_ctx *ctx, int32_t users, int32_t W); /* 0 for invalid arguments */
int irs_bind_beam_trace(irs_ctx *ctx, float *dev_lp_item, float *dev_lp_target, int32_t *dev_rank_target, int32_t users, int32_t W,
                        int32_t ld, void *dev_scratch, size_t bytes);
int irs_beam_step_linked(irs_ctx *ctx, const int64_t *dev_seq_in, const int32_t *dev_hep_in, const double *dev_cum_in,
                         const float *dev_paths_in, const int32_t *dev_fin_in, const float *dev_val, const int64_t *dev_ids0,
                         const float *dev_lse_max, const float *dev_lse_sum, int32_t B, int32_t W, int32_t k, int32_t step,
                         int32_t P, int32_t stop_rule, int64_t *dev_seq_out, int32_t *dev_hep_out, double *dev_cum_out,
                         float *dev_paths_out, int32_t *dev_fin_out, int32_t *dev_done, int32_t *dev_status, int32_t *dev_link,
                         float *dev_link_val);
int irs_beam_trace_carry(irs_ctx *ctx, const int32_t *dev_link, const float *dev_link_val, const float *dev_max,
                         const float *dev_sumexp, const float *dev_target_score, const int32_t *dev_rank, int32_t B, int32_t W,
                         int32_t step, float *dev_lp_item, float *dev_lp_target, int32_t *dev_rank_target, int32_t ld,
                         const int32_t *dev_row_map);

/* ---- guided choice: the Rec2Inf rule of the greedy path step (opt-in; replaces the Python double loop over users and steps of
 *      the reference's get_path, main_baselines.py:93-121, and its distance cal_fv_dist, utils.py:202-206) ----------------------
 * A context can hold one bound GUIDE: a feature table over the catalog and a candidate count k_c in [1, IRS_MAX_GUIDE_KC].
 * While it does, a greedy path step does this for a row:
 *   1. It walks the row's ranked list exactly as irs_path_step does, with the same admissibility test: the window seq[row, 0 ..
 *      hep[row]], plus the bound exclusion list, plus the path under no_repeat.  The list ends at its first negative id.  The
 *      first min(k_c, available) survivors are collected in rank order.
 *   2. The target is t = seq[row][L-1] (1-based).  t == 0 (or t outside [1, n_item]): the row takes its first survivor, the
 *      greedy choice.  Otherwise it takes the survivor with the smallest distance to t: walking the survivors in rank order, a
 *      later one replaces the current best only if its distance is STRICTLY smaller, so ties go to the better rank; a NaN
 *      distance never replaces anything and is replaced by any distance that is not a NaN (np.argsort(dists)[0]: NaN sorts
 *      last; all NaN: the first survivor).  The target itself gets no preference beyond its distance 0 (the reference gives it
 *      none).  A survivor whose id lies outside [1, n_item] is never looked up and counts as the farthest.
 *   3. No survivor: IRS_ROW_NO_CANDIDATE, paths[row, step] = 0, window and hep untouched, as in irs_path_step.
 *   4. Record, then grow or shift the window: byte for byte what irs_path_step does with its chosen item.
 * Distances (table row i belongs to the 1-based item i: n_item + 1 rows, row 0 is never read -- the reference's fv[i]):
 *   IRS_GUIDE_BINARY  F features, 1 <= F <= IRS_MAX_GUIDE_BITS, packed 32 to a word (feature f = bit f % 32 of word f / 32, the
 *                     bits behind F zero); the distance is the popcount of the XOR over the ceil(F / 32) words (Hamming).
 *   IRS_GUIDE_FLOAT   F float32 features, 1 <= F <= IRS_MAX_GUIDE_FLOATS, row stride F; the distance is the SQUARED Euclidean
 *                     distance as ONE float32 chain, acc = fmaf(t_f - c_f, t_f - c_f, acc), f ascending from 0, acc starting at
 *                     0 (t_f - c_f rounded to float32 once).  The square root is monotone and would only merge neighbours, so it
 *                     is not taken.  The chain order is part of the semantics: chosen ids can be compared exactly.
 * irs_guide_scratch_bytes: binary: the packed table, (n_item + 1) ceil(F / 32) words, rounded up to 256 bytes; float: 0 (the
 *   table is read where it lies); 0 for invalid arguments as well.
 * irs_bind_guide:
 *   IRS_GUIDE_BINARY  dev_table uint8 [n_item + 1][F], nonzero = 1.  ONE launch on `stream` packs it into dev_scratch (16-byte
 *                     aligned, >= irs_guide_scratch_bytes); the caller's table need not outlive that launch, the scratch must
 *                     stay valid, and untouched, until the unbind.
 *   IRS_GUIDE_FLOAT   dev_table float32 [n_item + 1][F], kept BY POINTER: the caller keeps it alive and unchanged until the
 *                     unbind.  dev_scratch / bytes are ignored (NULL / 0).  Rows are read 16 bytes at a time where F % 4 == 0
 *                     and the table is 16-byte aligned.
 *   dev_table == NULL unbinds.  A second bind replaces the first.  Bind and unbind drop the captured steps of the context.
 *   Refused before any launch: a null context, kind not one of the two, F < 1, k_c < 1, k_c > max_k, a binary scratch that is
 *   NULL, too small or misaligned -> IRS_E_INVALID; k_c > IRS_MAX_GUIDE_KC, F beyond the limits above, world != 1 ->
 *   IRS_E_UNSUPPORTED.
 * While bound:
 *   irs_path_step, irs_generate_paths (stream launches and the captured step alike) and irs_generate_paths_until apply the rule;
 *     sample != 0 -> IRS_E_UNSUPPORTED (the rule is deterministic), k < k_c -> IRS_E_INVALID, before any launch;
 *   irs_beam_step[_until], irs_beam_search[_until] and the two _sharded loops return IRS_E_UNSUPPORTED;
 *   exclusions and no_repeat compose through the shared admissibility test; with exact candidates bound as well
 *     (irs_bind_survivor_scratch) the loops ask the survivor pass for want = k_c, so a row with fewer than k_c admissible
 *     entries in its list is repaired to the exact best k_c admissible items (size the scratch for want = k_c);
 *   a bound path trace records the guided choice: lp_item is the chosen item's, found in the step's list as always;
 *   the route where one workgroup ranks and steps a row is not taken (as under exclusions).
 * No atomics: two identical calls give identical bytes.  With nothing bound every entry point launches exactly what it
 * launched before. */
#define IRS_GUIDE_BINARY 1
#define IRS_GUIDE_FLOAT 2
#define IRS_MAX_GUIDE_KC 32       /* the survivor pass's `want` limit */
#define IRS_MAX_GUIDE_BITS 1024   /* features of a binary guide */
#define IRS_MAX_GUIDE_FLOATS 512  /* features of a float guide */
size_t irs_guide_scratch_bytes(const irs_ctx *ctx, int32_t kind, int32_t F);
int irs_bind_guide(irs_ctx *ctx, int32_t kind, const void *dev_table, int32_t F, int32_t k_c, void *dev_scratch, size_t bytes,
                   void *stream);

/* ---- lookahead choice: among the top k_c candidates, the one that moves the target furthest (opt-in; BUILD-DEFINED: the
 *      reference steers with the impressionability mask alone, Rec2Inf with a static feature distance; here the model itself is
 *      asked where the target stands one step after each candidate.  The host-side alternative costs k_c decode round trips per
 *      step) ------------------------------------------------------------------------------------------------------------------
 * A context can hold one bound LOOKAHEAD with a candidate count k_c in [1, IRS_MAX_LOOKAHEAD_KC].  While it does, a greedy step
 * of the loops does this for a live row, behind the top-k, the survivor pass, the trace sweep and the arrival offer and BEFORE
 * the path step:
 *   1. EXPAND.  It walks the row's ranked list exactly as irs_path_step does, with the same admissibility test: the window
 *      seq[row, 0 .. hep[row]], plus the bound exclusion list (looked up through the until loop's row map), plus the path so far
 *      under no_repeat.  The list ends at its first negative id.  The first min(k_c, available) survivors are collected in rank
 *      order.  For survivor j, child row * k_c + j is the parent window after irs_path_step would have chosen that item, byte
 *      for byte: grow (hep < L - 2: the item goes to slot hep + 1, child_hep = hep + 1) or shift (slots 1 .. L - 2 move down by
 *      one, the item goes to slot L - 2, child_hep = hep), the target kept in slot L - 1.  child_user is the parent's user (0
 *      without one), child_target0 the parent's target as a 0-based id, seq[row][L - 1] - 1.  A slot j without a survivor holds
 *      a copy of the parent window with the parent's hep (well-formed to decode), candidate id -1 and candidate value -inf.
 *      cand_ids0 [M, k_c] int64 (0-based) and cand_val [M, k_c] float are the survivors' entries of the list.  A row with
 *      fin != 0 expands as a row without survivors.
 *   2. SCORE.  One rows-only decode of the M k_c child windows at child_hep, then irs_score_lse and irs_score_gather (one id per
 *      row: child_target0) on those rows.  lp[row][j] = (float)((double)ts - ((double)max + log((double)sumexp))), the path
 *      trace's expression, rounded to float32 once; a slot without a candidate reads -inf.  t == 0, or t outside the catalog:
 *      ts is -inf, and so is every lp.
 *   3. CHOOSE.  If the target itself is among the row's candidates it is chosen outright: offering it is the arrival.  Otherwise
 *      the candidates are walked in rank order: a later one replaces the current best only if its lp is STRICTLY greater; a NaN
 *      never replaces anything and is replaced by anything that is not a NaN (the guide's tie rules: ties go to the better rank,
 *      and an all -inf row keeps its first survivor, the greedy choice).  The row's list is then rewritten as irs_arrival_offer
 *      rewrites it: entry 0 becomes (cand_val, cand_ids0) of the chosen candidate -- its ORIGINAL score -- and entry 1 becomes
 *      (-inf, -1) when k > 1.  A row without a survivor is not written (the unchanged path step reports IRS_ROW_NO_CANDIDATE);
 *      a row with fin != 0 is not written.  lp [M, k_c] float32, the values compared, and choice [M] int32 (the chosen slot, -1:
 *      none; -1 for a row with fin != 0) are written for every row, so that every decision can be replayed from arrays.
 *   4. STEP.  The unchanged irs_path_step takes its only survivor and the unchanged trace record finds the chosen item in entry
 *      0; irs_generate_paths_until retires a user whose choice was the target.
 * Consequences: k_c = 1 gives the greedy search id for id; after the step the row's window equals the chosen child's window
 * byte for byte; no atomics, so two identical calls give identical bytes.
 * irs_lookahead_scratch_bytes(ctx, rows, k_c): the caller-owned scratch for `rows` parent rows: the child windows, hep, users
 *   and targets, the child rows [rows k_c, d], max / sumexp / target score, candidate ids and values, lp and choice, every array
 *   rounded up to 256 bytes.  0 for invalid arguments (rows < 1, k_c outside [1, IRS_MAX_LOOKAHEAD_KC]).  irs_workspace_bytes
 *   does not change.
 * irs_bind_lookahead(ctx, k_c, dev_scratch, bytes, dev_rec_item, dev_rec_lp, users, ld):
 *   k_c == 0 unbinds.  dev_scratch: 16-byte aligned, >= irs_lookahead_scratch_bytes(ctx, users, k_c), valid until the unbind.
 *   dev_rec_item int32 [users, ld, k_c] (1-based candidate ids, 0: none) and dev_rec_lp float [users, ld, k_c] are the RECORD;
 *   both may be NULL (they go together).  When given, the choose step of a loop also writes each live row's candidates and lp
 *   at the caller's row (through the until loop's row map) and the step's column (the device step counter), exactly as the
 *   trace record does; irs_generate_paths_until zeroes rows [0, B) of both at entry, so a record is zero behind an arrival.
 *   Bind and unbind drop the captured steps of the context; the binding is part of a captured step's key.
 *   Refused before any launch, each with a message naming irs_bind_lookahead: k_c outside [0, IRS_MAX_LOOKAHEAD_KC], users or
 *   ld < 1, one record pointer without the other, a scratch that is NULL, too small or misaligned -> IRS_E_INVALID; world != 1
 *   -> IRS_E_UNSUPPORTED; a bound guide (irs_bind_guide) -> IRS_E_UNSUPPORTED, and irs_bind_guide refuses the same way while
 *   a lookahead is bound.
 * While bound:
 *   irs_generate_paths (stream launches and the captured step alike) and irs_generate_paths_until apply the rule;
 *     sample != 0 -> IRS_E_UNSUPPORTED; k < k_c, B > users, max_path_len > ld (with a record) -> IRS_E_INVALID; B k_c above
 *     max_seqs or max_rows -> IRS_E_INVALID with both numbers in the message; all before any launch;
 *   irs_beam_step[_until], irs_beam_search[_until] and the two _sharded loops return IRS_E_UNSUPPORTED;
 *   exclusions, no_repeat, the trace and the arrival rule compose as under a guide; with exact candidates bound as well the
 *     loops ask the survivor pass for want = k_c;
 *   the route where one workgroup ranks and steps a row is not taken;
 *   irs_path_step ALONE is unchanged: the rule lives in the loops and in the two entry points below;
 *   irs_decoder_route_last reports the INNER decode (of the children), the last one a step launches.
 * irs_lookahead_expand / irs_lookahead_choose are the two kernels alone, for tests and for replaying a decision from arrays (no
 * binding needed; bound exclusions are honoured as irs_path_step honours them).  Unlike the loops they are SYNCHRONOUS and take
 * no stream: the kernel is launched on the null stream and the call returns when it has finished.  The caller makes sure that
 * the work that produces the inputs has finished (a stream created non-blocking does not wait for the null stream, nor the null
 * stream for it); the outputs are complete on return.  Not for use inside a stream capture.
 *  dev_seq int64 [M, L], dev_hep int32 [M], dev_user int64 [M] (may be NULL on a context whose mask needs no user)
 *  dev_val float [M, k] / dev_ids0 int64 [M, k]: the rows' ranked lists (expand reads them, choose rewrites them)
 *  dev_fin int32 [M] (may be NULL); dev_paths float [users, path_ld] (may be NULL) / step: the path so far under no_repeat, as in
 *            irs_arrival_offer; dev_row_map int32 [M] (may be NULL: the identity): row -> bound user
 *  expand out: dev_child_seq int64 [M k_c, L], dev_child_hep int32 [M k_c], dev_child_user int64 [M k_c], dev_child_target0
 *            int64 [M k_c], dev_cand_ids0 int64 [M, k_c], dev_cand_val float [M, k_c]
 *  choose in: dev_cand_ids0 / dev_cand_val, dev_max / dev_sumexp / dev_target_score float [M, k_c] (of the child rows)
 *  choose out: dev_val / dev_ids0 rewritten, dev_lp float [M, k_c], dev_choice int32 [M]
 * Null pointers, M < 1, k outside [1, max_k], k_c outside [1, min(k, IRS_MAX_LOOKAHEAD_KC)], step < 0 or beyond path_ld, M above
 * the bound exclusion users, no_repeat bound and dev_paths NULL, a NULL dev_user on a context whose mask needs one ->
 * IRS_E_INVALID; world != 1 -> IRS_E_UNSUPPORTED; all before any launch.
 * Both kernels: one wave per row, no LDS, no atomics.  With nothing bound every entry point launches exactly what it launched
 * before. */
#define IRS_MAX_LOOKAHEAD_KC 32
size_t irs_lookahead_scratch_bytes(const irs_ctx *ctx, int32_t rows, int32_t k_c);
int irs_bind_lookahead(irs_ctx *ctx, int32_t k_c, void *dev_scratch, size_t bytes, int32_t *dev_rec_item, float *dev_rec_lp,
                       int32_t users, int32_t ld);
int irs_lookahead_expand(irs_ctx *ctx, const int64_t *dev_seq, const int32_t *dev_hep, const int64_t *dev_user, int32_t M,
                         const float *dev_val, const int64_t *dev_ids0, int32_t k, int32_t k_c, const int32_t *dev_fin,
                         const float *dev_paths, int32_t path_ld, int32_t step, const int32_t *dev_row_map, int64_t *dev_child_seq,
                         int32_t *dev_child_hep, int64_t *dev_child_user, int64_t *dev_child_target0, int64_t *dev_cand_ids0,
                         float *dev_cand_val);
int irs_lookahead_choose(irs_ctx *ctx, const int64_t *dev_seq, int32_t M, int32_t k_c, const int64_t *dev_cand_ids0,
                         const float *dev_cand_val, const float *dev_max, const float *dev_sumexp, const float *dev_target_score,
                         const int32_t *dev_fin, float *dev_val, int64_t *dev_ids0, int32_t k, float *dev_lp, int32_t *dev_choice);

/* ---- sampler: temperature, nucleus and wide top-k draws that can be replayed (opt-in; BUILD-DEFINED: the reference draws among
 *      three survivors at temperature 1 and keeps no record; the stock sampled step, sample != 0, is that rule and stays as it is) --
 * A context can hold one bound SAMPLER (top_k, temperature, top_p).  While it does, a step of the greedy loops does this for a
 * live row, behind the top-k, the survivor pass, the trace sweep and the arrival offer and BEFORE the path step:
 *   1. WALK.  The row's ranked list is walked exactly as irs_path_step walks it, with the same admissibility test: the window
 *      seq[row, 0 .. hep[row]], plus the bound exclusion list, plus the path so far under no_repeat.  The list ends at its first
 *      negative id.  The first n = min(top_k, admissible entries) candidates (v_i, id_i), i = 0 .. n - 1, are kept in list order.
 *   2. WEIGH, in float32, in an order that is fixed for a given n (two calls give the same bits):
 *        w_i = expf((v_i - v_0) * inv_T), inv_T = 1.0f / temperature formed once at the bind; v_i = -inf gives w_i = 0;
 *        S_m = w_0 + ... + w_(m-1), by a scan over the wave;
 *        the SUPPORT m* is the smallest m >= 1 with S_m >= top_p * S_n (the nucleus; top_p = 1 keeps all n);
 *        a row whose v_0 is not finite takes candidate 0 with lq = 0 and support = 1.
 *   3. DRAW.  u = (z >> 40) * 2^-24, z the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * (row_id * 1315423911 + step + 1):
 *      the stock sampled step's expression with the CALLER'S row in place of the launch row -- the until loop's row map, the
 *      identity elsewhere -- and the device step counter, so a captured step draws what a streamed one draws and a compacted row
 *      draws what its user would have drawn in irs_generate_paths.  t = u * S_m*; the chosen index is the smallest i < m* with
 *      S_(i+1) > t, and m* - 1 if there is none.  lq = logf(w_i / S_m*): the chosen candidate's log-probability under the
 *      distribution it was drawn from.
 *      ACCURACY against the same expressions in float64 on the same float32 values: a cumulative share S_m / S_m* is within
 *      5e-5 (two roundings of an argument of magnitude <= 20, expf within 2 ulp, a sum of <= 256 terms, a ratio), so the chosen
 *      index is the float64 one unless u lies that near a share; lq is within 1e-4 max(1, |lq|) of the float64 value.  The bound
 *      is relative only from |lq| = 1 on: the ratio nearest to 1 that float32 holds is 1 - 2^-24, so next to lq = 0 no relative
 *      bound can be met.
 *   4. REWRITE.  The row's list becomes (v_chosen, id_chosen), then (-inf, -1) when k > 1, exactly as irs_arrival_offer writes
 *      it.  The unchanged irs_path_step takes its only survivor, the unchanged trace record finds the chosen item in entry 0, and
 *      irs_generate_paths_until retires a user whose draw was its target.
 * Rows that are not written: a row with fin != 0 (nothing at all, records included); a row the arrival rule has chosen for at
 * this step -- IRS_ROW_OFFERED in its status word, and its list the offer's: the row's target seq[row][L - 1] - 1 in entry 0 and
 * the end mark behind it (the loops' status words keep the bit of an earlier step) -- whose records are u = 0, lq = 0, support = 1;
 * (so in irs_generate_paths, whose status words keep the bit, a LATER step of such a row whose list is by itself the target and
 * the end mark -- k = 1, or a one-entry offer set or repaired list -- is read as offered too: the item chosen is the same, the
 * target, and only the record differs: u = 0, support = 1 where a walk would have recorded the draw);
 * a row without an admissible candidate, whose list is left alone (the step reports IRS_ROW_NO_CANDIDATE) and whose records are 0.
 * The records are optional: dev_rec_u float, dev_rec_lq float, dev_rec_support int32, each [users, ld], written at the caller's
 * row and the step's column (cells outside [users, ld] are not written); irs_generate_paths_until zeroes rows [0, B) of them at
 * entry, so a record is zero behind an arrival.
 * irs_bind_sampler(ctx, top_k, temperature, top_p, dev_rec_u, dev_rec_lq, dev_rec_support, users, ld): top_k == 0 unbinds.
 *   temperature not finite or <= 0, top_p outside (0, 1], a record array with users < 1 or ld < 1 -> IRS_E_INVALID; top_k outside
 *   [1, min(max_k, IRS_MAX_SAMPLER_K)], world != 1, a bound guide or lookahead (which refuse the same way while a sampler is
 *   bound: one choice rule at a time) -> IRS_E_UNSUPPORTED.  Bind and unbind drop the captured steps of the context.
 * While bound:
 *   irs_generate_paths (stream launches and the captured step alike) and irs_generate_paths_until apply the rule; their `seed`
 *     keys the draws.  sample != 0 -> IRS_E_INVALID (two samplers); k < top_k, B > users or max_path_len > ld (with a record)
 *     -> IRS_E_INVALID; top_k > 32 together with a bound survivor scratch -> IRS_E_UNSUPPORTED; all before any launch;
 *   irs_generate_paths_until(check_every) draws, for the same seed, the u of irs_generate_paths bit for bit in every (row,
 *     step).  The choices, and so the paths cut at the target, are then the same wherever the lists are: after a compaction the
 *     decode runs on fewer rows and a float32 score may move in its last bits (by at most 4e-5 max_j ||W_j||_1, the bound of the
 *     path trace), which moves a choice only where u lies within that distance, over T, of a cumulative share, or where the
 *     order of two candidates hangs on it;
 *   irs_beam_step[_until | _linked | _ruled], irs_beam_search[_until] and the two _sharded loops return IRS_E_UNSUPPORTED;
 *   exclusions, no_repeat, the offer set, the trace and the arrival rule compose; with exact candidates bound as well the loops
 *     ask the survivor pass for want = top_k;
 *   the route where one workgroup ranks and steps a row is not taken; irs_path_step ALONE is unchanged.
 * irs_sampler_choose is the kernel alone on the caller's lists, under the bound parameters and into the bound records (IRS_E_STATE
 * without a binding); bound exclusions are honoured as irs_path_step honours them.  Like irs_lookahead_expand / irs_lookahead_choose
 * it is SYNCHRONOUS and takes no stream: the kernel is launched on the null stream and the call returns when it has finished; the
 * caller makes sure that the work that produces the inputs has finished.  Not for use inside a stream capture.
 *  dev_seq int64 [M, L], dev_hep int32 [M]; dev_val float [M, k] / dev_ids0 int64 [M, k]: the rows' ranked lists, rewritten
 *  step / seed: the step index (the records' column) and the draws' seed
 *  dev_row_ids int32 [M] (may be NULL: the identity): row -> the caller's row: the draw's key, the records' row, the bound user
 *  dev_status int32 [M]: read only
 *  dev_fin int32 [M] (may be NULL); dev_paths float [users, path_ld] (may be NULL): the path so far under no_repeat, as in
 *            irs_arrival_offer
 * Null pointers, M < 1, k outside [top_k, max_k], step < 0 or beyond path_ld, M above the bound exclusion users, no_repeat bound
 * and dev_paths NULL -> IRS_E_INVALID; all before the launch.
 * The kernel: one wave per row, four rows per workgroup; 2 KB of LDS per wave for the candidates besides the window and path
 * images; no atomics. */
#define IRS_MAX_SAMPLER_K 256
int irs_bind_sampler(irs_ctx *ctx, int32_t top_k, float temperature, float top_p, float *dev_rec_u, float *dev_rec_lq,
                     int32_t *dev_rec_support, int32_t users, int32_t ld);
int irs_sampler_choose(irs_ctx *ctx, const int64_t *dev_seq, const int32_t *dev_hep, int32_t M, float *dev_val, int64_t *dev_ids0,
                       int32_t k, int32_t step, uint64_t seed, const int32_t *dev_row_ids, const int32_t *dev_status,
                       const int32_t *dev_fin, const float *dev_paths, int32_t path_ld);

/* ---- arrival rule: offer the target once its rank or probability allows (opt-in; a deployed recommender shows a slate, so a
 *      persuasion path has done its work once the target stands among the best items the window leaves, not only when it is the
 *      best of them) --------------------------------------------------------------------------------------------------------------
 * A context can hold one ARRIVAL RULE, irs_set_arrival_rule(ctx, rank_max, lp_min):
 *   rank_max >= 1 turns the rank clause on, rank_max == 0 turns it off; rank_max < 0 -> IRS_E_INVALID.
 *   lp_min <= 0 turns the probability clause on (-inf included: it always holds); lp_min > 0 or NaN turns it off.
 *   Both clauses off clears the rule.  Setting a rule on a context with world != 1 -> IRS_E_UNSUPPORTED.
 *   Setting, changing or clearing the rule drops the captured steps; the rule is part of a captured step's key.
 * The rule reads what the path trace records and nothing else: while a rule is set, irs_generate_paths (stream launches and the
 * captured step alike) and irs_generate_paths_until need a bound path trace (irs_bind_path_trace) and return IRS_E_STATE with a
 * message, before any launch, without one.  irs_beam_search[_until] and the two _sharded loops return IRS_E_UNSUPPORTED while a
 * rule is set (they refuse a bound trace in any case).
 * For a live row of a step, behind the top-k, the survivor pass and the trace sweep and BEFORE the step chooses, let
 *   t  = seq[row][L-1],
 *   rk = the row's rank_target of this step (the trace's: the rank among what the window leaves),
 *   lp = rk ? (float)((double)ts - ((double)max + log((double)sumexp))) : 0 -- the very expression the trace stores as
 *        lp_target, so that the decision can be replayed from the recorded arrays alone.
 * The rule FIRES when rk != 0, the target is admissible under the step's own test, and at least one clause holds:
 *   the rank clause is on and rk <= rank_max, or the probability clause is on and lp >= lp_min (a NaN lp never fires).
 * The target is admissible when it lies in [1, n_item], is not in the window seq[row][0 .. hep[row]] (a window slot behind hep
 * does not count), is not in the bound exclusion list of the row's user (looked up through the until loop's compaction map) and,
 * under no_repeat, is not in the row's path so far.
 * A row that fires has its candidate list rewritten: entry 0 becomes (ts, t - 1), entry 1 becomes (-inf, -1) when k > 1, and
 * IRS_ROW_OFFERED is OR-ed into the row's status word.  A row that does not fire is not written; a finished row of the until loop
 * (still stepped until the next compaction) is skipped.  Nothing else changes: the unchanged path step -- greedy, sampled or
 * guided -- then chooses the target, its only survivor; the trace record finds the target in entry 0, so at a fired step lp_item
 * equals lp_target bit for bit; irs_generate_paths_until sees the target chosen and retires the user; irs_generate_paths
 * searches on behind the arrival, as the reference does.
 * The rank is the trace's unless the rule was set with irs_set_arrival_rule_ex(..., IRS_RANK_ADMISSIBLE): see "admissible rank"
 * below for the rank among what a bound exclusion list, no_repeat and an offer set ALSO leave.  That rank carried through beam
 * state is out of scope here: the beam trace and the beam rule keep the window's.
 * irs_arrival_offer is the kernel alone, on the outputs of irs_score_target_trace:
 *  dev_seq int64 [M, L], dev_hep int32 [M]; dev_max / dev_sumexp / dev_target_score float [M], dev_rank int32 [M] in
 *  dev_fin int32 [M] (may be NULL): rows with fin != 0 are skipped
 *  dev_val float [M, k] / dev_ids0 int64 [M, k] in / out: the rows' ranked lists
 *  rank_max, lp_min: as in irs_set_arrival_rule; both clauses off -> IRS_E_INVALID
 *  dev_paths float [M or users, path_ld] (may be NULL), step: under a bound no_repeat the path entries [0, step) of the row's user
 *            are inadmissible, as in irs_path_step; no_repeat bound and dev_paths NULL -> IRS_E_INVALID
 *  dev_row_map int32 [M] (may be NULL: the identity): row -> bound user, for the exclusion list and the path row; its values
 *            must lie in [0, users bound)
 *  dev_status int32 [M] in / out: IRS_ROW_OFFERED is OR-ed in
 * It honours bound exclusions as irs_path_step does.  Null pointers, M < 1, k outside [1, max_k], rank_max < 0, step < 0 or
 * beyond path_ld, M above the bound users -> IRS_E_INVALID; world != 1 -> IRS_E_UNSUPPORTED; all before any launch.
 * One wave per row, no LDS, no atomics: two identical calls give identical bytes.  With no rule set every entry point launches
 * exactly what it launched before. */
int irs_set_arrival_rule(irs_ctx *ctx, int32_t rank_max, float lp_min);
int irs_arrival_offer(irs_ctx *ctx, const int64_t *dev_seq, const int32_t *dev_hep, int32_t M, const float *dev_max,
                      const float *dev_sumexp, const float *dev_target_score, const int32_t *dev_rank, const int32_t *dev_fin,
                      float *dev_val, int64_t *dev_ids0, int32_t k, int32_t rank_max, float lp_min, const float *dev_paths,
                      int32_t path_ld, int32_t step, const int32_t *dev_row_map, int32_t *dev_status, void *stream);

/* ---- admissible rank: the target's rank among what the user could be OFFERED (opt-in; rank_target counts every excluded item
 *      that outscores the target, so it is not the position a slate of irs_recommend or a step of the search would give it) ----
 * Row b at step i, measured BEFORE the step chooses, with the path trace's scores e_j and total order (score descending, id
 * ascending, -0 folded onto +0):
 *   H(b,i) = the items the step's own admissibility test hides: the non-pad entries of the window seq[b][0 .. hep]; the bound
 *            exclusion list of the row's user; under no_repeat the non-zero path entries [0, i).
 *   U      = the valid (sanitised) ids of a bound offer set, or the whole catalog when none is bound.
 *   rank_adm[b][i] = 1 + #{ j in U \ H, j != t-1 : (e_j, j) ranks before (e_{t-1}, t-1) }.
 * The rank is defined whether or not the target itself is in H or outside U: it is where the target WOULD stand; the arrival rule
 * keeps its own admissibility test.  t == 0 or t outside the catalog: 0.  An item counts once however often it occurs in the list
 * (duplicates are legal there), the window, the path, or across the three.  With nothing but a trace bound, rank_adm equals
 * rank_target in every cell.  rank_adm <= rank_target without an offer set.  Where the target is admissible and rank_adm <= n, its
 * 0-based position in irs_recommend's slate of n on the same row and bindings is rank_adm - 1.
 * One kernel behind the trace sweep corrects the sweep's count exactly: the distinct union of H is gathered per row, each member is
 * scored with the exact chain (irs_score_gather's bits) and compared with the target; with an offer set the count over U comes
 * from the set's score pass (same bits).  Integer sums only: two identical calls give identical bits.  (A set with holes is not a
 * valid set: an id then counts as often as the sanitised array holds it, which is what the set's ranking emits.)
 * irs_score_target_rank_admissible is irs_score_target_trace's launches and then that kernel.  It takes no stream, like
 * irs_recommend and irs_score_topk_offer, whose score pass it runs in the bound offer set's scratch: the work is enqueued on the
 * null stream and the call returns without waiting (the ordering rules are those stated under irs_score_topk_offer):
 *  dev_xrows / dev_seq / dev_hep / M, dev_trace_scratch / trace_bytes, dev_max / dev_sumexp / dev_target_score / dev_rank: as in
 *            irs_score_target_trace, with the same results
 *  dev_paths float [M, path_ld] (may be NULL), step: the non-zero entries [0, step) of row r's path enter H, whether or not
 *            no_repeat is bound; step in [0, min(path_ld, 64)]
 *  dev_scratch: caller-owned, >= irs_admissible_scratch_bytes(M) bytes (one int32 per row, rounded up to 256), 16-byte aligned
 *  dev_rank_adm int32 [M] out
 *  It reads the bound exclusion LIST (row r is bound user r, as in irs_recommend; a binding of no_repeat alone holds no list)
 *  and a bound offer set, whose scratch must hold M rows (the set's score pass runs for them).  It is no search: no search
 *  option refuses it, and it drops no captured step.  Null pointers, M outside [1, max_rows], a scratch too small or misaligned,
 *  a bad step, more rows than the bound list's users or the set's pass -> IRS_E_INVALID; world != 1 -> IRS_E_UNSUPPORTED; then
 *  weights / workspace -> IRS_E_STATE; all before any launch.
 * irs_bind_trace_admissible adds a fourth array to a BOUND path trace: dev_rank_adm int32 [users, ld] with the trace's users and
 * ld (else IRS_E_INVALID; no trace bound -> IRS_E_STATE), and a caller-owned scratch >= irs_admissible_scratch_bytes(users) that
 * must stay valid until the unbind.  A NULL array unbinds; unbinding or rebinding the path trace drops this binding as well.
 * Binding and unbinding drop the captured steps.  While bound, irs_generate_paths and irs_generate_paths_until run the kernel
 * behind the trace sweep of every step and write the value at the caller's row and the step's column in exactly the cells where
 * rank_target is written (every column; up to and including the arrival step, zero behind it, in the until loop).  Sampling,
 * guide, lookahead, exact candidates, exclusions, no_repeat, an offer set and long windows compose: the kernel reads the step's
 * own exclusion arguments.
 * irs_set_arrival_rule_ex is irs_set_arrival_rule with the rank the rank clause reads: IRS_RANK_WINDOW (irs_set_arrival_rule's)
 * or IRS_RANK_ADMISSIBLE, under which rk above is the row's rank_adm of this step; any other kind -> IRS_E_INVALID.  A loop
 * entered with an IRS_RANK_ADMISSIBLE rule and no admissible binding returns IRS_E_STATE with a message, before any launch.
 * With rank_max = 1 the rule then fires exactly where the target is the best admissible item: the greedy step's own choice. */
#define IRS_RANK_WINDOW 0
#define IRS_RANK_ADMISSIBLE 1
size_t irs_admissible_scratch_bytes(const irs_ctx *ctx, int32_t rows); /* 0 for invalid arguments */
int irs_score_target_rank_admissible(irs_ctx *ctx, const float *dev_xrows, const int64_t *dev_seq, const int32_t *dev_hep, int32_t M,
                                     const float *dev_paths, int32_t path_ld, int32_t step, void *dev_trace_scratch,
                                     size_t trace_bytes, void *dev_scratch, size_t bytes, float *dev_max, float *dev_sumexp,
                                     float *dev_target_score, int32_t *dev_rank, int32_t *dev_rank_adm);
int irs_bind_trace_admissible(irs_ctx *ctx, int32_t *dev_rank_adm, int32_t users, int32_t ld, void *dev_scratch, size_t bytes);
int irs_set_arrival_rule_ex(irs_ctx *ctx, int32_t rank_max, float lp_min, int32_t rank_kind);

/* ---- beam rule: an arrival rule and a target-aware ranking on beam trace state (opt-in, off by default; BUILD-DEFINED like the
 *      beam search itself.  Without it a beam search ranks by acceptance alone -- the cumulative log-probability of the offered
 *      items -- and meets the target only where it happens to be a beam's most probable admissible child) ----------------------
 * A separate option from the arrival rule above: what irs_set_arrival_rule admits and refuses is unchanged, and the beam loops
 * still refuse it.  A context can hold one BEAM RULE, irs_set_beam_rule(ctx, rank_max, lp_min, target_weight):
 *   rank_max and lp_min mean what they mean in irs_set_arrival_rule: rank_max >= 1 turns the rank clause on, 0 turns it off,
 *     rank_max < 0 -> IRS_E_INVALID; lp_min <= 0 turns the probability clause on (-inf included), lp_min > 0 or NaN turns it off.
 *   target_weight is lambda: finite and >= 0, 0 turns the ranking off; negative, NaN or infinite -> IRS_E_INVALID.
 *   All three off clears the rule.  Setting a rule on a context with world != 1 -> IRS_E_UNSUPPORTED.
 *   Setting, changing or clearing the rule drops the captured steps, so a captured step never meets another rule.
 * The rule reads what the beam trace's sweep leaves on the device and nothing else: while a rule is set, irs_beam_search (stream
 * launches and the two captured ping-pong steps alike) and irs_beam_search_until need a bound beam trace (irs_bind_beam_trace)
 * and return IRS_E_STATE, with a message that names both calls, before any launch, without one.  With one they run, per step:
 * decode, top-k (+ lse), the survivor pass if bound, the trace sweep, the RULED step, the carry (unchanged), the step counter.
 * Every other search entry point -- irs_generate_paths[_until], irs_path_step, irs_beam_step[_until], irs_beam_step_linked and
 * the two _sharded loops -- returns IRS_E_UNSUPPORTED with a message that names the rule: it is never silently ignored.
 *
 * A ruled step.  For a live, unfinished input beam row r of a user that is not done, let
 *   t   = seq[r][L-1],  rk = dev_rank[r],
 *   lpt = rk ? (float)((double)ts - ((double)max + log((double)sumexp))) : 0 -- the very expression the beam trace stores as
 *         lp_target, so that every decision can be replayed from the recorded arrays alone.
 * 1. ARRIVAL.  The rule fires for r when rk != 0, a clause holds -- the rank clause is on and rk <= rank_max, or the probability
 *    clause is on and lpt >= lp_min (a NaN never fires) -- and t is admissible under the beam step's own test: it lies in
 *    [1, n_item], outside the window seq[r][0 .. hep[r]], outside the bound exclusion list of the user, under no_repeat outside
 *    the beam's own path [0, step), and inside a bound offer set (irs_bind_offer_set).  A fired beam contributes exactly ONE
 *    candidate, the target: index parent * W + 0, list value ts, score cum + ((double)ts - norm) with the step's usual
 *    norm = (double)lse_max + log((double)lse_sum) (no norm at W == 1).  Its ranked list is not walked and not rewritten, and
 *    IRS_ROW_OFFERED is OR-ed into the user's status word (through the until loop's map).  In the until forms the child is
 *    finished by the existing end-symbol test; in the plain forms the search goes on behind the arrival, as the greedy loop does.
 *    The carry then gives lp_item == lp_target bit for bit at a fired step.
 * 2. RANKING.  Every candidate keeps its acceptance score s = cum_parent + log p(item | parent): dev_cum_out, dev_scores and the
 *    trace hold what they held.  The candidates are ORDERED by the key s + (double)lambda * (double)bonus, descending, then by
 *    index ascending.  bonus = lpt(r) for the children of row r, 0 for a row without a target or with a NaN lpt, and 0 for a
 *    finished beam that re-enters as itself (it has arrived: 0 is the largest value lpt can take).  This is the one-step-lagged
 *    form of sum log p(item) + lambda * lp_target(state): the term is common to all children of a parent, so it decides between
 *    prefixes, costs no decode and carries no state across steps.  At lambda == 0 the key IS s (0 * -inf is never formed), and a
 *    ruled step with both clauses off besides would be the linked step bit for bit.
 * 3. STOP RULES.  IRS_BEAM_STOP_BEST stays "done once output beam 0 is finished".  Under lambda > 0 the argument that BEST
 *    returns what ALL would (irs_beam_search_until) no longer holds: a child's bonus can exceed its parent's, so a later
 *    candidate's key can overtake a finished beam 0.  BEST then returns the earlier answer.
 * 4. RETURNED SCORES.  dev_scores / dev_cum_out are acceptance sums in KEY order: with lambda > 0 they need not be descending.
 *
 * irs_beam_step_ruled is the step alone: irs_beam_step_linked's arguments, checks and outputs (the until form when dev_fin_in,
 * dev_fin_out and dev_done are all given; it refuses what irs_beam_step_linked refuses and looks at neither a bound beam trace nor
 * a set rule), then
 *  dev_max / dev_sumexp / dev_target_score float [B*W], dev_rank int32 [B*W]: irs_score_target_trace on the step's INPUT rows
 *  rank_max, lp_min, target_weight: as in irs_set_beam_rule; all three off -> IRS_E_INVALID
 * It honours bound exclusions and a bound offer set's membership for the target, as irs_arrival_offer does.  Null pointers and
 * bad values -> IRS_E_INVALID; world != 1 -> IRS_E_UNSUPPORTED; all before the launch.  SYNCHRONOUS on the null stream, like
 * irs_beam_step_linked.  No float atomics; the status word takes an integer atomic OR: identical calls give identical bytes. */
int irs_set_beam_rule(irs_ctx *ctx, int32_t rank_max, float lp_min, float target_weight);
int irs_beam_step_ruled(irs_ctx *ctx, const int64_t *dev_seq_in, const int32_t *dev_hep_in, const double *dev_cum_in,
                        const float *dev_paths_in, const int32_t *dev_fin_in, const float *dev_val, const int64_t *dev_ids0,
                        const float *dev_lse_max, const float *dev_lse_sum, int32_t B, int32_t W, int32_t k, int32_t step,
                        int32_t P, int32_t stop_rule, int64_t *dev_seq_out, int32_t *dev_hep_out, double *dev_cum_out,
                        float *dev_paths_out, int32_t *dev_fin_out, int32_t *dev_done, int32_t *dev_status, int32_t *dev_link,
                        float *dev_link_val, const float *dev_max, const float *dev_sumexp, const float *dev_target_score,
                        const int32_t *dev_rank, int32_t rank_max, float lp_min, float target_weight);

/* ---- path replay: every step of SAVED paths scored in one batched pass (opt-in; replaces the Python loop of dependent launches
 *      of Evaluator.get_grad_in_batch, evaluator.py:162-243 -- one decode + LogSoftmax + gather per step -- and the two extra
 *      decodes of get_rr_increase_in_batch, evaluator.py:245-290; and gives the loops that carry no trace -- beam, sharded, paths
 *      read from paths_d_<n>.npy -- the trace's three values after the fact) ---------------------------------------------------
 * A saved path is teacher-forced: the window before step i is known from the start window and the first i path items, so no
 * step waits for another.  A REPLAY ROW is a pair (b, i): user b after i forced items.  Its window is the user's start window
 * with path[b][0 .. i) applied by the layout's step rule; its consumed row is hep; its forced item is c = path[b][i] (0 when
 * i == P, or when the path holds 0 there: the row then has no item).  dev_paths is int64 [B, path_ld], 1-based ids, P <= path_ld.
 * Two layouts:
 *   IRS_REPLAY_SLOT  the search loops' layout.  The start window is seq0[b][0 .. L) with the target in slot L-1 and hep0[b]
 *                    given (in [0, L-2]).  The step rule is irs_path_step's: grow while hep < L-2 (the item goes to slot hep+1),
 *                    otherwise shift slots [0, L-2] left by one and append at L-2; the target stays.  Closed form, with g = L-2
 *                    - hep0: for i <= g slot p in (hep0, hep0+i] holds path[p-hep0-1], every other slot is seq0's, hep = hep0+i;
 *                    for i > g slot p <= L-2 holds entry p+i-g of seq0[0 .. hep0] ++ path[0 .. i), hep = L-2.
 *                    The target is seq0[b][L-1]: dev_target must be NULL.  Both mask modes (a causal context uses the layout as
 *                    Rec2Inf does).
 *   IRS_REPLAY_FULL  the evaluator's layout.  Windows are post-padded and all L slots are window; n0 is the index of the first
 *                    0 of the start row (L if there is none).  The step rule is get_grad_in_batch's: write at n0+i while the
 *                    window is not full, otherwise shift the WHOLE window left by one and append at L-1.  Closed form, with n =
 *                    n0+i and s = max(n-L, 0): slot p holds entry p+s of seq0[0 .. n0) ++ path[0 .. i), 0 from entry n on;
 *                    hep = min(n, L) - 1.  The target is dev_target[b] (required); slot L-1 is an ordinary window slot.
 *                    IRS_MASK_CAUSAL contexts only for irs_replay_paths: the IRN mask gives column L-1 a meaning.
 * Values of a row, defined exactly as the path trace defines them and formed with the same arithmetic: lse over the WHOLE
 * catalog from the float32 pair (max, sumexp);
 *   lp_target   = e_{t-1} - lse;    lp_item = e_{c-1} - lse, 0 without an item or with c outside [1, n_item];
 *   rank_target = the rank among what the window seq[0 .. hep] leaves, in the library's total order;
 * each log-probability is (double)e - ((double)max + log((double)sumexp)) rounded to float32 once; a target of 0 or outside the
 * catalog gives 0 / 0.  A bound trace, guide, exclusion list or arrival rule does not enter: replay chooses nothing.
 * A row is INVALID when b is outside [0, B), i is outside [0, P], one of path[b][0 .. i) is outside [1, n_item], the window
 * would be empty (FULL with n0 + i == 0), or (SLOT) hep0[b] is outside [0, L-2].  An invalid row never faults and never reads
 * out of bounds: it gets the user's start window if b is valid, otherwise user 0's (FULL: entries [0, n0) and zeros; the single
 * item 1 in slot 0 when that is empty; SLOT: the row as it is, hep0 clamped into [0, L-2]), so every launched window is well
 * formed; it records 0 / 0 / 0 and IRS_ROW_NO_CANDIDATE in dev_status[r].  Valid rows get IRS_ROW_OK.
 * irs_replay_windows is the builder alone, as irs_score_target_trace is the sweep alone: one launch, one wave per row, no
 * weights and no workspace needed, any mask mode, R up to 2^24, L up to IRS_MAX_LEN_LONG.
 *  dev_seq0 int64 [B, L], dev_hep0 int32 [B] (SLOT; ignored and may be NULL for FULL), dev_user int64 [B] (may be NULL)
 *  dev_row_user / dev_row_step int32 [R]: the rows, in any order, repeats allowed
 *  dev_seq_out int64 [R, L], dev_hep_out int32 [R], dev_user_out int64 [R] (may be NULL; written when dev_user is given),
 *  dev_status int32 [R] out
 * irs_replay_paths walks the rows in order, in passes of `chunk` rows (in [1, min(max_rows, max_seqs)]) with a ragged last
 * pass.  A pass is: windows -> the decoder with pos = hep and no [B, L, d] output -> the target's and the forced item's exact
 * scores (irs_score_gather's arithmetic) -> the chain-order sweep, its reduction and the window correction of
 * irs_score_target_trace, unchanged -> one record kernel that forms the three values.  All passes go on the caller's stream;
 * no host reads, no allocation, no hipGraph, no float atomics: two identical calls give identical bits.
 *  dev_target int64 [B] (FULL; NULL for SLOT); dev_lp_item / dev_lp_target float [R], dev_rank int32 [R], dev_status int32 [R] out
 *  dev_scratch: caller-owned like irs_ce_backward's, >= irs_replay_scratch_bytes(chunk) bytes, 16-byte aligned: the pass's
 *            windows, hep, users, items, targets, x rows, the item scores and the trace rows
 *            (irs_path_trace_scratch_bytes(chunk)), each rounded up to 256 bytes.  irs_workspace_bytes does not change.
 * Checks, all before any launch: a null pointer, R < 1 (R > 2^24), B < 1, P < 0, path_ld < P, a chunk out of range, an unknown
 * layout, FULL without dev_target, SLOT with dev_target or without dev_hep0, an IRN context without dev_user, a scratch too
 * small or misaligned -> IRS_E_INVALID; world != 1, FULL on an IRN context -> IRS_E_UNSUPPORTED; no weights or no workspace
 * -> IRS_E_STATE.  Every other entry point launches exactly what it launched before. */
#define IRS_REPLAY_SLOT 0
#define IRS_REPLAY_FULL 1
#define IRS_REPLAY_MAX_ROWS (1 << 24)
size_t irs_replay_scratch_bytes(const irs_ctx *ctx, int32_t chunk); /* 0 for invalid arguments */
int irs_replay_windows(irs_ctx *ctx, int32_t layout, const int64_t *dev_seq0, const int32_t *dev_hep0, const int64_t *dev_user,
                       int32_t B, const int64_t *dev_paths, int32_t P, int32_t path_ld, const int32_t *dev_row_user,
                       const int32_t *dev_row_step, int32_t R, int64_t *dev_seq_out, int32_t *dev_hep_out, int64_t *dev_user_out,
                       int32_t *dev_status, void *stream);
int irs_replay_paths(irs_ctx *ctx, int32_t layout, const int64_t *dev_seq0, const int32_t *dev_hep0, const int64_t *dev_user,
                     const int64_t *dev_target, int32_t B, const int64_t *dev_paths, int32_t P, int32_t path_ld,
                     const int32_t *dev_row_user, const int32_t *dev_row_step, int32_t R, int32_t chunk, void *dev_scratch,
                     size_t scratch_bytes, float *dev_lp_item, float *dev_lp_target, int32_t *dev_rank, int32_t *dev_status,
                     void *stream);

/* ---- multi-GPU: the exchange steps and the sharded search loops below the ABI (section 8 row B2's
 *      `allgather_merge(ctx, comm, ...)`).  One process per GPU; rank r holds item rows [item_lo, item_hi) (irs_shard).
 * A communicator is either RCCL (librccl.so is dlopen()ed on first use: ncclCommInitRank over a 128-byte unique id the
 * caller distributes, e.g. with its torch.distributed store) or a set of caller-supplied collectives (the CPU
 * rehearsal tests run gloo through it).  Every collective is enqueued on the caller's stream: decode -> row
 * all-gather -> shard sweep -> pack -> key exchange -> merge -> path / beam step is ONE stream-ordered sequence over
 * buffers of the context's workspace, nothing is allocated per call, and with RCCL the whole step can be captured
 * into a hipGraph (use_graph).  The reference has no counterpart (nn.DataParallel only, pipeline.py:43-44). */
typedef struct irs_comm irs_comm;
#define IRS_COMM_ID_BYTES 128
#define IRS_REDUCE_SUM 0
#define IRS_REDUCE_MAX 1
/* all-gather: every rank contributes bytes_per_rank bytes, receives world * bytes_per_rank (rank-major);
 * all-to-all: slice j of send (bytes_per_rank bytes) goes to rank j, slice i of recv came from rank i;
 * all-reduce: in place over `count` float32.  Device pointers; ordered against `stream`; return 0 on success. */
typedef int (*irs_allgather_fn)(void *user, const void *dev_send, void *dev_recv, size_t bytes_per_rank, void *stream);
typedef int (*irs_alltoall_fn)(void *user, const void *dev_send, void *dev_recv, size_t bytes_per_rank, void *stream);
typedef int (*irs_allreduce_f32_fn)(void *user, float *dev_buf, size_t count, int op, void *stream);

int irs_comm_unique_id(void *out_id128);                        /* RCCL: ncclGetUniqueId (call on one rank) */
int irs_comm_init_rccl(irs_comm **out, const void *id128, int32_t rank, int32_t world); /* ncclCommInitRank on the CURRENT device */
int irs_comm_init_callbacks(irs_comm **out, int32_t rank, int32_t world, void *user, irs_allgather_fn allgather,
                            irs_alltoall_fn alltoall, irs_allreduce_f32_fn allreduce);
void irs_comm_destroy(irs_comm *comm);
const char *irs_comm_last_error(void);
int irs_comm_is_rccl(const irs_comm *comm);
/* how irs_exchange_topk moves the keys: 0 = caller-supplied callbacks, 1 = ncclAllToAll (an RCCL extension), 2 = grouped
 * ncclSend / ncclRecv (libraries without the extension; IRS_RCCL_NO_ALLTOALL=1 in the environment at irs_comm_init_rccl
 * forces it, so that the fallback can be tested on a library that has the extension) */
int irs_comm_exchange_kind(const irs_comm *comm);
/* NCCL version code of the librccl.so in use (0 before the first irs_comm_unique_id / irs_comm_init_rccl).  The library is
 * refused at load time unless its major version is the one csrc/comm.hip was compiled against (rccl.h: 2.x). */
int irs_comm_rccl_version(void);

/* rows decoded data-parallel -> all rows on every rank, rank-major: dev_rows_all float [world * B, d]. */
int irs_allgather_rows(irs_ctx *ctx, irs_comm *comm, const float *dev_rows_local, int32_t B, float *dev_rows_all, void *stream);
/* packed per-shard lists of ALL rows (dev_keys_send uint64 [world, B, k], rank-major rows: what irs_pack_topk makes of
 * this rank's irs_score_topk over the gathered rows) -> the world's lists of THIS rank's B rows (dev_keys_recv
 * uint64 [world, B, k], shard-major): one all-to-all of M * k * 8 bytes per rank (SURVEY 8e's budget). */
int irs_exchange_topk(irs_ctx *ctx, irs_comm *comm, const uint64_t *dev_keys_send, uint64_t *dev_keys_recv, int32_t B,
                      int32_t k, void *stream);

/* irs_generate_paths over an item-sharded catalog (replaces the loop of IRSNN.get_seq_in_batch, influentialRS.py:412-450):
 * this rank's B users, per step { decode, row all-gather, sweep of the local shard for all world * B rows, pack,
 * all-to-all of keys, merge, path step }.  Needs max_rows >= world * B, max_seqs >= B; every rank calls it with the
 * same B / max_path_len / k / sweep.  Results equal the single-device irs_generate_paths bit for bit. */
int irs_generate_paths_sharded(irs_ctx *ctx, irs_comm *comm, int64_t *dev_seq, const int64_t *dev_user, int32_t *dev_hep,
                               int32_t B, int32_t max_path_len, int32_t k, int32_t sweep, int32_t sample, int32_t sample_k,
                               uint64_t seed, int32_t use_graph, float *dev_paths, int32_t *dev_status, void *stream);

/* irs_beam_search over an item-sharded catalog.  split_decode == 0: this rank's OWN B users (rows = B * W per rank;
 * all-gather of rows, all-to-all of keys, all-reduce of the rows' (max, sum exp)); needs max_rows >= world * B * W.
 * split_decode != 0 (BASELINE configs[4]: ONE user's beams spread over the node): every rank passes the SAME B users
 * and keeps the same beam state; per step rank r decodes rows [r R/world, (r+1) R/world) of the R = B * W beam windows
 * (R a multiple of world), the rows are all-gathered, every rank sweeps its shard for all R rows, the packed lists are
 * all-gathered and merged on every rank, and the (deterministic) beam step runs replicated; needs max_rows >= R,
 * max_k * world <= 2048.  Outputs as irs_beam_search (identical on every rank when split_decode). */
int irs_beam_search_sharded(irs_ctx *ctx, irs_comm *comm, const int64_t *dev_seq0, const int64_t *dev_user,
                            const int32_t *dev_hep0, int32_t B, int32_t W, int32_t P, int32_t k, int32_t sweep,
                            int32_t split_decode, int32_t use_graph, float *dev_paths, double *dev_scores,
                            int64_t *dev_seq_final, int32_t *dev_status, void *stream);

/* irs_ce_forward / irs_ce_backward over an item-sharded catalog: the vocabulary-parallel form of CrossEntropyLoss(project(x)[valid],
 * label - 1) as the reference runs it on one device in IRSNN.train_batch / get_loss_on_eval_data (influentialRS.py:252-310) and
 * Evaluator.train_batch / get_loss_on_eval_data (evaluator.py:53-92).  Rows are data-parallel: every rank passes ITS OWN B rows
 * (the same B on every rank) with GLOBAL 0-based labels (-1 = row ignored) and holds item rows [item_lo, item_hi) of project.*;
 * the loss is the one over the WORLD's rows.  Needs max_rows >= world * B (IRS_E_INVALID otherwise).  Both work over either kind
 * of communicator and with world == 1, where they equal irs_ce_forward / irs_ce_backward bit for bit.  project.* are read where
 * they were bound and the derived bf16 catalog is marked stale, exactly as irs_ce_forward does.  Nothing is allocated: the
 * gathered rows, labels and per-shard terms live in the bound workspace, the backward's partial outputs in the caller's scratch;
 * all kernels and collectives are enqueued on the caller's stream.  Null pointers, B < 1, world * B > max_rows and (backward) a
 * scratch smaller than irs_ce_backward_sharded_scratch_bytes(B) or not 16-byte aligned return IRS_E_INVALID before any launch or
 * collective; unbound weights / workspace IRS_E_STATE.
 *  irs_ce_forward_sharded: all-gather of rows and labels (rank-major) -> the float32 log-sum-exp sweep and the label gather of
 *                   irs_ce_forward over this shard for all world * B rows (label score -inf where the label is outside the
 *                   shard) -> all-gather of the per-shard (lse, label score) -> per row, shards in rank order:
 *                   lse = m + log sum_r exp(lse_r - m), m = max_r lse_r; label score = the one entry that is not -inf.
 *                   dev_lse / dev_label_score float [B]: this rank's own rows.  dev_loss double [3] as irs_ce_forward's, over the
 *                   rows of the whole world in gathered order: identical bits on every rank.  Ignored rows and labels >= n_item
 *                   behave as in irs_ce_forward.
 *  irs_ce_backward_sharded: dev_lse float [B] is the forward's (global).  All-gather of rows, labels and lse -> the two passes of
 *                   irs_ce_backward over this shard for all world * B rows: dev_dw [n_local, d] / dev_db [n_local] are then
 *                   COMPLETE for the shard (overwritten or, accumulate != 0, added to; no reduction over ranks), the dx partial
 *                   [world * B, d] goes to the scratch -> one all-to-all hands every rank the world's partials of its own B rows
 *                   -> dev_dx float [B, d] = their sum in rank order (always overwritten; an ignored row is exactly zero).  No
 *                   float atomics and no all-reduce of dx: two identical calls give identical bits.  Scratch: the single-device
 *                   backward's at world * B rows plus 8 world B d bytes. */
int irs_ce_forward_sharded(irs_ctx *ctx, irs_comm *comm, const float *dev_xrows_local, const int64_t *dev_labels0_local, int32_t B,
                           float *dev_lse, float *dev_label_score, double *dev_loss, void *stream);
size_t irs_ce_backward_sharded_scratch_bytes(const irs_ctx *ctx, int32_t B); /* 0 for an invalid B */
int irs_ce_backward_sharded(irs_ctx *ctx, irs_comm *comm, const float *dev_xrows_local, const int64_t *dev_labels0_local,
                            const float *dev_lse, int32_t B, float scale, int32_t accumulate, float *dev_dx, float *dev_dw,
                            float *dev_db, void *dev_scratch, size_t scratch_bytes, void *stream);

/* Opt-in overlap of irs_generate_paths_sharded's collectives with its compute (round 5; greedy choice only): the step's users run
 * as TWO micro-batches, the row all-gather and the key all_to_all of one on a side stream (chained by events) while the other
 * decodes / sweeps / merges on the caller's stream -- per step one all-gather and one all_to_all leave the critical path.  Same
 * results bit for bit (rows are independent).  Off by default: two micro-batches cost decoder efficiency on small batches, and
 * the build loop has one GPU (the overlap itself has never been measured).  Stream launches only (use_graph is ignored). */
int irs_set_sharded_overlap(irs_ctx *ctx, int32_t on);
int irs_get_sharded_overlap(const irs_ctx *ctx);

/* State of the sharded loops' step capture (tests / diagnostics): bit 0 = a captured step is held, bit 1 = capture was
 * attempted and refused by the collective library (plain stream launches from then on). */
int irs_sharded_graph_state(const irs_ctx *ctx);

/* ---- decoder GEMM arithmetic -------------------------------------------
 * The throughput path's fused layer kernel (d = 128, ffn = 256: out-projection, both layer norms, feed-forward, the
 * next layer's q | k | v) multiplies in one of three ways; all accumulate in float32 and agree to ~1e-6 relative on the
 * decoder rows (tests/test_gpu_decoder_path.py holds the bound):
 *   IRS_GEMM_H3  (default since round 4) two float16 planes per operand, three products: see the constant below;
 *   IRS_GEMM_X6  every float32 operand is split exactly into three bf16 planes (h + m + l) and the six
 *                leading products hh, hm, mh, hl, lh, mm are summed on v_mfma_f32_32x32x16_bf16: float32-grade products
 *                at 6/16 of the float32-MFMA instruction time;
 *   IRS_GEMM_F32 v_mfma_f32_32x32x2f32.
 * The initial mode is IRS_GEMM_H3 unless the environment holds IRS_DECODER_GEMM=x6 or =f32 when the context is created
 * (any other value than h3 / x6 / f32 fails irs_create; the same holds for IRS_ATTN_GEMM).
 * Changing the mode drops the context's captured steps (they are re-captured on the next graph call).
 * Attention of the throughput path at head dim 32 behind a split-precision layer kernel (environment IRS_ATTN_GEMM, read at
 * creation): default "h3" -- scores on the float32 matrix chain, O^T += V^T P^T on float16 plane pairs, the V section of a
 * q | k | v row being WRITTEN as [32 f16 h | 32 f16 l] per (token, head) by the layer kernel (same 128 bytes; rows within 6e-6
 * of the float32 attention's); "f32": the float32-MFMA attention on float32 q | k | v rows.  (Round 5 removed the variants that
 * lost twice -- split-bf16 attention "x6", the persistent work-list attention IRS_ATTN_PERSIST, the one-wave d = 256 layer kernel
 * IRS_X6D_MIN_ROWS: their records are under profiles/r03, profiles/r04 and in HISTORY.md.)  The q | k | v buffer is internal to
 * irs_decode: no caller sees the plane format. */
#define IRS_GEMM_F32 0
#define IRS_GEMM_X6 1
/* IRS_GEMM_H3 (round 4): two FLOAT16 planes per float32 operand (h = f16(x), l = f16(x - h)) and the three leading products hh,
 * hl, lh on v_mfma_f32_32x32x16_f16 -- half the matrix instructions of IRS_GEMM_X6.  Error model (round 5): a value's two planes
 * carry it to 2^-22 RELATIVE while l is a normal float16 (|x| >= 2^-3) and to 2^-25 ABSOLUTE below that (l subnormal).  The weight
 * operands -- O(0.05) in a trained model -- are therefore packed times 2^8 (exact; the epilogues fold the 2^-8 into their bias
 * multiply-add), which puts their absolute floor at 2^-33; the activation operands are O(1) LayerNorm outputs, hidden units and
 * attention outputs, where 2^-25 absolute is 2^-25 of the sum they enter.  Needs 2^8 |weights|, |activations| < 65504 (float16):
 * checked at finalisation, see irs_h3_range_bound. */
#define IRS_GEMM_H3 2
int irs_set_decoder_gemm(irs_ctx *ctx, int32_t mode);
int irs_get_decoder_gemm(const irs_ctx *ctx);           /* the selected mode (a get / set round trip restores it) */
int irs_get_decoder_gemm_effective(const irs_ctx *ctx); /* the mode that runs (IRS_GEMM_X6 where IRS_GEMM_H3 fails its range bound) */
/* Sequence-resident decoder layers (round 5; reference model/influentialRS.py:183-193 is ONE nn.TransformerDecoder call): with
 * IRS_GEMM_H3 at d = 128, 4 heads, ffn 256, L <= 256, rows-only decodes of a throughput batch run every layer but the last as ONE
 * launch -- q | k | v from x, K / V of a head in LDS, attention, out-projection, feed-forward, layer norms -- on whole sequences
 * per workgroup (k_block_x6<.., SEQ>), instead of a layer kernel + an attention kernel exchanging q | k | v rows through HBM.
 * The launch covers layers 0 .. n - 2 (x stays in registers from layer to layer) and the q | k | v + attention of the last layer
 * for the consumed token's block: no q | k | v row ever reaches HBM.  GEMM arithmetic as in the default kernels; attention scores as
 * three float16 plane products (the default kernels: float32 MFMAs): rows within 2e-5 of theirs, as close to the float32 kernels.
 * mode: 0 never, 1 whenever the shape allows, 2 (default) from 384 sequences per call up, where it measured 8-12 % ahead of the
 * two-kernel path.  Environment IRS_DECODER_SEQ=0 / 1 / auto at creation or this call.
 * irs_decoder_seq_last: 1 when the last irs_decode took this path. */
int irs_set_decoder_seq(irs_ctx *ctx, int32_t mode);
int irs_get_decoder_seq(const irs_ctx *ctx);
int irs_decoder_seq_last(const irs_ctx *ctx);
/* Dense form of the swept top-k (small catalogs, many rows).  Where a shard's padded item count fits a row's candidate array
 * (n_tiles * 32 <= 4096), irs_score_topk[_carry] and the search loops' steps with IRS_SWEEP_BF16, d_pad >= 32 and k <= 256 can run
 * as three launches instead of five: k_prep_x, ONE bf16 sweep that stores every approximate score of a row into its candidate array
 * (k_sweep_ring16, image mode), and k_dense_select, one workgroup per row: a bound T from the 256 per-thread maxima, the items with
 * approx >= T - 2 eps re-scored with the exact chain and ranked.  Results are those of the other routes bit for bit.  Not taken with
 * IRS_SWEEP_F32 (which stays an independent check), when the log-sum-exp is wanted, or for a fused path step.
 * On this form nothing is speculative: IRS_ROW_FALLBACK is set only for a row with more than 1024 items within 2 eps of its k-th
 * approximate score (near-duplicate catalogs), which the selection workgroup redoes exhaustively; a carried call is a plain call.
 * mode: 0 never, 1 wherever the form is eligible (any row count), 2 (default) where it is eligible and measured ahead -- see
 * profiles/dense_topk/README.md for where that is.  Environment IRS_TOPK_DENSE=0 / 1 / auto at creation or this call.
 * irs_topk_dense_last: 1 when the last top-k launch took this form. */
int irs_set_topk_dense(irs_ctx *ctx, int32_t mode);
int irs_get_topk_dense(const irs_ctx *ctx);
int irs_topk_dense_last(const irs_ctx *ctx);
/* irs_decoder_route_last (tests): the kernel route the last irs_decode took, as int32 fields in this order:
 *   rows_only, small_plan, plan, embed, layer, tail, frag, seq, kv_planes, att_fused, kv_only, x6, npl, nt
 * plan: 0 NONE (full decode), 1 MULTI, 2 SMALL, 3 IN_EMBED; embed: 0 FULL, 1 PACKED, 2 FRAG, 3 FRAG_QKV, 4 SMALL16_QKV, 5 ANY_QKV,
 * 6 SEQ; layer / tail: 0 GEMM, 1 GEMM_LN, 2 FRAG_GEMM, 3 FRAG_BLOCK, 4 FRAG_FUSED, 5 SMALL16, 6 WIDE, 7 ANY; the flags 0 / 1.
 * Writes min(n, IRS_ROUTE_FIELDS) fields to out and returns that number; IRS_E_STATE before any decode.  Launches nothing.
 * Behind a search loop with a bound lookahead (irs_bind_lookahead) it reports the step's inner decode, of the child windows. */
#define IRS_ROUTE_FIELDS 14
int irs_decoder_route_last(const irs_ctx *ctx, int32_t *out, int32_t n);
/* (tests / lab) device address of a decoder workspace buffer: 0 x (fragment-major), 1 attention output (fragment-major), 2 / 3 the
 * sequence-resident plan's tile -> sequence / tile index, 4 image row of a sequence, 5 tile-order consumed row, 6 workgroup count,
 * 7 / 8 packed offset / count per sequence, 9 q | k | v rows, 10 packed consumed row.  Null for an unknown index. */
void *irs_debug_ptr(const irs_ctx *ctx, int32_t which);
/* Float16 planes overflow at 65504.  irs_finalize_weights bounds every operand of the float16-plane kernels from the bound
 * weights (embedded tokens, LayerNorm outputs, hidden activations, V rows, the weights themselves) and keeps half the range as
 * margin: a model whose bound is 32752 or more runs IRS_GEMM_X6 (no range limit) wherever IRS_GEMM_H3 is selected, with float32
 * V rows -- irs_get_decoder_gemm_effective reports the mode that RUNS (irs_get_decoder_gemm the selected one).  irs_h3_range_bound returns the bound (-1 before finalisation).
 * A NaN or infinite weight makes the bound infinite; the split-bf16 kernels then return the NaN rows the float32 kernels return.
 * (The reference has no counterpart: model/influentialRS.py:67-74 multiplies in float32 throughout.) */
float irs_h3_range_bound(const irs_ctx *ctx);

/* ---- measurement hooks (bench.py only) ---------------------------------
 * While enabled, every launch of the named kernel family is bracketed by HIP
 * events on the launch stream; irs_prof_read() synchronises those events and
 * returns launches and total milliseconds since the last reset. */
#define IRS_PROF_NONE 0
#define IRS_PROF_LINEAR 1  /* decoder GEMM family (fused layer kernel, layer-0 QKV) */
#define IRS_PROF_ATTN 2    /* decoder attention */
#define IRS_PROF_SWEEP 3   /* catalog sweep (pre-pass + emit) */
#define IRS_PROF_REFINE 4  /* candidate refine / exact re-score / sort */
#define IRS_PROF_SWEEP_EMIT 5 /* the emission sweep of irs_score_topk alone (the kernel the bf16 MFMA roofline is quoted on) */
#define IRS_PROF_LAYER 6   /* the fused layer kernel with the next layer's q | k | v (k_block_x6 / k_block) alone: the
                            * launches the decoder roofline is quoted on; flops are the algorithmic (float32-product) ones */
int irs_prof_enable(irs_ctx *ctx, int32_t family);
int irs_prof_read(irs_ctx *ctx, int32_t *launches, double *total_ms, double *total_flops, double *total_bytes);

#ifdef __cplusplus
}
#endif
#endif /* IRS_HIP_H */
