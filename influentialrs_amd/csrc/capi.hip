// C ABI of libirs_hip.so (include/irs_hip.h): context, weight binding, workspace
// planning, entry points, hipGraph-captured path generation, measurement hooks.
#include <stdlib.h>

#include <new>
#include <type_traits>

#include "irs_internal.h"

int irs_launch_topk_exhaustive(irs_ctx *ctx, const float *xrows, int M, int k, float *val, int64_t *ids0,
                               int32_t *status, hipStream_t s);

static char g_create_err[512] = "";

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

extern "C" int irs_abi_version(void) { return IRS_ABI_VERSION; }

extern "C" const char *irs_last_error(const irs_ctx *ctx) { return ctx ? ctx->err : g_create_err; }

extern "C" int irs_create(irs_ctx **out, const irs_dims *dims, const irs_shard *shard) { return irs_create_ex(out, dims, shard, 0u); }

extern "C" int irs_create_ex(irs_ctx **out, const irs_dims *dims, const irs_shard *shard, uint32_t flags) {
    if (!out || !dims) {
        snprintf(g_create_err, sizeof(g_create_err), "irs_create: null argument");
        return IRS_E_INVALID;
    }
    const irs_dims &D = *dims;
#define BAD(...)                                                   \
    do {                                                           \
        snprintf(g_create_err, sizeof(g_create_err), __VA_ARGS__); \
        return IRS_E_INVALID;                                      \
    } while (0)
    if (D.n_item < 1) BAD("n_item must be >= 1");
    if (D.d < 2 || D.d > 256 || (D.d & 1)) BAD("emb_dim must be even and in [2, 256] (got %d)", D.d);
    if (flags & ~IRS_CREATE_LONG_WINDOWS) BAD("irs_create_ex: unknown flag bits 0x%x", flags & ~IRS_CREATE_LONG_WINDOWS);
    const int len_max = (flags & IRS_CREATE_LONG_WINDOWS) ? IRS_MAX_LEN_LONG : 256;
    if (D.max_len < 2 || D.max_len > len_max) BAD("max_len must be in [2, %d] (got %d)", len_max, D.max_len);
    if (D.n_heads < 1 || D.d % D.n_heads) BAD("n_heads must divide emb_dim");
    if (D.d / D.n_heads > 64) BAD("head dim > 64 unsupported");
    if (D.n_layers < 1 || D.n_layers > IRS_MAX_LAYERS) BAD("n_layers out of range");
    if (D.ffn_dim < 1) BAD("ffn_dim must be >= 1");
    if (D.mask_mode != IRS_MASK_IRN && D.mask_mode != IRS_MASK_CAUSAL) BAD("bad mask_mode");
    if (D.mask_mode == IRS_MASK_IRN && (D.u_dim < 1 || D.n_user < 1)) BAD("IRN mask needs user embeddings");
    if (D.max_rows < 1) BAD("max_rows must be >= 1");
    if (D.max_k < 1 || D.max_k > 1024) BAD("max_k must be in [1, 1024]");
    irs_shard sh;
    if (shard) sh = *shard;
    else {
        sh.rank = 0;
        sh.world = 1;
        sh.item_lo = 0;
        sh.item_hi = D.n_item;
    }
    if (sh.item_lo < 0 || sh.item_hi > D.n_item || sh.item_lo >= sh.item_hi) BAD("bad item shard [%lld, %lld)", (long long)sh.item_lo, (long long)sh.item_hi);
    if (sh.item_hi - sh.item_lo > 0x7FFFFFE0LL) BAD("shard too large");
    {   // the launchers' per-device caches (MaxDynamicSharedMemorySize attributes, occupancy) are keyed by device ordinal
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && (dev < 0 || dev >= IRS_MAX_DEVICES))
            BAD("device ordinal %d: contexts are supported on devices 0 .. %d", dev, IRS_MAX_DEVICES - 1);
    }
#undef BAD
    irs_ctx *c = new (std::nothrow) irs_ctx();
    if (!c) {
        snprintf(g_create_err, sizeof(g_create_err), "out of host memory");
        return IRS_E_INVALID;
    }
    memset(c, 0, sizeof(*c));
    c->dims = D;
    c->shard = sh;
    c->n_local = sh.item_hi - sh.item_lo;
    int dp = 16;
    while (dp < D.d) dp <<= 1;
    c->d_pad = dp;
    c->KS = dp / 16;
    c->n_tiles = (int)((c->n_local + 31) / 32);
    c->max_rows = D.max_rows;
    c->max_seqs = D.max_seqs > 0 ? D.max_seqs : D.max_rows;
    c->m_pad_max = (c->max_rows + 31) & ~31;
    c->lse_slots = 2048;
    {   // decoder GEMMs of the throughput path: split-bf16 MFMAs (k_block_x6, the default) or float32 MFMAs (k_block);
        // the environment variable sets the initial mode, irs_set_decoder_gemm() changes it on a live context
        // (an unrecognised value is an error, not a silent default: a typo would otherwise select another arithmetic)
        const char *e = getenv("IRS_DECODER_GEMM");
        if (e && strcmp(e, "f32") && strcmp(e, "x6") && strcmp(e, "h3")) {
            snprintf(g_create_err, sizeof(g_create_err), "IRS_DECODER_GEMM=%s (expected h3, x6 or f32)", e);
            delete c;
            return IRS_E_INVALID;
        }
        c->use_x6 = e ? (strcmp(e, "f32") == 0 ? IRS_GEMM_F32 : strcmp(e, "x6") == 0 ? IRS_GEMM_X6 : IRS_GEMM_H3) : IRS_GEMM_H3;
        const char *ea = getenv("IRS_ATTN_GEMM");
        if (ea && strcmp(ea, "f32") && strcmp(ea, "h3")) {
            snprintf(g_create_err, sizeof(g_create_err), "IRS_ATTN_GEMM=%s (expected h3 or f32)", ea);
            delete c;
            return IRS_E_INVALID;
        }
        c->use_attn_h3 = ea ? (strcmp(ea, "h3") == 0) : 1; // (IRS_ATTN_GEMM=f32: float32 K / V rows and the float32-MFMA attention)
        const char *es = getenv("IRS_DECODER_SEQ");
        c->use_seq = es ? (strcmp(es, "auto") == 0 ? 2 : (atoi(es) != 0 ? 1 : 0)) : 2;
        const char *ed = getenv("IRS_TOPK_DENSE");
        c->use_dense = ed ? (strcmp(ed, "auto") == 0 ? 2 : (atoi(ed) != 0 ? 1 : 0)) : 2;
        const char *ec = getenv("IRS_THR_CARRY"); // steps between two pre-pass + threshold selections inside a path search (0 / 1: every step)
        c->carry_period = ec ? atoi(ec) : 8;
        if (c->carry_period < 0 || c->carry_period > 1024) c->carry_period = 8;
        const char *eo = getenv("IRS_SHARDED_OVERLAP");
        c->sh_overlap = eo ? (atoi(eo) != 0 ? 1 : 0) : 0; // (irs_set_sharded_overlap: off by default)
        const char *er = getenv("IRS_LSE_RING");
        c->lse_no_ring = er ? (strcmp(er, "0") == 0) : 0;
    }
    *out = c;
    return IRS_OK;
}

extern "C" void irs_destroy(irs_ctx *ctx) {
    if (!ctx) return;
    irs_drop_graphs(ctx);
    if (ctx->sh_side) {
        for (int i = 0; i < 8; ++i) (void)hipEventDestroy(ctx->sh_ev[i]);
        (void)hipStreamDestroy(ctx->sh_side);
    }
    if (ctx->prof_ev) {
        for (int i = 0; i < ctx->prof_cap; ++i) {
            hipEventDestroy(ctx->prof_ev[i].a);
            hipEventDestroy(ctx->prof_ev[i].b);
        }
        free(ctx->prof_ev);
    }
    delete ctx;
}

// ------------------------------------------------------------------ weights
extern "C" int irs_bind_weight(irs_ctx *ctx, const char *name, const float *p, int64_t numel) {
    if (!ctx || !name || !p) return IRS_E_INVALID;
    if (strncmp(name, "module.", 7) == 0) name += 7;
    const irs_dims &D = ctx->dims;
    const int64_t d = D.d, F = D.ffn_dim;
    const float **slot = nullptr;
    int64_t want = -1;
    if (!strcmp(name, "item_embedder.weight") || !strcmp(name, "word_embedder.weight")) {
        slot = &ctx->item_emb;
        want = (D.n_item + 1) * d;
    } else if (!strcmp(name, "user_embedder.weight")) {
        slot = &ctx->user_emb;
        want = D.n_user * D.u_dim;
    } else if (!strcmp(name, "pos_embedder.pe")) {
        slot = &ctx->pe;
        want = -2; // >= max_len * d
        if (numel < (int64_t)D.max_len * d) IRS_FAIL(ctx, IRS_E_INVALID, "pos_embedder.pe too small");
    } else if (!strcmp(name, "user_mask_layer.weight")) {
        slot = &ctx->um_w;
        want = D.u_dim;
    } else if (!strcmp(name, "user_mask_layer.bias")) {
        slot = &ctx->um_b;
        want = 1;
    } else if (!strcmp(name, "project.weight")) {
        slot = &ctx->proj_w;
        want = ctx->n_local * d;
    } else if (!strcmp(name, "project.bias")) {
        slot = &ctx->proj_b;
        want = ctx->n_local;
    } else if (!strncmp(name, "decoder.layers.", 15)) {
        char *end = nullptr;
        long l = strtol(name + 15, &end, 10);
        if (l < 0 || l >= D.n_layers || !end || *end != '.') IRS_FAIL(ctx, IRS_E_INVALID, "bad layer in '%s'", name);
        const char *rest = end + 1;
        irs_layer_w &w = ctx->layer[l];
        struct { const char *n; const float **s; int64_t numel; } tab[] = {
            {"self_attn.in_proj_weight", &w.sa_in_w, 3 * d * d}, {"self_attn.in_proj_bias", &w.sa_in_b, 3 * d},
            {"self_attn.out_proj.weight", &w.sa_out_w, d * d},   {"self_attn.out_proj.bias", &w.sa_out_b, d},
            {"multihead_attn.in_proj_weight", &w.ca_in_w, 3 * d * d}, {"multihead_attn.in_proj_bias", &w.ca_in_b, 3 * d},
            {"multihead_attn.out_proj.weight", &w.ca_out_w, d * d},   {"multihead_attn.out_proj.bias", &w.ca_out_b, d},
            {"linear1.weight", &w.l1_w, F * d}, {"linear1.bias", &w.l1_b, F},
            {"linear2.weight", &w.l2_w, d * F}, {"linear2.bias", &w.l2_b, d},
            {"norm1.weight", &w.n1_w, d}, {"norm1.bias", &w.n1_b, d},
            {"norm2.weight", &w.n2_w, d}, {"norm2.bias", &w.n2_b, d},
            {"norm3.weight", &w.n3_w, d}, {"norm3.bias", &w.n3_b, d},
        };
        for (auto &e : tab)
            if (!strcmp(rest, e.n)) {
                slot = e.s;
                want = e.numel;
            }
    }
    if (!slot) IRS_FAIL(ctx, IRS_E_INVALID, "unknown weight '%s'", name);
    if (want >= 0 && numel != want) IRS_FAIL(ctx, IRS_E_INVALID, "weight '%s': numel %lld, expected %lld", name, (long long)numel, (long long)want);
    *slot = p;
    ctx->finalized = false;
    return IRS_OK;
}

static int check_bound(irs_ctx *ctx) {
    const irs_dims &D = ctx->dims;
    if (!ctx->item_emb || !ctx->pe || !ctx->proj_w || !ctx->proj_b) IRS_FAIL(ctx, IRS_E_STATE, "embedding / pe / project weights not bound");
    if (D.mask_mode == IRS_MASK_IRN && (!ctx->user_emb || !ctx->um_w || !ctx->um_b)) IRS_FAIL(ctx, IRS_E_STATE, "user weights not bound");
    for (int l = 0; l < D.n_layers; ++l) {
        const irs_layer_w &w = ctx->layer[l];
        const float *all[] = {w.sa_in_w, w.sa_in_b, w.sa_out_w, w.sa_out_b, w.ca_in_b, w.ca_out_w, w.ca_out_b, w.l1_w,
                              w.l1_b, w.l2_w, w.l2_b, w.n1_w, w.n1_b, w.n2_w, w.n2_b, w.n3_w, w.n3_b};
        for (auto p : all)
            if (!p) IRS_FAIL(ctx, IRS_E_STATE, "decoder layer %d has unbound weights", l);
    }
    return IRS_OK;
}

static size_t derived_plan(const irs_ctx *ctx, size_t *o_wp, size_t *o_bias, size_t *o_cl, size_t *o_wn, size_t *o_wf, size_t *o_x6 = nullptr) {
    size_t off = 0;
    *o_wp = off;
    off = align_up(off + (size_t)ctx->n_tiles * ctx->KS * 1024, 256);
    *o_bias = off;
    off = align_up(off + (size_t)ctx->n_tiles * 32 * sizeof(float), 256);
    *o_cl = off;
    off = align_up(off + (size_t)ctx->dims.n_layers * ctx->dims.d * sizeof(float), 256);
    *o_wn = off;
    off = align_up(off + 256, 256);
    *o_wf = off;
    off = align_up(off + irs_small_frag_floats(ctx) * sizeof(float), 256);
    if (o_x6) *o_x6 = off;
    off = align_up(off + irs_x6_bytes(ctx), 256);
    return off;
}

extern "C" size_t irs_derived_bytes(const irs_ctx *ctx) {
    size_t a, b, c, d, e;
    return ctx ? derived_plan(ctx, &a, &b, &c, &d, &e) : 0;
}

extern "C" int irs_finalize_weights(irs_ctx *ctx, void *arena, size_t bytes, void *stream) {
    if (!ctx || !arena) return IRS_E_INVALID;
    int rc = check_bound(ctx);
    if (rc) return rc;
    size_t o_wp, o_bias, o_cl, o_wn, o_wf, o_x6;
    size_t need = derived_plan(ctx, &o_wp, &o_bias, &o_cl, &o_wn, &o_wf, &o_x6);
    if (bytes < need) IRS_FAIL(ctx, IRS_E_INVALID, "derived arena too small: %zu < %zu", bytes, need);
    if (((uintptr_t)arena) & 255) IRS_FAIL(ctx, IRS_E_INVALID, "derived arena must be 256-byte aligned");
    char *base = (char *)arena;
    ctx->wp = (uint4 *)(base + o_wp);
    ctx->bias_pad = (float *)(base + o_bias);
    ctx->c_l = (float *)(base + o_cl);
    ctx->wnorm_max = (float *)(base + o_wn);
    ctx->w_frag16 = irs_small_frag_floats(ctx) ? (float *)(base + o_wf) : nullptr;
    ctx->w_x6 = irs_x6_bytes(ctx) ? (uint4 *)(base + o_x6) : nullptr;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = irs_launch_pack_w(ctx, s))) return rc;
    if ((rc = irs_launch_cross_const(ctx, s))) return rc;
    if ((rc = irs_launch_pack_small(ctx, s))) return rc;
    if ((rc = irs_launch_pack_x6(ctx, s))) return rc;
    // float16 planes (IRS_GEMM_H3, the V planes of the attention) need every operand below 65504: bound them from the weights,
    // keep half the range as margin; a model outside it runs the split-bf16 kernels (no range limit) -- the one host
    // synchronisation of finalisation
    ctx->h3_ok = true, ctx->h3_bound = 0.f;
    if (ctx->w_x6) {
        float *st = ctx->wnorm_max + 8, hst[8];
        if ((rc = irs_launch_h3_range(ctx, st, s))) return rc;
        IRS_CHECK_HIP(ctx, hipMemcpyAsync(hst, st, sizeof(hst), hipMemcpyDeviceToHost, s));
        IRS_CHECK_HIP(ctx, hipStreamSynchronize(s));
        ctx->h3_bound = irs_h3_operand_bound(ctx, hst);
        ctx->h3_ok = ctx->h3_bound < 32752.f; // (a NaN or infinite statistic fails the comparison)
    }
    ctx->finalized = true;
    ctx->proj_stale = false;
    ctx->thr_valid = 0; // (carried emission thresholds belong to the catalog they were selected on)
    irs_drop_graphs(ctx);
    return IRS_OK;
}

// ------------------------------------------------------------------ workspace
// The one walk over the workspace.  Every buffer is named here once: its irs_ctx field, its size, and its presence condition if it
// has one.  A buffer takes its bytes rounded up to 256; an absent one takes none and is bound to nullptr.  base == nullptr: nothing
// is assigned.  Returns the total.
static size_t workspace_walk(irs_ctx *ctx, char *base) {
    size_t off = 0;
    auto take = [&](auto *&field, size_t bytes, bool present = true) {
        if (base) field = present ? (std::remove_reference_t<decltype(field)>)(base + off) : nullptr;
        if (present) off = align_up(off + bytes, 256);
    };
    const irs_dims &D = ctx->dims;
    const size_t S = ctx->max_seqs, R = ctx->max_rows, mp = ctx->m_pad_max, RL = S * D.max_len;
    // decoder activations
    take(ctx->act_x, RL * D.d * 4);
    take(ctx->act_y, RL * D.d * 4);
    // (the sequence-resident layer kernel pads every sequence to whole 32-token tiles and every workgroup to 8 tiles: up to 256 rows
    //  per sequence in the fragment-major images)
    const bool seq_shape = irs_seq_shape(D);
    const size_t RLs = seq_shape ? S * 256 : RL;
    const size_t RLf = (((RLs > RL ? RLs : RL) + 127) / 128) * 128; // 128-token tiles x 128 padded columns
    const size_t fcols = D.d > 128 ? (size_t)((D.d + 31) / 32) * 32 : 128; // (d = 256: eight column tiles per token tile)
    take(ctx->act_xf, RLf * fcols * 4); // fragment-major copies of x / y (residual inputs of the LN-fused GEMMs)
    take(ctx->act_yf, RLf * fcols * 4);
    take(ctx->act_qkv, RL * 3 * D.d * 4);
    take(ctx->act_qkv_b1, (RL < 256 ? RL : 256) * 3 * D.d * 4); // second q | k | v buffer of the single-sequence fused-attention path
    take(ctx->act_ao, RL * D.d * 4);
    take(ctx->act_h, RL * D.ffn_dim * 4);
    take(ctx->act_ru, S * 4);
    // scoring
    take(ctx->xb, mp * ctx->d_pad * 2);
    take(ctx->eps, mp * 4);
    take(ctx->thr, mp * 4);
    take(ctx->gm, (size_t)IRS_MAX_GROUPS * mp * 4);
    take(ctx->cand_cnt, mp * (size_t)IRS_CAND_BUCKETS * 4);
    take(ctx->cand, mp * (size_t)IRS_CAND_CAP * 8);
    const size_t lse_b = (size_t)ctx->lse_slots * mp * 8, ring_b = (size_t)IRS_LSE_SLOTS_RING * 32 * 8; // (the ring form: <= 32 rows, more slots)
    take(ctx->lse_part, lse_b > ring_b ? lse_b : ring_b);
    take(ctx->ref_tmp, mp * 4);
    // path generation scratch
    take(ctx->xrows, R * D.d * 4);
    take(ctx->top_val, R * D.max_k * 4);
    take(ctx->top_ids, R * D.max_k * 8);
    take(ctx->row_status, R * 4);
    take(ctx->step_ctr, 256); // [0..1] step pair of the path loops, [8..40) arrival counters of k_topk_direct
    take(ctx->pos_tmp, S * 4);
    // beam-search state
    for (irs_beam_state &b : ctx->bm) {
        take(b.seq, RL * 8);
        take(b.hep, S * 4);
        take(b.cum, S * 8);
        take(b.paths, S * IRS_MAX_PATH * 4);
    }
    take(ctx->bm_side[0].user, S * 8);
    take(ctx->lse_max, R * 4);
    take(ctx->lse_sum, R * 4);
    // packed (pad-free) decode plan
    take(ctx->tok_row, RL * 4);
    take(ctx->seq_cnt, S * 4);
    take(ctx->seq_off, S * 4);
    take(ctx->seq_qrow, S * 4);
    take(ctx->seq_padq, S * 4);
    take(ctx->m_dev, 256);
    // plan of the sequence-resident layer kernel
    take(ctx->tile_seq, S * 16 * 4, seq_shape);
    take(ctx->tile_idx, S * 16 * 4, seq_shape);
    take(ctx->seq_row0, S * 4, seq_shape);
    take(ctx->qrow_tile, S * 4, seq_shape);
    take(ctx->n_wg_dev, 256, seq_shape);
    // item-sharded loops (comm.hip): this rank's decoded rows, the exchange buffers, the all-reduced row maxima
    take(ctx->x_local, S * D.d * 4);
    take(ctx->keys_send, R * D.max_k * 8);
    take(ctx->keys_recv, R * D.max_k * 8);
    take(ctx->lse_gmax, R * 4);
    take(ctx->ce_pairs, (size_t)ctx->shard.world * 2 * R * 4); // irs_ce_forward_sharded (ce_sharded.hip)
    // cooperative exhaustive fallback: the recorded rows, and on large shards the per-strip lists
    take(ctx->fb_count, 256);
    take(ctx->fb_list, R * 4);
    take(ctx->exh_keys, (size_t)IRS_EXH_SCRATCH_KEYS * 8, ctx->n_local >= IRS_COOP_FALLBACK_MIN_ITEMS);
    // irs_generate_paths_until: the live users' compacted state
    for (int i = 0; i < 2; ++i) {
        take(ctx->un_seq[i], RL * 8);
        take(ctx->un_user[i], S * 8);
        take(ctx->un_hep[i], S * 4);
        take(ctx->un_map[i], S * 4);
    }
    take(ctx->un_fin, S * 4);
    take(ctx->un_dst, S * 4);
    take(ctx->un_status, S * 4);
    take(ctx->un_stage, S * IRS_MAX_PATH * 4);
    take(ctx->un_count, 256);
    // irs_beam_search_until: the per-row arrays only (24 bytes per sequence)
    take(ctx->bm_side[1].user, S * 8);
    for (int i = 0; i < 2; ++i) {
        take(ctx->bm[i].fin, S * 4);
        take(ctx->bm_side[i].done, S * 4);
    }
    return off;
}

extern "C" size_t irs_workspace_bytes(const irs_ctx *ctx) {
    return ctx ? workspace_walk(const_cast<irs_ctx *>(ctx), nullptr) : 0; // (no base: the walk writes nothing)
}

extern "C" int irs_bind_workspace(irs_ctx *ctx, void *ws, size_t bytes) {
    if (!ctx || !ws) return IRS_E_INVALID;
    const size_t need = workspace_walk(ctx, nullptr);
    if (bytes < need) IRS_FAIL(ctx, IRS_E_INVALID, "workspace too small: %zu < %zu", bytes, need);
    if (((uintptr_t)ws) & 255) IRS_FAIL(ctx, IRS_E_INVALID, "workspace must be 256-byte aligned");
    ctx->ws = (char *)ws;
    ctx->ws_bytes = bytes;
    workspace_walk(ctx, ctx->ws);
    ctx->thr_valid = 0;
    IRS_CHECK_HIP(ctx, hipMemset(ctx->step_ctr, 0, 256));
    irs_drop_graphs(ctx);
    return IRS_OK;
}

// captured steps hold kernel choices, workspace addresses and derived weights: whatever changes one of them drops all three
void irs_drop_graphs(irs_ctx *ctx) {
    for (irs_step_graph *g : {&ctx->g_greedy, &ctx->g_beam, &ctx->g_sharded}) {
        if (g->exec) (void)hipGraphExecDestroy(g->exec);
        g->exec = nullptr;
    }
}

extern "C" int irs_set_decoder_gemm(irs_ctx *ctx, int32_t mode) {
    if (!ctx) return IRS_E_INVALID;
    if (mode != IRS_GEMM_F32 && mode != IRS_GEMM_X6 && mode != IRS_GEMM_H3)
        IRS_FAIL(ctx, IRS_E_INVALID, "decoder GEMM mode %d (IRS_GEMM_F32, IRS_GEMM_X6 or IRS_GEMM_H3)", mode);
    if (ctx->use_x6 != mode) {
        ctx->use_x6 = mode;
        irs_drop_graphs(ctx);
    }
    return IRS_OK;
}

extern "C" int irs_set_decoder_seq(irs_ctx *ctx, int32_t mode) {
    if (!ctx) return IRS_E_INVALID;
    if (mode < 0 || mode > 2) IRS_FAIL(ctx, IRS_E_INVALID, "decoder seq mode %d (0 off, 1 on, 2 auto)", mode);
    if (ctx->use_seq != mode) {
        ctx->use_seq = mode;
        irs_drop_graphs(ctx);
    }
    return IRS_OK;
}
extern "C" int irs_get_decoder_seq(const irs_ctx *ctx) { return ctx ? ctx->use_seq : IRS_E_INVALID; }
extern "C" int irs_decoder_seq_last(const irs_ctx *ctx) { return ctx ? (ctx->seq_last ? 1 : 0) : IRS_E_INVALID; }
extern "C" int irs_set_topk_dense(irs_ctx *ctx, int32_t mode) {
    if (!ctx) return IRS_E_INVALID;
    if (mode < 0 || mode > 2) IRS_FAIL(ctx, IRS_E_INVALID, "top-k dense mode %d (0 off, 1 on, 2 auto)", mode);
    if (ctx->use_dense != mode) {
        ctx->use_dense = mode;
        irs_drop_graphs(ctx); // (a captured step bakes the form in: like every route switch, a change drops the captured steps)
    }
    return IRS_OK;
}
extern "C" int irs_get_topk_dense(const irs_ctx *ctx) { return ctx ? ctx->use_dense : IRS_E_INVALID; }
extern "C" int irs_topk_dense_last(const irs_ctx *ctx) { return ctx ? (ctx->dense_last ? 1 : 0) : IRS_E_INVALID; }
extern "C" int irs_decoder_route_last(const irs_ctx *ctx, int32_t *out, int32_t n) {
    if (!ctx || !out || n < 0) return IRS_E_INVALID;
    if (ctx->route_n == 0) return IRS_E_STATE;
    const int m = n < ctx->route_n ? n : ctx->route_n;
    for (int i = 0; i < m; ++i) out[i] = ctx->route_last[i];
    return m;
}
// (lab / tests: device addresses of decoder workspace buffers, so that a test can look at what a decode left behind)
extern "C" void *irs_debug_ptr(const irs_ctx *ctx, int32_t which) {
    if (!ctx) return nullptr;
    switch (which) {
    case 0: return ctx->act_xf;
    case 1: return ctx->act_yf;
    case 2: return ctx->tile_seq;
    case 3: return ctx->tile_idx;
    case 4: return ctx->seq_row0;
    case 5: return ctx->qrow_tile;
    case 6: return ctx->n_wg_dev;
    case 7: return ctx->seq_off;
    case 8: return ctx->seq_cnt;
    case 9: return ctx->act_qkv;
    case 10: return ctx->seq_qrow;
    default: return nullptr;
    }
}

// the SELECTED mode (what irs_set_decoder_gemm stored: a get / set round trip restores it) ...
extern "C" int irs_get_decoder_gemm(const irs_ctx *ctx) {
    if (!ctx) return IRS_E_INVALID;
    return ctx->use_x6;
}
// ... and the mode that RUNS: a model whose weights fail finalisation's float16 range bound runs IRS_GEMM_X6 where
// IRS_GEMM_H3 is selected
extern "C" int irs_get_decoder_gemm_effective(const irs_ctx *ctx) {
    if (!ctx) return IRS_E_INVALID;
    return (ctx->use_x6 == IRS_GEMM_H3 && ctx->finalized && !ctx->h3_ok) ? IRS_GEMM_X6 : ctx->use_x6;
}
extern "C" float irs_h3_range_bound(const irs_ctx *ctx) { return ctx && ctx->finalized ? ctx->h3_bound : -1.f; }

static int ready(irs_ctx *ctx) {
    if (!ctx) return IRS_E_INVALID;
    if (!ctx->finalized) IRS_FAIL(ctx, IRS_E_STATE, "weights not finalized (irs_finalize_weights)");
    if (!ctx->ws) IRS_FAIL(ctx, IRS_E_STATE, "workspace not bound (irs_bind_workspace)");
    return IRS_OK;
}

// entry points that filter through the bf16 catalog copy and its norms: a training entry point since the last
// irs_finalize_weights means project.* may have moved under them (the filter's |approx - exact| <= eps would not hold)
int irs_ready_filter(irs_ctx *ctx, int sweep) {
    int rc = ready(ctx);
    if (rc) return rc;
    if (ctx->proj_stale && sweep == IRS_SWEEP_BF16)
        IRS_FAIL(ctx, IRS_E_STATE, "project.* may have changed since irs_finalize_weights (irs_ce_forward / irs_ce_grad_logits "
                                   "ran): call irs_finalize_weights before filtering through the bf16 catalog");
    return IRS_OK;
}

// ------------------------------------------------------------------ entry points
extern "C" int irs_pif(irs_ctx *ctx, const int64_t *user, int32_t B, float *r_u, void *stream) {
    int rc = ready(ctx);
    if (rc) return rc;
    if (B < 1 || !r_u) IRS_FAIL(ctx, IRS_E_INVALID, "irs_pif: bad arguments");
    if (ctx->dims.mask_mode == IRS_MASK_IRN && !user) IRS_FAIL(ctx, IRS_E_INVALID, "irs_pif: user is null");
    return irs_launch_pif(ctx, user, B, r_u, (hipStream_t)stream);
}

extern "C" int irs_decode(irs_ctx *ctx, const int64_t *seq, const int64_t *user, int32_t B, float *x, const int32_t *pos,
                          float *xrows, float *r_u, void *stream) {
    int rc = ready(ctx);
    if (rc) return rc;
    if (!seq || B < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_decode: bad arguments");
    if (B > ctx->max_seqs) IRS_FAIL(ctx, IRS_E_INVALID, "irs_decode: B=%d exceeds max_seqs=%d", B, ctx->max_seqs);
    if (ctx->dims.mask_mode == IRS_MASK_IRN && !user) IRS_FAIL(ctx, IRS_E_INVALID, "irs_decode: user is null");
    if ((pos == nullptr) != (xrows == nullptr)) IRS_FAIL(ctx, IRS_E_INVALID, "irs_decode: pos and xrows go together");
    return irs_launch_decode(ctx, seq, user, B, x, pos, xrows, r_u, (hipStream_t)stream);
}

static int check_rows(irs_ctx *ctx, const char *fn, const void *xrows, int M) {
    if (!xrows || M < 1) IRS_FAIL(ctx, IRS_E_INVALID, "%s: bad arguments", fn);
    if (M > ctx->max_rows) IRS_FAIL(ctx, IRS_E_INVALID, "%s: M=%d exceeds max_rows=%d", fn, M, ctx->max_rows);
    return IRS_OK;
}

extern "C" int irs_score_topk_carry(irs_ctx *ctx, const float *xrows, int32_t M, int32_t k, int32_t sweep, float *val,
                                    int64_t *ids0, int32_t *status, void *stream) {
    int rc = irs_ready_filter(ctx, sweep);
    if (rc) return rc;
    if ((rc = check_rows(ctx, "irs_score_topk_carry", xrows, M))) return rc;
    if (k < 1 || k > ctx->dims.max_k || !val || !ids0 || !status) IRS_FAIL(ctx, IRS_E_INVALID, "irs_score_topk_carry: bad k / outputs");
    if (sweep != IRS_SWEEP_BF16) IRS_FAIL(ctx, IRS_E_INVALID, "irs_score_topk_carry: the bf16 filter only");
    return irs_launch_topk(ctx, xrows, M, k, sweep, val, ids0, status, (hipStream_t)stream, nullptr, nullptr, nullptr, 1);
}

extern "C" int irs_score_topk(irs_ctx *ctx, const float *xrows, int32_t M, int32_t k, int32_t sweep, float *val,
                              int64_t *ids0, int32_t *status, void *stream) {
    int rc = irs_ready_filter(ctx, sweep);
    if (rc) return rc;
    if ((rc = check_rows(ctx, "irs_score_topk", xrows, M))) return rc;
    if (k < 1 || k > ctx->dims.max_k || !val || !ids0 || !status) IRS_FAIL(ctx, IRS_E_INVALID, "irs_score_topk: bad k / outputs");
    if (sweep == IRS_SWEEP_EXHAUSTIVE) return irs_launch_topk_exhaustive(ctx, xrows, M, k, val, ids0, status, (hipStream_t)stream);
    if (sweep != IRS_SWEEP_BF16 && sweep != IRS_SWEEP_F32) IRS_FAIL(ctx, IRS_E_INVALID, "irs_score_topk: bad sweep");
    return irs_launch_topk(ctx, xrows, M, k, sweep, val, ids0, status, (hipStream_t)stream);
}

extern "C" int irs_score_gather(irs_ctx *ctx, const float *xrows, int32_t M, const int64_t *ids0, int32_t g, float *out,
                                void *stream) {
    int rc = ready(ctx);
    if (rc) return rc;
    if ((rc = check_rows(ctx, "irs_score_gather", xrows, M))) return rc;
    if (!ids0 || g < 1 || !out) IRS_FAIL(ctx, IRS_E_INVALID, "irs_score_gather: bad arguments");
    return irs_launch_gather(ctx, xrows, M, ids0, g, out, (hipStream_t)stream);
}

extern "C" int irs_score_count_before(irs_ctx *ctx, const float *xrows, int32_t M, const float *ref_score,
                                      const int64_t *ref_id0, const int64_t *excl, int32_t n_excl, int64_t *count,
                                      void *stream) {
    int rc = ready(ctx);
    if (rc) return rc;
    if ((rc = check_rows(ctx, "irs_score_count_before", xrows, M))) return rc;
    if (!ref_score || !ref_id0 || !count || n_excl < 0) IRS_FAIL(ctx, IRS_E_INVALID, "irs_score_count_before: bad arguments");
    return irs_launch_count_before(ctx, xrows, M, ref_score, ref_id0, excl, n_excl, count, (hipStream_t)stream);
}

extern "C" int irs_score_dense(irs_ctx *ctx, const float *xrows, int32_t M, float *out, int64_t ld, void *stream) {
    int rc = ready(ctx);
    if (rc) return rc;
    if ((rc = check_rows(ctx, "irs_score_dense", xrows, M))) return rc;
    if (!out || ld < ctx->n_local) IRS_FAIL(ctx, IRS_E_INVALID, "irs_score_dense: bad out / ld");
    return irs_launch_dense(ctx, xrows, M, out, ld, (hipStream_t)stream);
}

extern "C" int irs_score_lse(irs_ctx *ctx, const float *xrows, int32_t M, float *omax, float *osum, void *stream) {
    int rc = ready(ctx);
    if (rc) return rc;
    if ((rc = check_rows(ctx, "irs_score_lse", xrows, M))) return rc;
    if (!omax || !osum) IRS_FAIL(ctx, IRS_E_INVALID, "irs_score_lse: null outputs");
    return irs_launch_lse(ctx, xrows, M, omax, osum, (hipStream_t)stream);
}

extern "C" int irs_score_topk_lse(irs_ctx *ctx, const float *xrows, int32_t M, int32_t k, int32_t sweep, float *val,
                                  int64_t *ids0, int32_t *status, float *omax, float *osum, void *stream) {
    int rc = irs_ready_filter(ctx, sweep);
    if (rc) return rc;
    if ((rc = check_rows(ctx, "irs_score_topk_lse", xrows, M))) return rc;
    if (k < 1 || k > ctx->dims.max_k || !val || !ids0 || !status || !omax || !osum)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_score_topk_lse: bad k / outputs");
    if (sweep != IRS_SWEEP_BF16 && sweep != IRS_SWEEP_F32) IRS_FAIL(ctx, IRS_E_INVALID, "irs_score_topk_lse: bad sweep");
    return irs_launch_topk(ctx, xrows, M, k, sweep, val, ids0, status, (hipStream_t)stream, nullptr, omax, osum);
}

// ---- projection + cross entropy, training side
extern "C" int irs_ce_forward(irs_ctx *ctx, const float *xrows, const int64_t *labels0, int32_t M, float *lse,
                              float *label_score, double *loss, void *stream) {
    int rc = ready(ctx);
    if (rc) return rc;
    if ((rc = check_rows(ctx, "irs_ce_forward", xrows, M))) return rc;
    if (!labels0 || !lse || !label_score || !loss) IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_forward: null arguments");
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_ce_forward needs the whole catalog on one device");
    hipStream_t s = (hipStream_t)stream;
    ctx->proj_stale = true;
    if ((rc = irs_launch_refresh_bias(ctx, s))) return rc;
    if ((rc = irs_launch_lse(ctx, xrows, M, ctx->lse_max, ctx->lse_sum, s))) return rc;
    if ((rc = irs_launch_lse_combine(ctx, ctx->lse_max, ctx->lse_sum, lse, M, s))) return rc;
    if ((rc = irs_launch_gather(ctx, xrows, M, labels0, 1, label_score, s))) return rc;
    return irs_launch_ce_reduce(ctx, lse, label_score, labels0, M, loss, s);
}

extern "C" int irs_ce_grad_logits(irs_ctx *ctx, const float *xrows, const int64_t *labels0, const float *lse, int32_t M,
                                  float scale, float *out, int64_t ld, void *stream) {
    int rc = ready(ctx);
    if (rc) return rc;
    if ((rc = check_rows(ctx, "irs_ce_grad_logits", xrows, M))) return rc;
    if (!labels0 || !lse || !out || ld < ctx->n_local) IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_grad_logits: bad arguments");
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_ce_grad_logits needs the whole catalog on one device");
    hipStream_t s = (hipStream_t)stream;
    ctx->proj_stale = true;
    if ((rc = irs_launch_refresh_bias(ctx, s))) return rc;
    return irs_launch_ce_grad(ctx, xrows, labels0, lse, M, scale, out, ld, s);
}

extern "C" int irs_merge_topk(irs_ctx *ctx, const float *val_in, const int64_t *ids_in, int32_t W, int32_t M, int32_t k,
                              float *val, int64_t *ids0, void *stream) {
    if (!ctx) return IRS_E_INVALID;
    if (!val_in || !ids_in || !val || !ids0 || W < 1 || M < 1 || k < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_merge_topk: bad arguments");
    return irs_launch_merge(ctx, val_in, ids_in, W, M, k, val, ids0, (hipStream_t)stream);
}

extern "C" int irs_pack_topk(irs_ctx *ctx, const float *val, const int64_t *ids0, int64_t n, uint64_t *keys, void *stream) {
    if (!ctx) return IRS_E_INVALID;
    if (!val || !ids0 || !keys || n < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_pack_topk: bad arguments");
    return irs_launch_pack_topk(ctx, val, ids0, n, keys, (hipStream_t)stream);
}

extern "C" int irs_merge_topk_keys(irs_ctx *ctx, const uint64_t *keys_in, int32_t W, int32_t M, int32_t k, float *val,
                                   int64_t *ids0, void *stream) {
    if (!ctx) return IRS_E_INVALID;
    if (!keys_in || !val || !ids0 || W < 1 || M < 1 || k < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_merge_topk_keys: bad arguments");
    return irs_launch_merge_keys(ctx, keys_in, W, M, k, val, ids0, (hipStream_t)stream);
}

extern "C" int irs_build_eval_batch(irs_ctx *ctx, const int64_t *items, const int64_t *offsets, int32_t B, int32_t raw_len,
                                    int32_t gap_len, const int64_t *targets_in, const int64_t *pool, int64_t n_pool,
                                    uint64_t seed, int64_t *seq, int64_t *target, int64_t *label, int64_t *raw,
                                    int32_t *raw_n, int32_t *status, void *stream) {
    if (!ctx) return IRS_E_INVALID;
    if (!items || !offsets || !seq || !target || !label || B < 1 || raw_len < 1 || gap_len < 0 || (pool && n_pool < 1))
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_build_eval_batch: bad arguments");
    const irs_eval_batch_args a{items, offsets, B, ctx->dims.max_len, raw_len, gap_len, ctx->dims.n_item, targets_in, pool, n_pool, seed,
                               seq, target, label, raw, raw_n, status};
    return irs_launch_build_eval_batch(ctx, a, (hipStream_t)stream);
}

// ------------------------------------------------------------------ bound exclusions (irs_bind_exclusions)
// What a kernel takes of the binding: all zero when nothing is bound.  div: rows per user slot; map: user slot -> bound user;
// paths / path_ld / path_by_user: where a row's path so far lies (used under no_repeat only); the step index for the survivor pass
static irs_excl excl_args(const irs_ctx *ctx, int div, const int32_t *map, const float *paths, int path_ld, int path_by_user,
                          const int32_t *step_ptr, int step_arg) {
    irs_excl e = {};
    const auto &x = ctx->opt.excl;
    if (!x.on) return e;
    e.rows = x.rows, e.cnt = x.cnt, e.stride = x.stride;
    e.map = map, e.div = div;
    if (x.no_repeat) e.paths = paths, e.path_ld = path_ld, e.path_by_user = path_by_user, e.step_ptr = step_ptr, e.step_arg = step_arg;
    e.on = 1;
    return e;
}

// every change of a search option comes here: a captured step holds the kernels and the pointers of the options bound when it
// was captured, or lacks them (irs_internal.h: irs_step_key)
static void opts_changed(irs_ctx *ctx) { irs_drop_graphs(ctx); }

// a caller's scratch: large enough, and aligned for the 16-byte accesses of the kernels that use it
static int check_scratch(irs_ctx *ctx, const char *fn, const void *scratch, size_t bytes, size_t need) {
    if (!scratch || bytes < need) IRS_FAIL(ctx, IRS_E_INVALID, "%s: scratch too small: %zu < %zu", fn, scratch ? bytes : (size_t)0, need);
    if (((uintptr_t)scratch) & 15) IRS_FAIL(ctx, IRS_E_INVALID, "%s: scratch must be 16-byte aligned", fn);
    return IRS_OK;
}

// ------------------------------------------------------------------ which entry point admits which search option
// A search call as the rules see it.  W == 0: a greedy call over B rows; else B * W beam rows.  P: the path length (the steps:
// the step index).  ptrs_ok: none of a loop's required pointers is null
struct search_call {
    int B, W, P, k, sweep, sample, sample_k;
    bool ptrs_ok;
};

// ---- an option's argument checks, where an entry point admits it
// exclusions: the call's users fit the binding; under no_repeat a wave holds the path in one entry per lane
static int check_excl(irs_ctx *ctx, const char *fn, int users, int path_len) {
    const auto &x = ctx->opt.excl;
    if (!x.on) return IRS_OK;
    if (users > x.users) IRS_FAIL(ctx, IRS_E_INVALID, "%s: %d users, exclusions are bound for %d", fn, users, x.users);
    if (x.no_repeat && path_len > IRS_MAX_PATH)
        IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "%s: no_repeat is bound: path length %d > %d", fn, path_len, IRS_MAX_PATH);
    return IRS_OK;
}
static int args_excl(irs_ctx *ctx, const char *fn, const search_call &c) { return check_excl(ctx, fn, c.B, c.P); }
// exact candidates: the bound scratch must serve this call's rows
static int args_surv(irs_ctx *ctx, const char *fn, const search_call &c) {
    const int rows = c.W ? c.B * c.W : c.B, want = irs_opt_choices(ctx->opt, c.W, c.sample, c.sample_k);
    if (want > c.k) IRS_FAIL(ctx, IRS_E_INVALID, "%s: exact candidates need k >= %d", fn, want);
    const size_t need = irs_surv_scratch(ctx, rows, want);
    if (ctx->opt.surv.bytes < need) IRS_FAIL(ctx, IRS_E_INVALID, "%s: bound survivor scratch too small: %zu < %zu", fn, ctx->opt.surv.bytes, need);
    ctx->surv_rows = rows;
    return IRS_OK;
}
static int args_trace(irs_ctx *ctx, const char *fn, const search_call &c) {
    const auto &t = ctx->opt.trace;
    if (c.B > t.users || c.P > t.ld)
        IRS_FAIL(ctx, IRS_E_INVALID, "%s: B=%d / path length %d, the path trace is bound for [%d, %d]", fn, c.B, c.P, t.users, t.ld);
    return IRS_OK;
}
// a guide: the rule is deterministic, and it chooses among k_c candidates of the list
static int args_guide(irs_ctx *ctx, const char *fn, const search_call &c) {
    const int kc = ctx->opt.guide.g.k_c;
    if (c.sample) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "%s: a guide is bound (irs_bind_guide): the guided choice is deterministic, sample must be 0", fn);
    if (c.k < kc) IRS_FAIL(ctx, IRS_E_INVALID, "%s: a guide is bound (irs_bind_guide): k=%d < k_c=%d", fn, c.k, kc);
    return IRS_OK;
}
// a lookahead: the rule is deterministic, it chooses among k_c candidates of the list, and its B * k_c children are decoded and
// scored in one call each
static int args_look(irs_ctx *ctx, const char *fn, const search_call &c) {
    const auto &l = ctx->opt.look;
    if (c.sample) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "%s: a lookahead is bound (irs_bind_lookahead): the choice is deterministic, sample must be 0", fn);
    if (c.k < l.kc) IRS_FAIL(ctx, IRS_E_INVALID, "%s: a lookahead is bound (irs_bind_lookahead): k=%d < k_c=%d", fn, c.k, l.kc);
    if (c.B > l.users) IRS_FAIL(ctx, IRS_E_INVALID, "%s: B=%d, the lookahead is bound for %d users", fn, c.B, l.users);
    if (l.rec_item && c.P > l.ld)
        IRS_FAIL(ctx, IRS_E_INVALID, "%s: path length %d, the lookahead record is bound for %d steps", fn, c.P, l.ld);
    if ((int64_t)c.B * l.kc > ctx->max_seqs || (int64_t)c.B * l.kc > ctx->max_rows)
        IRS_FAIL(ctx, IRS_E_INVALID, "%s: a lookahead is bound (irs_bind_lookahead): B*k_c=%lld exceeds max_seqs=%d / max_rows=%d", fn,
                 (long long)c.B * l.kc, ctx->max_seqs, ctx->max_rows);
    return IRS_OK;
}
// an arrival rule reads what the trace sweep leaves in the bound scratch; one on the admissible rank what k_trace_rank_adm leaves
static int args_arrive(irs_ctx *ctx, const char *fn, const search_call &) {
    if (!ctx->opt.trace.on)
        IRS_FAIL(ctx, IRS_E_STATE, "%s: an arrival rule is set (irs_set_arrival_rule) and no path trace is bound (irs_bind_path_trace): "
                                   "the rule reads what the trace records", fn);
    if (ctx->opt.arrive.kind == IRS_RANK_ADMISSIBLE && !ctx->opt.adm.on)
        IRS_FAIL(ctx, IRS_E_STATE, "%s: an arrival rule on the admissible rank is set (irs_set_arrival_rule_ex, IRS_RANK_ADMISSIBLE) and no "
                                   "admissible rank is bound (irs_bind_trace_admissible): the rule reads what that binding records", fn);
    return IRS_OK;
}
// an admissible rank shares the bound trace's users and ld (irs_bind_trace_admissible), which args_trace has checked
static int args_adm(irs_ctx *ctx, const char *fn, const search_call &) {
    if (!ctx->opt.trace.on) IRS_FAIL(ctx, IRS_E_STATE, "%s: an admissible rank is bound (irs_bind_trace_admissible) without a path trace", fn);
    return IRS_OK;
}
// a beam trace: the call's users, width and path length fit the bound arrays, whose row stride holds the bound W
static int args_btrace(irs_ctx *ctx, const char *fn, const search_call &c) {
    const auto &t = ctx->opt.btrace;
    if (c.B > t.users || c.W != t.W || c.P > t.ld)
        IRS_FAIL(ctx, IRS_E_INVALID, "%s: B=%d / W=%d / path length %d, the beam trace is bound for [%d, %d, %d]", fn, c.B, c.W, c.P,
                 t.users, t.W, t.ld);
    return IRS_OK;
}

// a beam rule reads what the beam trace's sweep leaves in the bound scratch
static int args_brule(irs_ctx *ctx, const char *fn, const search_call &) {
    if (!ctx->opt.btrace.on)
        IRS_FAIL(ctx, IRS_E_STATE, "%s: a beam rule is set (irs_set_beam_rule) and no beam trace is bound (irs_bind_beam_trace): "
                                   "the rule reads what the trace sweep leaves", fn);
    return IRS_OK;
}

// an offer set: one pass of the bound scratch serves the call's rows
static int args_offer(irs_ctx *ctx, const char *fn, const search_call &c) {
    const int rows = c.W ? c.B * c.W : c.B;
    if (rows > ctx->opt.offer.rows)
        IRS_FAIL(ctx, IRS_E_INVALID, "%s: %d rows, the offer set's scratch (irs_bind_offer_set) is sized for %d", fn, rows, ctx->opt.offer.rows);
    return IRS_OK;
}

// a bound sampler: the loop's own sampled step is off, the lists hold its top_k, the records hold the call, and the survivor pass
// repairs a row to at most 32 candidates
static int args_sampler(irs_ctx *ctx, const char *fn, const search_call &c) {
    const auto &m = ctx->opt.sampler;
    if (c.sample) IRS_FAIL(ctx, IRS_E_INVALID, "%s: a sampler is bound (irs_bind_sampler): two samplers, sample must be 0", fn);
    if (c.k < m.top_k) IRS_FAIL(ctx, IRS_E_INVALID, "%s: a sampler is bound (irs_bind_sampler): k=%d < top_k=%d", fn, c.k, m.top_k);
    if ((m.rec_u || m.rec_lq || m.rec_support) && (c.B > m.users || c.P > m.ld))
        IRS_FAIL(ctx, IRS_E_INVALID, "%s: B=%d / path length %d, the sampler's records are bound for [%d, %d]", fn, c.B, c.P, m.users, m.ld);
    if (ctx->opt.surv.scratch && m.top_k > 32)
        IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "%s: a sampler is bound (irs_bind_sampler) with top_k=%d and exact candidates "
                                         "(irs_bind_survivor_scratch) repair a row to at most 32", fn, m.top_k);
    return IRS_OK;
}

// ---- the options, one row each.  greedy: its argument checks where a greedy entry point looks at it.  beam: why the beam entry
// points refuse it ("<fn>: <what>: <beam>"); null: they admit it, with the same argument checks.  sharded: the sharded loops'
// refusal, which every option has (a shard sees its own items only; most bindings refuse a sharded context themselves, so a
// binding cannot exist there, and must not be ignored if it does).  loops_only: why every entry point but the two beam LOOPS
// refuses it (the same message form); null for the options the greedy side admits
enum { OPT_SURV, OPT_EXCL, OPT_TRACE, OPT_GUIDE, OPT_LOOK, OPT_ARRIVE, OPT_BTRACE, OPT_OFFER, OPT_BRULE, OPT_N };
// behind the options that stand alone: an option bound ON TOP of another one, which exists only while that one does.  OPT_ADM
// (irs_bind_trace_admissible) lives and dies with OPT_TRACE, so a row of PLAN that refuses the trace never gets to it
// OPT_SAMPLER (irs_bind_sampler) stands alone; it sits here because it came last
enum { OPT_ADM = OPT_N, OPT_SAMPLER, OPT_ALL };
static const struct {
    bool (*on)(const irs_search_opts &);
    int (*args)(irs_ctx *, const char *, const search_call &);
    const char *what, *beam, *sharded, *loops_only;
} OPTS[OPT_ALL] = {
    {[](const irs_search_opts &o) { return o.surv.scratch != nullptr; }, args_surv, nullptr, nullptr,
     "%s: exact candidates (irs_bind_survivor_scratch) need the whole catalog on one device"},
    {[](const irs_search_opts &o) { return o.excl.on != 0; }, args_excl, nullptr, nullptr,
     "%s: bound exclusions (irs_bind_exclusions) need the whole catalog on one device"},
    {[](const irs_search_opts &o) { return o.trace.on != 0; }, args_trace, "a path trace is bound (irs_bind_path_trace)",
     "greedy and sampled loops only", "%s: a bound path trace (irs_bind_path_trace) needs the whole catalog on one device"},
    {[](const irs_search_opts &o) { return o.guide.on != 0; }, args_guide, "a guide is bound (irs_bind_guide)", "greedy loops only",
     "%s: a bound guide (irs_bind_guide) needs the whole catalog on one device"},
    {[](const irs_search_opts &o) { return o.look.on != 0; }, args_look, "a lookahead is bound (irs_bind_lookahead)", "greedy loops only",
     "%s: a bound lookahead (irs_bind_lookahead) needs the whole catalog on one device"},
    {[](const irs_search_opts &o) { return o.arrive.on != 0; }, args_arrive, "an arrival rule is set (irs_set_arrival_rule)",
     "greedy and sampled loops only", "%s: an arrival rule (irs_set_arrival_rule) is for the single-device greedy and sampled loops"},
    {[](const irs_search_opts &o) { return o.btrace.on != 0; }, args_btrace, "a beam trace is bound (irs_bind_beam_trace)", nullptr,
     "%s: a bound beam trace (irs_bind_beam_trace) needs the whole catalog on one device",
     "irs_beam_search and irs_beam_search_until only"},
    {[](const irs_search_opts &o) { return o.offer.on != 0; }, args_offer, nullptr, nullptr,
     "%s: a bound offer set (irs_bind_offer_set) needs the whole catalog on one device"},
    {[](const irs_search_opts &o) { return o.brule.on != 0; }, args_brule, "a beam rule is set (irs_set_beam_rule)", nullptr,
     "%s: a beam rule (irs_set_beam_rule) needs the whole catalog on one device", "irs_beam_search and irs_beam_search_until only"},
    {[](const irs_search_opts &o) { return o.adm.on != 0; }, args_adm, "an admissible rank is bound (irs_bind_trace_admissible)",
     "greedy and sampled loops only", "%s: a bound admissible rank (irs_bind_trace_admissible) needs the whole catalog on one device"},
    {[](const irs_search_opts &o) { return o.sampler.on != 0; }, args_sampler, "a sampler is bound (irs_bind_sampler)", "greedy loops only",
     "%s: a bound sampler (irs_bind_sampler) needs the whole catalog on one device"},
};

// ---- the entry points, one row each: what it checks, in its order -- the first failing check decides the code and the message.
// The orders differ, and an option that a row does not name is not looked at there; both are behaviour (tests/
// test_search_options_host.py holds every answer).  The loops' rows also hold their common checks: readiness, the whole catalog on
// one device, the call's shape, k.
// A bound beam trace is refused first wherever it is refused (nothing else of the call is looked at); the beam loops look at it
// once the call's shape stands.  AT_BEAM_STEP_LINKED, the trace's own step (irs_beam_step_linked), does not look at it.
// AT_RECOMMEND (irs_recommend / irs_recommend_take) is no search: only the exclusion set applies to it, and no option refuses it.
// A bound offer set is looked at last by the loops; the standalone steps and irs_recommend_take are kernels on the caller's
// lists and do not look at it (irs_recommend, which ranks inside the set, makes the set's argument check itself).  The set's
// sharded refusal is defensive: irs_bind_offer_set refuses a sharded context, so no test can reach it.
// A beam rule (irs_set_beam_rule) is refused right behind a bound beam trace wherever that is refused, and by irs_beam_step_linked;
// the beam loops look at it (is a beam trace bound?) behind the arrival rule and before readiness, so that a rule without a trace
// is answered before anything else of the call.  AT_BEAM_STEP_RULED, the rule's own step (irs_beam_step_ruled), takes the rule as
// arguments and looks at neither.
// A bound sampler (irs_bind_sampler) is looked at right behind the lookahead wherever that is: the greedy loops check its
// arguments there, the beam entry points and the sharded loops refuse it.  irs_path_step alone does not look at it.
// A bound admissible rank (irs_bind_trace_admissible) exists only while a path trace is bound, so every row that refuses the
// trace has refused it already; the greedy loops look at it right behind the trace.  irs_path_step looks at neither.
enum { AT_GREEDY_LOOP, AT_PATH_STEP, AT_BEAM_STEP, AT_BEAM_LOOP, AT_SHARDED_LOOP, AT_BEAM_STEP_LINKED, AT_RECOMMEND, AT_BEAM_STEP_RULED };
enum { DO_READY = OPT_ALL, DO_WORLD, DO_SHAPE, DO_K, DO_END };
static const int PLAN[][20] = {
    /* AT_GREEDY_LOOP  */ {OPT_BTRACE, OPT_BRULE, OPT_ARRIVE, OPT_GUIDE, OPT_LOOK, OPT_SAMPLER, DO_READY, DO_WORLD, DO_SHAPE, OPT_TRACE, OPT_ADM, DO_K, OPT_EXCL, OPT_SURV, OPT_OFFER, DO_END},
    /* AT_PATH_STEP    */ {OPT_BTRACE, OPT_BRULE, OPT_EXCL, OPT_GUIDE, DO_END},
    /* AT_BEAM_STEP    */ {OPT_BTRACE, OPT_BRULE, OPT_TRACE, OPT_GUIDE, OPT_LOOK, OPT_SAMPLER, OPT_EXCL, DO_END},
    /* AT_BEAM_LOOP    */ {OPT_GUIDE, OPT_LOOK, OPT_SAMPLER, OPT_ARRIVE, OPT_BRULE, DO_READY, DO_WORLD, OPT_TRACE, DO_SHAPE, OPT_BTRACE, DO_K, OPT_EXCL, OPT_SURV, OPT_OFFER, DO_END},
    /* AT_SHARDED_LOOP */ {OPT_BTRACE, OPT_BRULE, OPT_SURV, OPT_EXCL, OPT_TRACE, OPT_GUIDE, OPT_LOOK, OPT_SAMPLER, OPT_ARRIVE, OPT_OFFER, DO_END},
    /* AT_BEAM_STEP_LINKED */ {OPT_BRULE, OPT_TRACE, OPT_GUIDE, OPT_LOOK, OPT_SAMPLER, OPT_EXCL, DO_END},
    /* AT_RECOMMEND    */ {OPT_EXCL, DO_END},
    /* AT_BEAM_STEP_RULED */ {OPT_TRACE, OPT_GUIDE, OPT_LOOK, OPT_SAMPLER, OPT_EXCL, DO_END},
};
static int search_rules(irs_ctx *ctx, const char *fn, int at, const search_call &c) {
    const bool beam = at == AT_BEAM_STEP || at == AT_BEAM_LOOP || at == AT_BEAM_STEP_LINKED || at == AT_BEAM_STEP_RULED;
    int rc;
    for (const int *p = PLAN[at]; *p != DO_END; ++p) {
        switch (*p) {
        case DO_READY:
            if ((rc = irs_ready_filter(ctx, c.sweep))) return rc;
            break;
        case DO_WORLD:
            if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "%s needs the whole catalog on one device", fn);
            break;
        case DO_SHAPE:
            if (beam) {
                if ((rc = irs_check_beam_args(ctx, fn, c.ptrs_ok, c.B, c.W, c.P))) return rc;
                if ((int64_t)c.B * c.W > ctx->max_seqs || (int64_t)c.B * c.W > ctx->max_rows)
                    IRS_FAIL(ctx, IRS_E_INVALID, "%s: B*W=%d exceeds max_seqs=%d / max_rows=%d", fn, c.B * c.W, ctx->max_seqs, ctx->max_rows);
            } else {
                if (!c.ptrs_ok || c.B < 1 || c.P < 1) IRS_FAIL(ctx, IRS_E_INVALID, "%s: bad arguments", fn);
                if (c.B > ctx->max_seqs || c.B > ctx->max_rows) IRS_FAIL(ctx, IRS_E_INVALID, "%s: B too large", fn);
            }
            break;
        case DO_K:
            if ((rc = irs_check_k(ctx, fn, c.k, 1, c.sweep, c.sample, c.sample_k))) return rc;
            break;
        default: {
            const auto &o = OPTS[*p];
            if (!o.on(ctx->opt)) break;
            if (at == AT_SHARDED_LOOP) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, o.sharded, fn);
            if (o.loops_only && at != AT_BEAM_LOOP) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "%s: %s: %s", fn, o.what, o.loops_only);
            if (beam && o.beam) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "%s: %s: %s", fn, o.what, o.beam);
            if ((rc = o.args(ctx, fn, c))) return rc;
        }
        }
    }
    return IRS_OK;
}
int irs_sharded_option_rules(irs_ctx *ctx, const char *fn) { return search_rules(ctx, fn, AT_SHARDED_LOOP, search_call{}); }

extern "C" size_t irs_exclusion_scratch_bytes(const irs_ctx *ctx, int32_t users, int32_t n_excl) {
    if (!ctx || users < 1 || n_excl < 0 || n_excl > IRS_MAX_EXCL) return 0;
    return irs_excl_scratch(users, n_excl);
}

extern "C" int irs_bind_exclusions(irs_ctx *ctx, const int64_t *excl_ids0, int32_t users, int32_t n_excl, int32_t no_repeat,
                                   void *scratch, size_t bytes, void *stream) {
    if (!ctx) return IRS_E_INVALID;
    if (!excl_ids0 && users == 0 && n_excl == 0 && !no_repeat && !scratch && bytes == 0) { // unbind
        if (ctx->opt.excl.on) opts_changed(ctx);
        ctx->opt.excl = {};
        return IRS_OK;
    }
    if (n_excl < 0) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_exclusions: n_excl must be >= 0");
    if (n_excl > IRS_MAX_EXCL) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_exclusions: n_excl %d > %d", n_excl, IRS_MAX_EXCL);
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_exclusions needs the whole catalog on one device");
    if (users < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_exclusions: users must be >= 1");
    if ((excl_ids0 == nullptr) != (n_excl == 0)) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_exclusions: a list and n_excl >= 1 go together");
    if (n_excl == 0 && !no_repeat) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_exclusions: neither a list nor no_repeat");
    int rc = check_scratch(ctx, "irs_bind_exclusions", scratch, bytes, irs_excl_scratch(users, n_excl));
    if (rc) return rc;
    if ((rc = irs_launch_excl_prepare(ctx, excl_ids0, users, n_excl, scratch, (hipStream_t)stream))) return rc;
    ctx->opt.excl.on = 1, ctx->opt.excl.users = users, ctx->opt.excl.no_repeat = no_repeat ? 1 : 0;
    opts_changed(ctx);
    return IRS_OK;
}

// ------------------------------------------------------------------ offer set (irs_bind_offer_set; offer_set.hip)
static bool offer_shape_ok(const irs_ctx *ctx, int64_t n_ids, int rows) {
    return n_ids >= 1 && n_ids <= ctx->dims.n_item && rows >= 1 && rows <= ctx->max_rows;
}

extern "C" size_t irs_offer_set_scratch_bytes(const irs_ctx *ctx, int64_t n_ids, int32_t rows) {
    if (!ctx || !offer_shape_ok(ctx, n_ids, rows)) return 0;
    return irs_offer_layout(nullptr, n_ids, rows, nullptr);
}

// Neither entry point takes a stream: their launches are enqueued on the null stream and the call returns without waiting, as
// irs_recommend's are (irs_hip.h)
extern "C" int irs_bind_offer_set(irs_ctx *ctx, const int64_t *ids0, int64_t n_ids, void *scratch, size_t bytes) {
    if (!ctx) return IRS_E_INVALID;
    const char *fn = "irs_bind_offer_set";
    if (!ids0 && n_ids == 0) { // unbind
        if (ctx->opt.offer.on) opts_changed(ctx);
        ctx->opt.offer = {};
        return IRS_OK;
    }
    if (!ids0) IRS_FAIL(ctx, IRS_E_INVALID, "%s: an id array and n_ids >= 1 go together", fn);
    if (n_ids < 1 || n_ids > ctx->dims.n_item) IRS_FAIL(ctx, IRS_E_INVALID, "%s: n_ids must be in [1, n_item=%lld]", fn, (long long)ctx->dims.n_item);
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "%s needs the whole catalog on one device", fn);
    int rc = check_scratch(ctx, fn, scratch, bytes, irs_offer_layout(nullptr, n_ids, 1, nullptr));
    if (rc) return rc;
    // the rows of a pass: what the scratch holds behind the ids, at most max_rows
    irs_offer_rows o;
    const size_t head = irs_offer_layout(scratch, n_ids, 0, &o);
    const size_t fit = (bytes - head) / ((size_t)o.c_pad * sizeof(float));
    const int rows = fit < (size_t)ctx->max_rows ? (int)fit : ctx->max_rows;
    if ((rc = irs_launch_offer_prepare(ctx, ids0, n_ids, o, nullptr))) return rc;
    ctx->opt.offer = {1, o.ids, n_ids, scratch, rows};
    opts_changed(ctx);
    return IRS_OK;
}

extern "C" int irs_score_topk_offer(irs_ctx *ctx, const float *xrows, int32_t M, int32_t k, float *val, int64_t *ids0, int32_t *status) {
    // (the argument checks first: k bounds the selection's LDS buffer, and a context without weights can be asked about them)
    if (!ctx) return IRS_E_INVALID;
    int rc = check_rows(ctx, "irs_score_topk_offer", xrows, M);
    if (rc) return rc;
    if (k < 1 || k > ctx->dims.max_k) IRS_FAIL(ctx, IRS_E_INVALID, "irs_score_topk_offer: k must be in [1, %d]", ctx->dims.max_k);
    if (!val || !ids0 || !status) IRS_FAIL(ctx, IRS_E_INVALID, "irs_score_topk_offer: null output");
    if ((rc = ready(ctx))) return rc;
    if (!ctx->opt.offer.on) IRS_FAIL(ctx, IRS_E_STATE, "irs_score_topk_offer: no offer set is bound (irs_bind_offer_set)");
    return irs_launch_offer_topk(ctx, xrows, M, k, val, ids0, status, nullptr);
}

// ------------------------------------------------------------------ bound guide (irs_bind_guide; guide.hip)
extern "C" size_t irs_guide_scratch_bytes(const irs_ctx *ctx, int32_t kind, int32_t F) {
    if (!ctx || kind != IRS_GUIDE_BINARY || F < 1 || F > IRS_MAX_GUIDE_BITS) return 0; // (a float table is read where it lies)
    return irs_guide_scratch(ctx->dims.n_item, kind, F);
}

extern "C" int irs_bind_guide(irs_ctx *ctx, int32_t kind, const void *table, int32_t F, int32_t k_c, void *scratch, size_t bytes,
                              void *stream) {
    if (!ctx) return IRS_E_INVALID;
    if (!table) { // unbind
        if (ctx->opt.guide.on) opts_changed(ctx);
        ctx->opt.guide = {};
        return IRS_OK;
    }
    if (kind != IRS_GUIDE_BINARY && kind != IRS_GUIDE_FLOAT)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_guide: kind %d (IRS_GUIDE_BINARY or IRS_GUIDE_FLOAT)", kind);
    if (F < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_guide: F must be >= 1");
    if (k_c < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_guide: k_c must be >= 1");
    if (k_c > IRS_MAX_GUIDE_KC) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_guide: k_c %d > %d", k_c, IRS_MAX_GUIDE_KC);
    const int f_max = kind == IRS_GUIDE_BINARY ? IRS_MAX_GUIDE_BITS : IRS_MAX_GUIDE_FLOATS;
    if (F > f_max) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_guide: F %d > %d (%s)", F, f_max, kind == IRS_GUIDE_BINARY ? "bits" : "floats");
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_guide needs the whole catalog on one device");
    if (ctx->opt.look.on) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_guide: a lookahead is bound (irs_bind_lookahead): one choice rule at a time");
    if (ctx->opt.sampler.on) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_guide: a sampler is bound (irs_bind_sampler): one choice rule at a time");
    if (k_c > ctx->dims.max_k) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_guide: k_c %d > max_k %d", k_c, ctx->dims.max_k);
    const int64_t rows = ctx->dims.n_item + 1;
    irs_guide g{table, rows, F, 0, k_c, kind};
    if (kind == IRS_GUIDE_BINARY) {
        int rc = check_scratch(ctx, "irs_bind_guide", scratch, bytes, irs_guide_scratch(ctx->dims.n_item, kind, F));
        if (rc) return rc;
        g.words = (F + 31) / 32, g.table = scratch;
        if ((rc = irs_launch_guide_pack(ctx, (const uint8_t *)table, rows, F, (uint32_t *)scratch, (hipStream_t)stream))) return rc;
    } else if (((uintptr_t)table) & 3) {
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_guide: a float table must be 4-byte aligned");
    }
    ctx->opt.guide.g = g, ctx->opt.guide.on = 1;
    opts_changed(ctx);
    return IRS_OK;
}

// ------------------------------------------------------------------ bound lookahead (irs_bind_lookahead; lookahead.hip)
extern "C" size_t irs_lookahead_scratch_bytes(const irs_ctx *ctx, int32_t rows, int32_t k_c) {
    if (!ctx || rows < 1 || k_c < 1 || k_c > IRS_MAX_LOOKAHEAD_KC) return 0;
    return irs_look_layout(nullptr, rows, k_c, ctx->dims.max_len, ctx->dims.d, nullptr);
}

extern "C" int irs_bind_lookahead(irs_ctx *ctx, int32_t k_c, void *scratch, size_t bytes, int32_t *rec_item, float *rec_lp,
                                  int32_t users, int32_t ld) {
    if (!ctx) return IRS_E_INVALID;
    if (k_c == 0) { // unbind
        if (ctx->opt.look.on) opts_changed(ctx);
        ctx->opt.look = {};
        return IRS_OK;
    }
    if (k_c < 0 || k_c > IRS_MAX_LOOKAHEAD_KC) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_lookahead: k_c %d outside [0, %d]", k_c, IRS_MAX_LOOKAHEAD_KC);
    if (users < 1 || ld < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_lookahead: users >= 1 and ld >= 1");
    if ((rec_item == nullptr) != (rec_lp == nullptr)) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_lookahead: the two record arrays go together");
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_lookahead needs the whole catalog on one device");
    if (ctx->opt.guide.on) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_lookahead: a guide is bound (irs_bind_guide): one choice rule at a time");
    if (ctx->opt.sampler.on) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_lookahead: a sampler is bound (irs_bind_sampler): one choice rule at a time");
    const int rc = check_scratch(ctx, "irs_bind_lookahead", scratch, bytes, irs_look_layout(nullptr, users, k_c, ctx->dims.max_len, ctx->dims.d, nullptr));
    if (rc) return rc;
    ctx->opt.look = {1, k_c, users, ld, scratch, rec_item, rec_lp};
    opts_changed(ctx);
    return IRS_OK;
}

// The two kernels alone (tests, and replaying a recorded decision from arrays): SYNCHRONOUS calls.  They take no stream: the
// kernel is launched on the null stream and the call returns when it has finished, so nothing of it is in flight between calls
// and there is no stream order for a caller to keep (include/irs_hip.h).  What the two entry points share:
static int look_run_sync(irs_ctx *ctx, int rc) {
    if (rc) return rc;
    IRS_CHECK_HIP(ctx, hipStreamSynchronize(nullptr));
    return IRS_OK;
}
static int check_look_call(irs_ctx *ctx, const char *fn, bool ptrs_ok, int M, int k, int k_c) {
    if (!ptrs_ok) IRS_FAIL(ctx, IRS_E_INVALID, "%s: null pointer", fn);
    if (M < 1) IRS_FAIL(ctx, IRS_E_INVALID, "%s: M must be >= 1", fn);
    if (k < 1 || k > ctx->dims.max_k) IRS_FAIL(ctx, IRS_E_INVALID, "%s: k must be in [1, %d]", fn, ctx->dims.max_k);
    if (k_c < 1 || k_c > k || k_c > IRS_MAX_LOOKAHEAD_KC)
        IRS_FAIL(ctx, IRS_E_INVALID, "%s: k_c must be in [1, min(k, %d)]", fn, IRS_MAX_LOOKAHEAD_KC);
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "%s needs the whole catalog on one device", fn);
    return IRS_OK;
}

extern "C" int irs_lookahead_expand(irs_ctx *ctx, const int64_t *seq, const int32_t *hep, const int64_t *user, int32_t M, const float *val,
                                    const int64_t *ids0, int32_t k, int32_t k_c, const int32_t *fin, const float *paths, int32_t path_ld,
                                    int32_t step, const int32_t *row_map, int64_t *child_seq, int32_t *child_hep, int64_t *child_user,
                                    int64_t *child_target0, int64_t *cand_ids0, float *cand_val) {
    if (!ctx) return IRS_E_INVALID;
    int rc = check_look_call(ctx, "irs_lookahead_expand",
                             seq && hep && val && ids0 && child_seq && child_hep && child_user && child_target0 && cand_ids0 && cand_val, M, k, k_c);
    if (rc) return rc;
    if (ctx->dims.mask_mode == IRS_MASK_IRN && !user) IRS_FAIL(ctx, IRS_E_INVALID, "irs_lookahead_expand: user is null");
    if (step < 0 || (paths && (path_ld < 1 || step > path_ld)))
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_lookahead_expand: step must be in [0, path_ld], path_ld >= 1");
    if (ctx->opt.excl.on && ctx->opt.excl.no_repeat && !paths) IRS_FAIL(ctx, IRS_E_INVALID, "irs_lookahead_expand: no_repeat is bound: dev_paths is null");
    if ((rc = check_excl(ctx, "irs_lookahead_expand", M, step))) return rc;
    const irs_look_expand_args a{seq, hep, user, M, ctx->dims.max_len, k, k_c, val, ids0, fin, nullptr, step,
                                 excl_args(ctx, 1, row_map, paths, path_ld, 1, nullptr, step),
                                 child_seq, child_user, child_target0, cand_ids0, child_hep, cand_val};
    return look_run_sync(ctx, irs_launch_lookahead_expand(ctx, a, nullptr));
}

extern "C" int irs_lookahead_choose(irs_ctx *ctx, const int64_t *seq, int32_t M, int32_t k_c, const int64_t *cand_ids0, const float *cand_val,
                                    const float *mx, const float *sm, const float *tscore, const int32_t *fin, float *val, int64_t *ids0,
                                    int32_t k, float *lp, int32_t *choice) {
    if (!ctx) return IRS_E_INVALID;
    const int rc = check_look_call(ctx, "irs_lookahead_choose", seq && cand_ids0 && cand_val && mx && sm && tscore && val && ids0 && lp && choice,
                                   M, k, k_c);
    if (rc) return rc;
    const irs_look_choose_args a{seq, M, ctx->dims.max_len, k, k_c, cand_ids0, cand_val, mx, sm, tscore, fin, val, ids0, lp, choice,
                                 nullptr, nullptr, 0, nullptr, nullptr};
    return look_run_sync(ctx, irs_launch_lookahead_choose(ctx, a, nullptr));
}

// ------------------------------------------------------------------ bound sampler (irs_bind_sampler; sampler.hip)
extern "C" int irs_bind_sampler(irs_ctx *ctx, int32_t top_k, float temperature, float top_p, float *rec_u, float *rec_lq,
                                int32_t *rec_support, int32_t users, int32_t ld) {
    if (!ctx) return IRS_E_INVALID;
    if (top_k == 0) { // unbind
        if (ctx->opt.sampler.on) opts_changed(ctx);
        ctx->opt.sampler = {};
        return IRS_OK;
    }
    const int k_max = ctx->dims.max_k < IRS_MAX_SAMPLER_K ? ctx->dims.max_k : IRS_MAX_SAMPLER_K;
    if (!(temperature > 0.f) || temperature - temperature != 0.f)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_sampler: temperature %g must be finite and > 0", (double)temperature);
    if (!(top_p > 0.f && top_p <= 1.f)) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_sampler: top_p %g outside (0, 1]", (double)top_p);
    if (top_k < 1 || top_k > k_max) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_sampler: top_k %d outside [1, %d]", top_k, k_max);
    if ((rec_u || rec_lq || rec_support) && (users < 1 || ld < 1))
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_sampler: a record needs users >= 1 and ld >= 1");
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_sampler needs the whole catalog on one device");
    if (ctx->opt.guide.on) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_sampler: a guide is bound (irs_bind_guide): one choice rule at a time");
    if (ctx->opt.look.on) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_sampler: a lookahead is bound (irs_bind_lookahead): one choice rule at a time");
    const bool rec = rec_u || rec_lq || rec_support;
    ctx->opt.sampler = {1, top_k, temperature, 1.0f / temperature, top_p, rec_u, rec_lq, rec_support, rec ? users : 0, rec ? ld : 0};
    opts_changed(ctx);
    return IRS_OK;
}

// the kernel's arguments under the bound parameters: the loops' (step_ptr = the device counter) and the entry point's alike
static irs_sampler_args sampler_args(const irs_ctx *ctx, const int64_t *seq, const int32_t *hep, int M, float *val, int64_t *ids0, int k,
                                     const int32_t *fin, const int32_t *status, const int32_t *row_ids, const int32_t *step_ptr,
                                     int step, uint64_t seed, const irs_excl &ex) {
    const auto &m = ctx->opt.sampler;
    return irs_sampler_args{seq, hep, M, ctx->dims.max_len, k, m.top_k, m.inv_t, m.top_p, val, ids0, fin, status, row_ids, step_ptr, step,
                            (unsigned long long)seed, m.rec_u, m.rec_lq, m.rec_support, m.users, m.ld, ex};
}

extern "C" int irs_sampler_choose(irs_ctx *ctx, const int64_t *seq, const int32_t *hep, int32_t M, float *val, int64_t *ids0, int32_t k,
                                  int32_t step, uint64_t seed, const int32_t *row_ids, const int32_t *status, const int32_t *fin,
                                  const float *paths, int32_t path_ld) {
    if (!ctx) return IRS_E_INVALID;
    const char *fn = "irs_sampler_choose";
    if (!ctx->opt.sampler.on) IRS_FAIL(ctx, IRS_E_STATE, "%s: no sampler is bound (irs_bind_sampler)", fn);
    if (!seq || !hep || !val || !ids0 || !status) IRS_FAIL(ctx, IRS_E_INVALID, "%s: null pointer", fn);
    if (M < 1) IRS_FAIL(ctx, IRS_E_INVALID, "%s: M must be >= 1", fn);
    if (k < ctx->opt.sampler.top_k || k > ctx->dims.max_k)
        IRS_FAIL(ctx, IRS_E_INVALID, "%s: k must be in [top_k=%d, %d]", fn, ctx->opt.sampler.top_k, ctx->dims.max_k);
    if (step < 0 || (paths && (path_ld < 1 || step > path_ld))) IRS_FAIL(ctx, IRS_E_INVALID, "%s: step must be in [0, path_ld], path_ld >= 1", fn);
    if (ctx->opt.excl.on && ctx->opt.excl.no_repeat && !paths) IRS_FAIL(ctx, IRS_E_INVALID, "%s: no_repeat is bound: dev_paths is null", fn);
    const int rc = check_excl(ctx, fn, M, step);
    if (rc) return rc;
    // (synchronous, on the null stream, like the two lookahead kernels alone: irs_hip.h)
    return look_run_sync(ctx, irs_launch_sampler_choose(ctx, sampler_args(ctx, seq, hep, M, val, ids0, k, fin, status, row_ids, nullptr, step,
                                                                          seed, excl_args(ctx, 1, row_ids, paths, path_ld, 1, nullptr, step)),
                                                        nullptr));
}

extern "C" int irs_path_step(irs_ctx *ctx, int64_t *seq, int32_t *hep, int32_t B, const float *val, const int64_t *ids0,
                             int32_t k, int32_t step, float *paths, int32_t path_ld, int32_t sample, int32_t sample_k,
                             uint64_t seed, int32_t *status, void *stream) {
    if (!ctx) return IRS_E_INVALID;
    if (!seq || !hep || !val || !ids0 || !paths || !status || B < 1 || k < 1 || step < 0 || step >= path_ld)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_path_step: bad arguments");
    if (sample && (sample_k < 1 || sample_k > IRS_MAX_SAMPLE_K))
        IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_path_step: sample_k must be in [1, %d]", IRS_MAX_SAMPLE_K);
    const int rc = search_rules(ctx, "irs_path_step", AT_PATH_STEP, search_call{B, 0, step, k, 0, sample, sample_k, true});
    if (rc) return rc;
    const irs_path_args pa{seq, hep, ctx->dims.max_len, paths, path_ld, sample, sample_k, seed, status, nullptr, step, nullptr, 1,
                           excl_args(ctx, 1, nullptr, paths, path_ld, 1, nullptr, step)};
    return irs_launch_path_step(ctx, pa, B, val, ids0, k, (hipStream_t)stream);
}

// The ranked lists a step or a slate starts from.  Nothing bound: irs_launch_topk as it always was.  An offer set bound: the best k
// of the set from its own launcher, and where the caller needs the rows' (max, sum exp) they are irs_launch_lse's over the whole
// catalog -- the set restricts offers, not the softmax.  No threshold carry applies then, and the thr_* state is not touched.
static int launch_lists(irs_ctx *ctx, const float *xrows, int M, int k, int sweep, float *val, int64_t *ids0, int32_t *status, hipStream_t s,
                        float *lse_max, float *lse_sum, int carry) {
    if (!ctx->opt.offer.on) return irs_launch_topk(ctx, xrows, M, k, sweep, val, ids0, status, s, nullptr, lse_max, lse_sum, carry);
    const int rc = irs_launch_offer_topk(ctx, xrows, M, k, val, ids0, status, s);
    if (rc || !lse_max) return rc;
    return irs_launch_lse(ctx, xrows, M, lse_max, lse_sum, s);
}

// one search step on one device: decode -> rows at hep -> top-k -> choose/update.  `pa` is the loop's (loop_path_args): the step
// index comes from the device counter
// surv_fin (may be null): rows the survivor pass skips -- the until loop's finished rows, stepped until the next compaction
// row_map (may be null: the identity): compacted row -> the caller's row, for the bound path trace, which also skips surv_fin's rows
static int enqueue_step(irs_ctx *ctx, irs_path_args pa, const int64_t *user, int B, int k, int sweep, hipStream_t s, int carry = 0,
                        const int32_t *surv_fin = nullptr, const int32_t *row_map = nullptr) {
    int rc;
    const bool merged = irs_small_plan(ctx->dims, B); // (the decode below is rows-only: its plan is the single-workgroup one)
    pa.step_next = merged ? ctx->step_ctr + 1 : nullptr;
    ctx->step_pair = merged ? ctx->step_ctr : nullptr;
    rc = irs_launch_decode(ctx, pa.seq, user, B, nullptr, pa.hep, ctx->xrows, nullptr, s);
    ctx->step_pair = nullptr;
    if (rc) return rc;
    // small shard, few rows: the workgroup that ranks a row's candidates also takes the row's path step
    // (not while exact candidates are bound: the survivor pass goes between the ranking and the step; nor while exclusions are
    //  bound: only the separate step kernel has the form that tests them; nor while a path trace is bound: its sweep reads the
    //  window before the step, its record kernel the lists after it; nor while a guide is bound: the guided step is a kernel of its own;
    //  nor while a lookahead is bound: its expand, inner decode and choose go between the ranking and the step; nor while an offer
    //  set is bound: the lists come from its own launcher; nor while a sampler is bound: its choice goes in front of the step)
    if (merged && !irs_opt_splits_step(ctx->opt) && sweep != IRS_SWEEP_EXHAUSTIVE && irs_topk_is_direct(ctx, B, k))
        return irs_launch_topk(ctx, ctx->xrows, B, k, sweep, ctx->top_val, ctx->top_ids, ctx->row_status, s, &pa);
    if ((rc = launch_lists(ctx, ctx->xrows, B, k, sweep, ctx->top_val, ctx->top_ids, ctx->row_status, s, nullptr, nullptr, carry))) return rc;
    const irs_search_opts &o = ctx->opt;
    if (o.surv.scratch) {
        const irs_surv_args sa{ctx->xrows, pa.seq, pa.hep, B, 1, k, irs_opt_choices(o, 0, pa.sample, pa.sample_k), ctx->surv_rows, nullptr,
                               surv_fin, nullptr, ctx->top_val, ctx->top_ids, pa.status, nullptr, pa.ex};
        if ((rc = irs_launch_survivors(ctx, sa, o.surv.scratch, s))) return rc;
    }
    irs_trace_rows tr = {};
    if (o.trace.on) { // how the target stands before the step chooses: into the scratch, by launch row
        irs_trace_layout(o.trace.scratch, o.trace.users, &tr);
        if ((rc = irs_launch_target_trace(ctx, ctx->xrows, pa.seq, pa.hep, B, tr, tr.mx, tr.sm, tr.ts, tr.rank, s))) return rc;
    }
    // admissible rank: the trace's rank among what the step may offer -- behind the sweep, before anything rewrites the lists; the
    // value goes to the scratch by launch row and to the caller's cell of this step, where the record kernel writes rank_target.
    // A bound offer set's scores are those of this step's ranking: launch_lists wrote them for these B rows (one pass: args_offer),
    // and neither the survivor pass (its own scratch) nor the trace sweep (the trace scratch, ctx->lse_part) writes them
    const int32_t *arrive_rank = tr.rank;
    if (o.adm.on) {
        irs_adm_args aa = {ctx->xrows, pa.seq, pa.hep, B, tr.ts, tr.refid, tr.count, pa.ex};
        if (o.offer.on) {
            irs_offer_rows of;
            irs_offer_layout(o.offer.scratch, o.offer.n, o.offer.rows, &of);
            aa.oids = of.ids, aa.on = o.offer.n, aa.oc_pad = of.c_pad, aa.osc = of.sc, aa.oholes = of.holes;
        }
        aa.out = (int32_t *)o.adm.scratch;
        aa.rec = o.adm.rank, aa.rec_ld = o.trace.ld, aa.rec_map = row_map, aa.rec_fin = surv_fin, aa.rec_step = ctx->step_ctr;
        if ((rc = irs_launch_trace_rank_adm(ctx, aa, s))) return rc;
        if (o.arrive.kind == IRS_RANK_ADMISSIBLE) arrive_rank = aa.out;
    }
    // arrival rule: a row whose target stands well enough is offered the target alone (the entry points have seen to the trace)
    if (o.arrive.on && (rc = irs_launch_arrival_offer(ctx, pa.seq, pa.hep, B, tr.mx, tr.sm, tr.ts, arrive_rank, surv_fin, ctx->top_val,
                                                      ctx->top_ids, k, o.arrive.rank, o.arrive.lp, pa.status, pa.ex, s)))
        return rc;
    if (o.look.on) {
        // Lookahead choice: expand -> decode of the B * k_c children -> LSE and the target's score on their rows -> choose.
        // The inner decode and the two scoring passes run on the context's workspace in the middle of the step.  What they write
        // there: the decoder's activations (act_*) and plan tables (tok_row, seq_*, m_dev, tile_*, qrow_tile, n_wg_dev), all dead
        // once the outer decode has delivered ctx->xrows; ctx->lse_part, which no launch of this step reads again (the trace sweep
        // has reduced its own partials into the trace scratch); ctx->route_last, which then reports the inner decode.  What must
        // survive them and does, because they write none of it: ctx->xrows (anyway read for the last time by the survivor pass and
        // the trace sweep above), ctx->top_val / top_ids, the trace scratch, ctx->row_status, the carried thresholds (ctx->thr
        // and thr_valid / thr_M / thr_k: irs_launch_topk's alone) and ctx->step_ctr (ctx->step_pair is null here, so the inner
        // plan kernel does not hand the step counter over).  Everything the lookahead itself produces -- child windows, hep,
        // users, targets, the child rows, max / sumexp / target score, candidates, lp, choice -- lies in the caller's scratch.
        const int kc = o.look.kc, N = B * kc;
        irs_look_rows lk;
        irs_look_layout(o.look.scratch, o.look.users, kc, ctx->dims.max_len, ctx->dims.d, &lk);
        const irs_look_expand_args ea{pa.seq, pa.hep, user, B, ctx->dims.max_len, k, kc, ctx->top_val, ctx->top_ids, surv_fin,
                                      pa.step_ptr, pa.step_arg, pa.ex, lk.seq, lk.user, lk.tgt0, lk.ids0, lk.hep, lk.val};
        if ((rc = irs_launch_lookahead_expand(ctx, ea, s))) return rc;
        if ((rc = irs_launch_decode(ctx, lk.seq, user ? lk.user : nullptr, N, nullptr, lk.hep, lk.x, nullptr, s))) return rc;
        if ((rc = irs_launch_lse(ctx, lk.x, N, lk.mx, lk.sm, s))) return rc;
        if ((rc = irs_launch_gather(ctx, lk.x, N, lk.tgt0, 1, lk.ts, s))) return rc;
        const irs_look_choose_args ca{pa.seq, B, ctx->dims.max_len, k, kc, lk.ids0, lk.val, lk.mx, lk.sm, lk.ts, surv_fin, ctx->top_val,
                                      ctx->top_ids, lk.lp, lk.choice, o.look.rec_item, o.look.rec_lp, o.look.ld, row_map,
                                      ctx->step_ctr};
        if ((rc = irs_launch_lookahead_choose(ctx, ca, s))) return rc;
    }
    // bound sampler: a live row that the arrival rule has not chosen for draws among its first top_k admissible candidates; the
    // draw is keyed by the caller's row (row_map) and the device step counter
    if (o.sampler.on && (rc = irs_launch_sampler_choose(ctx, sampler_args(ctx, pa.seq, pa.hep, B, ctx->top_val, ctx->top_ids, k, surv_fin,
                                                                           pa.status, row_map, ctx->step_ctr, 0, pa.seed, pa.ex), s)))
        return rc;
    if ((rc = irs_launch_path_step(ctx, pa, B, ctx->top_val, ctx->top_ids, k, s))) return rc;
    if (o.trace.on) { // (the step index is still this step's: the merged loop publishes the next one in its second word)
        const irs_trace_rec rec{tr.mx, tr.sm, tr.ts, tr.rank, o.trace.item, o.trace.target, o.trace.rank, o.trace.ld};
        if ((rc = irs_launch_trace_record(ctx, rec, pa.seq, pa.hep, pa.paths, pa.path_ld, ctx->step_ctr, row_map, surv_fin, ctx->top_val,
                                          ctx->top_ids, k, B, s)))
            return rc;
    }
    return merged ? IRS_OK : irs_launch_inc(ctx, ctx->step_ctr, s);
}

// ------------------------------------------------------------------ exact candidates (survivors.hip)
extern "C" size_t irs_survivor_scratch_bytes(const irs_ctx *ctx, int32_t rows, int32_t want) {
    if (!ctx || rows < 1 || want < 1 || want > 32) return 0;
    return irs_surv_scratch(ctx, rows, want);
}

extern "C" int irs_topk_ensure_survivors(irs_ctx *ctx, const float *xrows, const int64_t *seq, const int32_t *hep, int32_t M,
                                         int32_t rows_per_status, int32_t k, int32_t want, const double *cum, const int32_t *fin,
                                         const int32_t *done, float *val, int64_t *ids0, int32_t *status, void *scratch,
                                         size_t scratch_bytes, void *stream) {
    if (!ctx) return IRS_E_INVALID;
    if (!xrows || !seq || !hep || !val || !ids0 || !status || !scratch) IRS_FAIL(ctx, IRS_E_INVALID, "irs_topk_ensure_survivors: null pointer");
    if (M < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_topk_ensure_survivors: M must be >= 1");
    if (k < 1 || k > ctx->dims.max_k) IRS_FAIL(ctx, IRS_E_INVALID, "irs_topk_ensure_survivors: k must be in [1, %d]", ctx->dims.max_k);
    if (want < 1 || want > k || want > 32) IRS_FAIL(ctx, IRS_E_INVALID, "irs_topk_ensure_survivors: want must be in [1, min(k, 32)]");
    if (rows_per_status < 1 || M % rows_per_status)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_topk_ensure_survivors: rows_per_status must be >= 1 and divide M");
    int rc = check_scratch(ctx, "irs_topk_ensure_survivors", scratch, scratch_bytes, irs_surv_scratch(ctx, M, want));
    if (rc) return rc;
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_topk_ensure_survivors needs the whole catalog on one device");
    if ((rc = check_excl(ctx, "irs_topk_ensure_survivors", M / rows_per_status, 0))) return rc;
    if ((rc = ready(ctx))) return rc;
    const irs_surv_args sa{xrows, seq, hep, M, rows_per_status, k, want, M, cum, fin, done, val, ids0, status, nullptr,
                           excl_args(ctx, rows_per_status, nullptr, nullptr, 0, 0, nullptr, 0)}; // (no path argument: the list only)
    return irs_launch_survivors(ctx, sa, scratch, (hipStream_t)stream);
}

extern "C" int irs_bind_survivor_scratch(irs_ctx *ctx, void *scratch, size_t bytes) {
    if (!ctx) return IRS_E_INVALID;
    if ((scratch == nullptr) != (bytes == 0)) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_survivor_scratch: a scratch and its size go together");
    if (((uintptr_t)scratch) & 15) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_survivor_scratch: scratch must be 16-byte aligned");
    ctx->opt.surv = {scratch, bytes};
    opts_changed(ctx);
    return IRS_OK;
}

// ------------------------------------------------------------------ recommend: the top-n admissible items of every row (recommend.hip)
// Both entry points take no stream: their launches are enqueued on the null stream and the call returns without waiting (irs_hip.h)
// The caller's scratch, in this order: the rows' ranked lists (ids, then values), their (max, sum exp), the empty windows of a call
// without dev_seq, then the survivor pass's own layout for want = n
struct recommend_rows {
    int64_t *ids0; // [M][k]
    float *val;    // [M][k]
    float *mx, *sm; // [M]
    int32_t *no_hep; // [M] all -1: the empty windows the repair reads when the caller gives none ...
    const int64_t *no_seq; // ... and the window rows that go with them: behind hep = -1 no slot of a row is ever read, so this
                           // points at no_hep's own bytes and is NOT [M][L] -- it only keeps the pass's pointer non-null
    void *surv;
};
static size_t recommend_layout(const irs_ctx *ctx, void *base, int M, int n, int k, recommend_rows *o) {
    const size_t n_val = align_up((size_t)M * k * sizeof(float), 16), n_ids = align_up((size_t)M * k * sizeof(int64_t), 16);
    const size_t r4 = align_up((size_t)M * sizeof(float), 16);
    if (o) {
        char *p = (char *)base;
        o->ids0 = (int64_t *)p, o->val = (float *)(p + n_ids);
        o->mx = (float *)(p + n_ids + n_val), o->sm = (float *)(p + n_ids + n_val + r4);
        o->no_hep = (int32_t *)(p + n_ids + n_val + 2 * r4), o->no_seq = (const int64_t *)o->no_hep;
        o->surv = p + n_ids + n_val + 3 * r4;
    }
    return n_ids + n_val + 3 * r4 + irs_surv_scratch(ctx, M, n);
}
static bool recommend_shape_ok(const irs_ctx *ctx, int M, int n, int k) {
    return M >= 1 && M <= ctx->max_rows && k >= 1 && k <= ctx->dims.max_k && n >= 1 && n <= k && n <= IRS_MAX_RECOMMEND;
}
static int check_recommend(irs_ctx *ctx, const char *fn, bool ptrs_ok, int M, int n, int k) {
    if (!ptrs_ok) IRS_FAIL(ctx, IRS_E_INVALID, "%s: null pointer", fn);
    if (M < 1) IRS_FAIL(ctx, IRS_E_INVALID, "%s: M must be >= 1", fn);
    if (M > ctx->max_rows) IRS_FAIL(ctx, IRS_E_INVALID, "%s: M=%d exceeds max_rows=%d", fn, M, ctx->max_rows);
    if (k < 1 || k > ctx->dims.max_k) IRS_FAIL(ctx, IRS_E_INVALID, "%s: k must be in [1, %d]", fn, ctx->dims.max_k);
    if (n < 1 || n > k || n > IRS_MAX_RECOMMEND) IRS_FAIL(ctx, IRS_E_INVALID, "%s: n must be in [1, min(k, %d)]", fn, IRS_MAX_RECOMMEND);
    return IRS_OK;
}
// the exclusion lists as the take and the repair read them: never a path, and a binding without a list (no_repeat alone) is none:
// nothing of it is read, so nothing of it is checked either (its user count included)
static irs_excl recommend_excl(const irs_ctx *ctx) {
    const irs_excl e = excl_args(ctx, 1, nullptr, nullptr, 0, 0, nullptr, 0);
    return e.rows ? e : irs_excl{};
}

extern "C" size_t irs_recommend_scratch_bytes(const irs_ctx *ctx, int32_t rows, int32_t n, int32_t k) {
    if (!ctx || !recommend_shape_ok(ctx, rows, n, k)) return 0;
    return recommend_layout(ctx, nullptr, rows, n, k, nullptr);
}

extern "C" int irs_recommend_take(irs_ctx *ctx, const int64_t *seq, const int32_t *hep, int32_t M, const float *val, const int64_t *ids0,
                                  int32_t k, const float *lse_max, const float *lse_sum, int32_t n, float *out_val, int64_t *out_ids0,
                                  float *out_lp, int32_t *out_count) {
    if (!ctx) return IRS_E_INVALID;
    const char *fn = "irs_recommend_take";
    int rc = check_recommend(ctx, fn, val && ids0 && out_val && out_ids0 && out_count && (seq == nullptr) == (hep == nullptr), M, n, k);
    if (rc) return rc;
    if (out_lp && (!lse_max || !lse_sum)) IRS_FAIL(ctx, IRS_E_INVALID, "%s: out_lp needs dev_lse_max and dev_lse_sum", fn);
    const irs_excl ex = recommend_excl(ctx);
    if (ex.on && (rc = search_rules(ctx, fn, AT_RECOMMEND, search_call{M, 0, 0, k, 0, 0, 0, true}))) return rc;
    return irs_launch_recommend_take(ctx, seq, hep, M, val, ids0, k, lse_max, lse_sum, n, out_val, out_ids0, out_lp, out_count, ex, nullptr);
}

extern "C" int irs_recommend(irs_ctx *ctx, const float *xrows, const int64_t *seq, const int32_t *hep, int32_t M, int32_t n, int32_t k,
                             int32_t sweep, float *out_val, int64_t *out_ids0, float *out_lp, int32_t *out_count, int32_t *status,
                             void *scratch, size_t scratch_bytes) {
    if (!ctx) return IRS_E_INVALID;
    const char *fn = "irs_recommend";
    int rc = check_recommend(ctx, fn, xrows && out_val && out_ids0 && out_count && status && (seq == nullptr) == (hep == nullptr), M, n, k);
    if (rc) return rc;
    if (sweep != IRS_SWEEP_BF16 && sweep != IRS_SWEEP_F32) IRS_FAIL(ctx, IRS_E_INVALID, "%s: bad sweep", fn);
    if ((rc = check_scratch(ctx, fn, scratch, scratch_bytes, recommend_layout(ctx, nullptr, M, n, k, nullptr)))) return rc;
    const irs_excl ex = recommend_excl(ctx);
    if (ex.on && (rc = search_rules(ctx, fn, AT_RECOMMEND, search_call{M, 0, 0, k, sweep, 0, 0, true}))) return rc;
    if (ctx->opt.offer.on && (rc = args_offer(ctx, fn, search_call{M, 0, 0, k, sweep, 0, 0, true}))) return rc;
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "%s needs the whole catalog on one device", fn);
    if ((rc = irs_ready_filter(ctx, sweep))) return rc;
    hipStream_t s = nullptr; // (the null stream: irs_hip.h)
    recommend_rows r;
    recommend_layout(ctx, scratch, M, n, k, &r);
    if ((rc = launch_lists(ctx, xrows, M, k, sweep, r.val, r.ids0, status, s, out_lp ? r.mx : nullptr, out_lp ? r.sm : nullptr, 0))) return rc;
    if (seq || ex.on) { // (with neither a window nor a list every entry is admissible: no row can be short)
        if (!seq) IRS_CHECK_HIP(ctx, hipMemsetAsync(r.no_hep, 0xFF, (size_t)M * sizeof(int32_t), s)); // every byte 0xFF: hep = -1
        const irs_surv_args sa{xrows, seq ? seq : r.no_seq, seq ? hep : r.no_hep, M, 1, k, n, M, nullptr, nullptr, nullptr, r.val, r.ids0, status,
                               nullptr, ex};
        if ((rc = irs_launch_survivors(ctx, sa, r.surv, s))) return rc;
    }
    return irs_launch_recommend_take(ctx, seq, hep, M, r.val, r.ids0, k, r.mx, r.sm, n, out_val, out_ids0, out_lp, out_count, ex, s);
}

// ------------------------------------------------------------------ path trace (irs_bind_path_trace)
extern "C" size_t irs_path_trace_scratch_bytes(const irs_ctx *ctx, int32_t rows) {
    if (!ctx || rows < 1 || rows > ctx->max_rows) return 0;
    return irs_trace_layout(nullptr, rows, nullptr);
}

extern "C" int irs_score_target_trace(irs_ctx *ctx, const float *xrows, const int64_t *seq, const int32_t *hep, int32_t M,
                                      void *scratch, size_t scratch_bytes, float *omax, float *osum, float *tscore, int32_t *rank,
                                      void *stream) {
    int rc = ready(ctx);
    if (rc) return rc;
    if ((rc = check_rows(ctx, "irs_score_target_trace", xrows, M))) return rc;
    if (!seq || !hep || !scratch || !omax || !osum || !tscore || !rank) IRS_FAIL(ctx, IRS_E_INVALID, "irs_score_target_trace: null pointer");
    if ((rc = check_scratch(ctx, "irs_score_target_trace", scratch, scratch_bytes, irs_trace_layout(nullptr, M, nullptr)))) return rc;
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_score_target_trace needs the whole catalog on one device");
    irs_trace_rows tr;
    irs_trace_layout(scratch, M, &tr);
    return irs_launch_target_trace(ctx, xrows, seq, hep, M, tr, omax, osum, tscore, rank, (hipStream_t)stream);
}

extern "C" int irs_bind_path_trace(irs_ctx *ctx, float *lp_item, float *lp_target, int32_t *rank_target, int32_t users, int32_t ld,
                                   void *scratch, size_t bytes) {
    if (!ctx) return IRS_E_INVALID;
    if (!lp_item && !lp_target && !rank_target) { // unbind
        if (ctx->opt.trace.on) opts_changed(ctx);
        ctx->opt.trace = {};
        ctx->opt.adm = {}; // (an admissible rank is bound to this trace: irs_bind_trace_admissible)
        return IRS_OK;
    }
    if (!lp_item || !lp_target || !rank_target) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_path_trace: the three arrays go together");
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_path_trace needs the whole catalog on one device");
    if (users < 1 || users > ctx->max_rows || ld < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_path_trace: users in [1, max_rows=%d], ld >= 1", ctx->max_rows);
    const int rc = check_scratch(ctx, "irs_bind_path_trace", scratch, bytes, irs_trace_layout(nullptr, users, nullptr));
    if (rc) return rc;
    ctx->opt.trace = {1, lp_item, lp_target, rank_target, users, ld, scratch};
    ctx->opt.adm = {}; // (a new trace: the admissible rank of the previous one is dropped with it)
    opts_changed(ctx);
    return IRS_OK;
}

// ------------------------------------------------------------------ admissible rank (admissible.hip)
extern "C" size_t irs_admissible_scratch_bytes(const irs_ctx *ctx, int32_t rows) {
    if (!ctx || rows < 1 || rows > ctx->max_rows) return 0;
    return irs_adm_layout(rows);
}

extern "C" int irs_bind_trace_admissible(irs_ctx *ctx, int32_t *rank_adm, int32_t users, int32_t ld, void *scratch, size_t bytes) {
    if (!ctx) return IRS_E_INVALID;
    if (!rank_adm) { // unbind
        if (ctx->opt.adm.on) opts_changed(ctx);
        ctx->opt.adm = {};
        return IRS_OK;
    }
    const auto &t = ctx->opt.trace;
    if (!t.on) IRS_FAIL(ctx, IRS_E_STATE, "irs_bind_trace_admissible: no path trace is bound (irs_bind_path_trace)");
    if (users != t.users || ld != t.ld)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_trace_admissible: [%d, %d], the path trace is bound for [%d, %d]", users, ld, t.users, t.ld);
    const int rc = check_scratch(ctx, "irs_bind_trace_admissible", scratch, bytes, irs_adm_layout(users));
    if (rc) return rc;
    ctx->opt.adm = {1, rank_adm, scratch};
    opts_changed(ctx);
    return IRS_OK;
}

extern "C" int irs_score_target_rank_admissible(irs_ctx *ctx, const float *xrows, const int64_t *seq, const int32_t *hep, int32_t M,
                                                const float *paths, int32_t path_ld, int32_t step, void *trace_scratch,
                                                size_t trace_bytes, void *scratch, size_t bytes, float *omax, float *osum, float *tscore,
                                                int32_t *rank, int32_t *rank_adm) {
    if (!ctx) return IRS_E_INVALID;
    const char *fn = "irs_score_target_rank_admissible";
    int rc = check_rows(ctx, fn, xrows, M);
    if (rc) return rc;
    if (!seq || !hep || !omax || !osum || !tscore || !rank || !rank_adm) IRS_FAIL(ctx, IRS_E_INVALID, "%s: null pointer", fn);
    if ((rc = check_scratch(ctx, fn, trace_scratch, trace_bytes, irs_trace_layout(nullptr, M, nullptr)))) return rc;
    if ((rc = check_scratch(ctx, fn, scratch, bytes, irs_adm_layout(M)))) return rc;
    if (step < 0 || (paths && (path_ld < 1 || step > path_ld))) IRS_FAIL(ctx, IRS_E_INVALID, "%s: step must be in [0, path_ld], path_ld >= 1", fn);
    if (paths && step > IRS_MAX_PATH) IRS_FAIL(ctx, IRS_E_INVALID, "%s: step %d > %d path entries", fn, step, IRS_MAX_PATH);
    const auto &o = ctx->opt;
    if (o.excl.on && o.excl.rows && M > o.excl.users) IRS_FAIL(ctx, IRS_E_INVALID, "%s: %d rows, exclusions are bound for %d users", fn, M, o.excl.users);
    if (o.offer.on && M > o.offer.rows)
        IRS_FAIL(ctx, IRS_E_INVALID, "%s: %d rows, the offer set's scratch (irs_bind_offer_set) is sized for %d", fn, M, o.offer.rows);
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "%s needs the whole catalog on one device", fn);
    if ((rc = ready(ctx))) return rc;
    hipStream_t s = nullptr; // (the null stream, as irs_recommend and irs_score_topk_offer: irs_hip.h)
    irs_trace_rows tr;
    irs_trace_layout(trace_scratch, M, &tr);
    if ((rc = irs_launch_target_trace(ctx, xrows, seq, hep, M, tr, omax, osum, tscore, rank, s))) return rc;
    // H: the bound list of user r for row r (a binding of no_repeat alone holds no list), and the caller's path rows whether or
    // not no_repeat is bound -- the call states what the step at `step` would hide
    irs_adm_args a = {xrows, seq, hep, M, tscore, tr.refid, tr.count};
    if (o.excl.on && o.excl.rows) a.ex.rows = o.excl.rows, a.ex.cnt = o.excl.cnt, a.ex.stride = o.excl.stride;
    if (paths && step > 0) a.ex.paths = paths, a.ex.path_ld = path_ld, a.ex.step_arg = step;
    a.ex.div = 1, a.ex.on = (a.ex.rows || a.ex.paths) ? 1 : 0;
    if (o.offer.on) { // the set's scores of these rows: the score pass of irs_score_topk_offer
        irs_offer_rows of;
        irs_offer_layout(o.offer.scratch, o.offer.n, o.offer.rows, &of);
        if ((rc = irs_launch_offer_scores(ctx, xrows, M, of, s))) return rc;
        a.oids = of.ids, a.on = o.offer.n, a.oc_pad = of.c_pad, a.osc = of.sc, a.oholes = of.holes;
    }
    a.out = rank_adm;
    return irs_launch_trace_rank_adm(ctx, a, s);
}

// ------------------------------------------------------------------ beam trace (irs_bind_beam_trace; beam_trace.hip)
static bool beam_trace_shape_ok(const irs_ctx *ctx, int users, int W) {
    return users >= 1 && W >= 1 && W <= 32 && (int64_t)users * W <= ctx->max_seqs && (int64_t)users * W <= ctx->max_rows;
}

extern "C" size_t irs_beam_trace_scratch_bytes(const irs_ctx *ctx, int32_t users, int32_t W) {
    if (!ctx || !beam_trace_shape_ok(ctx, users, W)) return 0;
    return irs_beam_trace_layout(nullptr, users * W, nullptr, nullptr);
}

extern "C" int irs_bind_beam_trace(irs_ctx *ctx, float *lp_item, float *lp_target, int32_t *rank_target, int32_t users, int32_t W,
                                   int32_t ld, void *scratch, size_t bytes) {
    if (!ctx) return IRS_E_INVALID;
    if (!lp_item && !lp_target && !rank_target) { // unbind
        if (ctx->opt.btrace.on) opts_changed(ctx);
        ctx->opt.btrace = {};
        return IRS_OK;
    }
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_bind_beam_trace needs the whole catalog on one device");
    if (!lp_item || !lp_target || !rank_target) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_beam_trace: the three arrays go together");
    if (W < 1 || W > 32) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_beam_trace: beam width must be in [1, 32]");
    if (!beam_trace_shape_ok(ctx, users, W))
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_beam_trace: users >= 1 and users*W within max_seqs=%d / max_rows=%d", ctx->max_seqs, ctx->max_rows);
    if (ld < 1 || ld > IRS_MAX_PATH) IRS_FAIL(ctx, IRS_E_INVALID, "irs_bind_beam_trace: ld must be in [1, %d]", IRS_MAX_PATH);
    const int rc = check_scratch(ctx, "irs_bind_beam_trace", scratch, bytes, irs_beam_trace_layout(nullptr, users * W, nullptr, nullptr));
    if (rc) return rc;
    ctx->opt.btrace = {1, lp_item, lp_target, rank_target, users, W, ld, scratch};
    opts_changed(ctx);
    return IRS_OK;
}

extern "C" int irs_beam_trace_carry(irs_ctx *ctx, const int32_t *link, const float *link_val, const float *mx, const float *sm,
                                    const float *tscore, const int32_t *rank, int32_t B, int32_t W, int32_t step, float *lp_item,
                                    float *lp_target, int32_t *rank_target, int32_t ld, const int32_t *row_map) {
    if (!ctx) return IRS_E_INVALID;
    if (!link || !link_val || !mx || !sm || !tscore || !rank || !lp_item || !lp_target || !rank_target)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_trace_carry: null pointer");
    if (B < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_trace_carry: B must be >= 1");
    if (W < 1 || W > 32) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_trace_carry: beam width must be in [1, 32]");
    if (ld < 1 || ld > IRS_MAX_PATH) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_trace_carry: ld must be in [1, %d]", IRS_MAX_PATH);
    if (step < 0 || step >= ld) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_trace_carry: step must be in [0, ld)");
    const irs_beam_carry_args a{{(int32_t *)link, (float *)link_val}, mx, sm, tscore, rank, W, ld, step, nullptr, lp_item, lp_target,
                                rank_target, row_map};
    return look_run_sync(ctx, irs_launch_beam_trace_carry(ctx, a, B, nullptr)); // (synchronous, on the null stream: irs_hip.h)
}

// ------------------------------------------------------------------ arrival rule (irs_set_arrival_rule; path.hip: k_arrival_offer)
static int set_arrival_rule(irs_ctx *ctx, const char *fn, int rank_max, float lp_min, int kind) {
    if (!ctx) return IRS_E_INVALID;
    if (rank_max < 0) IRS_FAIL(ctx, IRS_E_INVALID, "%s: rank_max must be >= 0 (0: the rank clause is off)", fn);
    if (kind != IRS_RANK_WINDOW && kind != IRS_RANK_ADMISSIBLE)
        IRS_FAIL(ctx, IRS_E_INVALID, "%s: rank_kind %d (IRS_RANK_WINDOW or IRS_RANK_ADMISSIBLE)", fn, kind);
    const int lp_on = irs_arrival_lp_on(lp_min) ? 1 : 0;
    const int on = (rank_max >= 1 || lp_on) ? 1 : 0;
    if (on && ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "%s needs the whole catalog on one device", fn);
    const float lp = lp_on ? lp_min : (on ? __builtin_nanf("") : 0.f); // (what the kernel takes: NaN is "clause off")
    if (!on) kind = IRS_RANK_WINDOW;
    auto &a = ctx->opt.arrive;
    if (on != a.on || rank_max != a.rank || lp_on != a.lp_on || memcmp(&lp, &a.lp, sizeof(lp)) || kind != a.kind) opts_changed(ctx);
    a = {on, on ? rank_max : 0, lp_on, lp, kind};
    return IRS_OK;
}

extern "C" int irs_set_arrival_rule(irs_ctx *ctx, int32_t rank_max, float lp_min) {
    return set_arrival_rule(ctx, "irs_set_arrival_rule", rank_max, lp_min, IRS_RANK_WINDOW);
}

extern "C" int irs_set_arrival_rule_ex(irs_ctx *ctx, int32_t rank_max, float lp_min, int32_t rank_kind) {
    return set_arrival_rule(ctx, "irs_set_arrival_rule_ex", rank_max, lp_min, rank_kind);
}

extern "C" int irs_arrival_offer(irs_ctx *ctx, const int64_t *seq, const int32_t *hep, int32_t M, const float *mx, const float *sm,
                                 const float *tscore, const int32_t *rank, const int32_t *fin, float *val, int64_t *ids0, int32_t k,
                                 int32_t rank_max, float lp_min, const float *paths, int32_t path_ld, int32_t step,
                                 const int32_t *row_map, int32_t *status, void *stream) {
    if (!ctx) return IRS_E_INVALID;
    if (!seq || !hep || !mx || !sm || !tscore || !rank || !val || !ids0 || !status) IRS_FAIL(ctx, IRS_E_INVALID, "irs_arrival_offer: null pointer");
    if (M < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_arrival_offer: M must be >= 1");
    if (k < 1 || k > ctx->dims.max_k) IRS_FAIL(ctx, IRS_E_INVALID, "irs_arrival_offer: k must be in [1, %d]", ctx->dims.max_k);
    if (rank_max < 0) IRS_FAIL(ctx, IRS_E_INVALID, "irs_arrival_offer: rank_max must be >= 0 (0: the rank clause is off)");
    if (rank_max == 0 && !irs_arrival_lp_on(lp_min)) IRS_FAIL(ctx, IRS_E_INVALID, "irs_arrival_offer: both clauses are off");
    if (step < 0 || (paths && (path_ld < 1 || step > path_ld)))
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_arrival_offer: step must be in [0, path_ld], path_ld >= 1");
    if (ctx->opt.excl.on && ctx->opt.excl.no_repeat && !paths) IRS_FAIL(ctx, IRS_E_INVALID, "irs_arrival_offer: no_repeat is bound: dev_paths is null");
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_arrival_offer needs the whole catalog on one device");
    const int rc = check_excl(ctx, "irs_arrival_offer", M, step);
    if (rc) return rc;
    return irs_launch_arrival_offer(ctx, seq, hep, M, mx, sm, tscore, rank, fin, val, ids0, k, rank_max, lp_min, status,
                                    excl_args(ctx, 1, row_map, paths, path_ld, 1, nullptr, step), (hipStream_t)stream);
}

// ------------------------------------------------------------------ beam rule (irs_set_beam_rule; path.hip: k_beam_step's ruled form)
static bool beam_weight_ok(float w) { return w >= 0.f && w <= 3.402823466e38f; } // finite and >= 0 (a NaN fails both)

extern "C" int irs_set_beam_rule(irs_ctx *ctx, int32_t rank_max, float lp_min, float target_weight) {
    if (!ctx) return IRS_E_INVALID;
    if (rank_max < 0) IRS_FAIL(ctx, IRS_E_INVALID, "irs_set_beam_rule: rank_max must be >= 0 (0: the rank clause is off)");
    if (!beam_weight_ok(target_weight)) IRS_FAIL(ctx, IRS_E_INVALID, "irs_set_beam_rule: target_weight must be finite and >= 0 (0: ranking is off)");
    const int lp_on = irs_arrival_lp_on(lp_min) ? 1 : 0;
    const int on = (rank_max >= 1 || lp_on || target_weight > 0.f) ? 1 : 0;
    if (on && ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_set_beam_rule needs the whole catalog on one device");
    const float lp = lp_on ? lp_min : (on ? __builtin_nanf("") : 0.f); // (what the kernel takes: NaN is "clause off")
    auto &r = ctx->opt.brule;
    if (on != r.on || rank_max != r.rank || lp_on != r.lp_on || memcmp(&lp, &r.lp, sizeof(lp)) || target_weight != r.weight) opts_changed(ctx);
    r = {on, on ? rank_max : 0, lp_on, lp, on ? target_weight : 0.f};
    return IRS_OK;
}

// ------------------------------------------------------------------ path replay (replay.hip)
static int replay_chunk_max(const irs_ctx *ctx) { return ctx->max_rows < ctx->max_seqs ? ctx->max_rows : ctx->max_seqs; }

extern "C" size_t irs_replay_scratch_bytes(const irs_ctx *ctx, int32_t chunk) {
    if (!ctx || chunk < 1 || chunk > replay_chunk_max(ctx)) return 0;
    return irs_replay_layout(nullptr, chunk, ctx->dims.max_len, ctx->dims.d, nullptr);
}

// what the builder and the replay share: the shapes, the layout and the pointers that go with it
static int check_replay(irs_ctx *ctx, const char *fn, int layout, const void *seq0, const void *hep0, int B, const void *paths, int P,
                        int path_ld, const void *row_user, const void *row_step, int R) {
    if (layout != IRS_REPLAY_SLOT && layout != IRS_REPLAY_FULL) IRS_FAIL(ctx, IRS_E_INVALID, "%s: unknown layout %d", fn, layout);
    if (!seq0 || !paths || !row_user || !row_step) IRS_FAIL(ctx, IRS_E_INVALID, "%s: null pointer", fn);
    if (layout == IRS_REPLAY_SLOT && !hep0) IRS_FAIL(ctx, IRS_E_INVALID, "%s: IRS_REPLAY_SLOT needs dev_hep0", fn);
    if (R < 1 || R > IRS_REPLAY_MAX_ROWS) IRS_FAIL(ctx, IRS_E_INVALID, "%s: R must be in [1, %d]", fn, IRS_REPLAY_MAX_ROWS);
    if (B < 1 || P < 0 || path_ld < P) IRS_FAIL(ctx, IRS_E_INVALID, "%s: B >= 1, P >= 0 and path_ld >= P", fn);
    return IRS_OK;
}

extern "C" int irs_replay_windows(irs_ctx *ctx, int32_t layout, const int64_t *seq0, const int32_t *hep0, const int64_t *user, int32_t B,
                                  const int64_t *paths, int32_t P, int32_t path_ld, const int32_t *row_user, const int32_t *row_step,
                                  int32_t R, int64_t *seq_out, int32_t *hep_out, int64_t *user_out, int32_t *status, void *stream) {
    if (!ctx) return IRS_E_INVALID;
    const int rc = check_replay(ctx, "irs_replay_windows", layout, seq0, hep0, B, paths, P, path_ld, row_user, row_step, R);
    if (rc) return rc;
    if (!seq_out || !hep_out || !status) IRS_FAIL(ctx, IRS_E_INVALID, "irs_replay_windows: null output");
    const irs_replay_args a{layout, B, ctx->dims.max_len, P, path_ld, R, ctx->dims.n_item, seq0, hep0, user, nullptr, paths,
                            row_user, row_step, seq_out, hep_out, user_out, status, nullptr, nullptr};
    return irs_launch_replay_windows(ctx, a, (hipStream_t)stream);
}

extern "C" int irs_replay_paths(irs_ctx *ctx, int32_t layout, const int64_t *seq0, const int32_t *hep0, const int64_t *user,
                                const int64_t *target, int32_t B, const int64_t *paths, int32_t P, int32_t path_ld,
                                const int32_t *row_user, const int32_t *row_step, int32_t R, int32_t chunk, void *scratch,
                                size_t scratch_bytes, float *lp_item, float *lp_target, int32_t *rank, int32_t *status, void *stream) {
    if (!ctx) return IRS_E_INVALID;
    int rc = check_replay(ctx, "irs_replay_paths", layout, seq0, hep0, B, paths, P, path_ld, row_user, row_step, R);
    if (rc) return rc;
    if (!lp_item || !lp_target || !rank || !status || !scratch) IRS_FAIL(ctx, IRS_E_INVALID, "irs_replay_paths: null pointer");
    if (layout == IRS_REPLAY_FULL && !target) IRS_FAIL(ctx, IRS_E_INVALID, "irs_replay_paths: IRS_REPLAY_FULL needs dev_target");
    if (layout == IRS_REPLAY_SLOT && target)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_replay_paths: IRS_REPLAY_SLOT takes the target from slot L-1: dev_target must be NULL");
    if (ctx->dims.mask_mode == IRS_MASK_IRN && !user) IRS_FAIL(ctx, IRS_E_INVALID, "irs_replay_paths: user is null");
    if (chunk < 1 || chunk > replay_chunk_max(ctx))
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_replay_paths: chunk must be in [1, min(max_rows, max_seqs) = %d]", replay_chunk_max(ctx));
    const size_t need = irs_replay_layout(nullptr, chunk, ctx->dims.max_len, ctx->dims.d, nullptr);
    if ((rc = check_scratch(ctx, "irs_replay_paths", scratch, scratch_bytes, need))) return rc;
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_replay_paths needs the whole catalog on one device");
    if (layout == IRS_REPLAY_FULL && ctx->dims.mask_mode == IRS_MASK_IRN)
        IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_replay_paths: IRS_REPLAY_FULL on an IRS_MASK_IRN context (its mask gives column L-1 a meaning)");
    if ((rc = ready(ctx))) return rc;
    hipStream_t s = (hipStream_t)stream;
    irs_replay_rows sc;
    irs_replay_layout(scratch, chunk, ctx->dims.max_len, ctx->dims.d, &sc);
    const int64_t *dec_user = ctx->dims.mask_mode == IRS_MASK_IRN ? sc.user : nullptr;
    for (int r0 = 0; r0 < R; r0 += chunk) { // a pass: windows -> decode at hep, rows only -> target and item -> sweep -> record
        const int m = R - r0 < chunk ? R - r0 : chunk;
        const irs_replay_args a{layout, B, ctx->dims.max_len, P, path_ld, m, ctx->dims.n_item, seq0, hep0, user, target, paths,
                                row_user + r0, row_step + r0, sc.seq, sc.hep, sc.user, status + r0, sc.item, sc.target};
        if ((rc = irs_launch_replay_windows(ctx, a, s))) return rc;
        if ((rc = irs_launch_decode(ctx, sc.seq, dec_user, m, nullptr, sc.hep, sc.x, nullptr, s))) return rc;
        if ((rc = irs_launch_replay_score(ctx, sc, m, status + r0, lp_item + r0, lp_target + r0, rank + r0, s))) return rc;
    }
    return IRS_OK;
}

// ------------------------------------------------------------------ what the search loops share
int irs_replay_steps(irs_ctx *ctx, irs_step_graph *g, const irs_step_key &key, const std::function<int(hipStream_t)> &body,
                     int times, hipStream_t s, int *capture_failed) {
    if (capture_failed) *capture_failed = 0;
    if (!g->exec || memcmp(&g->key, &key, sizeof(key))) {
        if (g->exec) (void)hipGraphExecDestroy(g->exec);
        g->exec = nullptr;
        hipStream_t cs = nullptr;
        hipGraph_t graph = nullptr;
        int rc = IRS_OK;
        hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
        if (e == hipSuccess && (e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal)) == hipSuccess) {
            rc = body(cs);
            const hipError_t e2 = hipStreamEndCapture(cs, &graph); // (a failed body's capture is ended too)
            if (rc == IRS_OK) e = e2;
        }
        if (rc == IRS_OK && e == hipSuccess) e = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
        if (graph) (void)hipGraphDestroy(graph);
        if (cs) (void)hipStreamDestroy(cs);
        if (rc != IRS_OK || e != hipSuccess) {
            g->exec = nullptr;
            if (capture_failed) *capture_failed = rc != IRS_OK ? IRS_CAPTURE_BODY : IRS_CAPTURE_HIP;
            if (rc != IRS_OK) return rc;
            IRS_FAIL(ctx, IRS_E_HIP, "graph capture failed: %s", hipGetErrorString(e));
        }
        g->key = key;
    }
    for (int i = 0; i < times; ++i) IRS_CHECK_HIP(ctx, hipGraphLaunch(g->exec, s));
    return IRS_OK;
}

// (the sharded entry points have checked `sweep` before they come here)
int irs_check_k(irs_ctx *ctx, const char *fn, int k, int world, int sweep, int sample, int sample_k) {
    if (k < 1 || k > ctx->dims.max_k || (int64_t)k * world > 2048) IRS_FAIL(ctx, IRS_E_INVALID, "%s: bad k", fn);
    if (sweep != IRS_SWEEP_BF16 && sweep != IRS_SWEEP_F32) IRS_FAIL(ctx, IRS_E_INVALID, "%s: bad sweep", fn);
    if (sample && (sample_k < 1 || sample_k > IRS_MAX_SAMPLE_K))
        IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "%s: sample_k must be in [1, %d]", fn, IRS_MAX_SAMPLE_K);
    return IRS_OK;
}

int irs_check_beam_args(irs_ctx *ctx, const char *fn, bool ptrs_ok, int B, int W, int P) {
    if (!ptrs_ok || B < 1) IRS_FAIL(ctx, IRS_E_INVALID, "%s: bad arguments", fn);
    if (W < 1 || W > 32) IRS_FAIL(ctx, IRS_E_INVALID, "%s: beam width must be in [1, 32]", fn);
    if (P < 1 || P > IRS_MAX_PATH) IRS_FAIL(ctx, IRS_E_INVALID, "%s: path length must be in [1, %d]", fn, IRS_MAX_PATH);
    return IRS_OK;
}

// the common opening of the four single-device search loops.  W == 0: a greedy loop over B rows; else a beam search over B * W
// rows.  ptrs_ok: none of the call's required pointers is null.  (A null context has no options: an arrival rule without a trace,
// the greedy loops' first refusal, is looked at behind it.)
static int check_search(irs_ctx *ctx, const char *fn, bool ptrs_ok, int B, int W, int P, int k, int sweep, int sample, int sample_k) {
    if (!ctx) return IRS_E_INVALID;
    return search_rules(ctx, fn, W ? AT_BEAM_LOOP : AT_GREEDY_LOOP, search_call{B, W, P, k, sweep, sample, sample_k, ptrs_ok});
}

// the path step's arguments inside a search loop: the step index comes from the device counter
// (`out_paths`: the caller's path rows, which a bound no_repeat reads back: row b in irs_generate_paths, the compaction map's in
//  the until loop, whose steps write `paths` = the stage)
static irs_path_args loop_path_args(irs_ctx *ctx, int64_t *seq, int32_t *hep, float *paths, int P, int sample, int sample_k,
                                    uint64_t seed, int32_t *status, const float *out_paths) {
    return irs_path_args{seq, hep, ctx->dims.max_len, paths, P, sample, sample_k, seed, status, ctx->step_ctr, 0, nullptr, 1,
                         excl_args(ctx, 1, nullptr, out_paths, P, 1, ctx->step_ctr, 0)};
}

// The check of the two until loops: places of the live rows in un_dst (irs_launch_until_scan over `fin`), their number in *left
// after a 4-byte copy and a synchronise.  `what`: what the caller's message calls a row
static int live_count(irs_ctx *ctx, const char *fn, const char *what, const int32_t *fin, int live, int *left, hipStream_t s) {
    int rc = irs_launch_until_scan(ctx, fin, live, ctx->un_dst, ctx->un_count, s);
    if (rc) return rc;
    IRS_CHECK_HIP(ctx, hipMemcpyAsync(&ctx->un_count_host, ctx->un_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    IRS_CHECK_HIP(ctx, hipStreamSynchronize(s));
    *left = ctx->un_count_host;
    if (*left < 0 || *left > live) IRS_FAIL(ctx, IRS_E_STATE, "%s: live count %d of %d %s", fn, *left, live, what);
    return IRS_OK;
}

int irs_search_begin(irs_ctx *ctx, int32_t *status, int B, hipStream_t s) {
    IRS_CHECK_HIP(ctx, hipMemsetAsync(ctx->step_ctr, 0, 2 * sizeof(int32_t), s));
    IRS_CHECK_HIP(ctx, hipMemsetAsync(status, 0, sizeof(int32_t) * B, s));
    return IRS_OK;
}

int irs_beam_finish(irs_ctx *ctx, size_t rows, int P, float *paths, double *scores, int64_t *seq_final, hipStream_t s) {
    const int fin = P & 1;
    IRS_CHECK_HIP(ctx, hipMemcpyAsync(paths, ctx->bm[fin].paths, rows * P * sizeof(float), hipMemcpyDeviceToDevice, s));
    IRS_CHECK_HIP(ctx, hipMemcpyAsync(scores, ctx->bm[fin].cum, rows * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (seq_final)
        IRS_CHECK_HIP(ctx, hipMemcpyAsync(seq_final, ctx->bm[fin].seq, rows * ctx->dims.max_len * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    return IRS_OK;
}

extern "C" int irs_generate_paths(irs_ctx *ctx, int64_t *seq, const int64_t *user, int32_t *hep, int32_t B,
                                  int32_t max_path_len, int32_t k, int32_t sweep, int32_t sample, int32_t sample_k,
                                  uint64_t seed, int32_t use_graph, float *paths, int32_t *status, void *stream) {
    int rc = check_search(ctx, "irs_generate_paths", seq && hep && paths && status, B, 0, max_path_len, k, sweep, sample, sample_k);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = irs_search_begin(ctx, status, B, s))) return rc;
    const irs_path_args pa = loop_path_args(ctx, seq, hep, paths, max_path_len, sample, sample_k, seed, status, paths);
    if (irs_may_capture(ctx, use_graph)) { // one step per graph; a captured step never carries emission thresholds
        irs_step_key key = {};
        key.kind = IRS_STEP_GREEDY, key.B = B, key.P = max_path_len, key.k = k, key.sweep = sweep;
        key.sample = sample, key.sample_k = sample_k, key.seed = seed;
        key.seq = seq, key.user = user, key.hep = hep, key.paths = paths, key.status = status;
        return irs_replay_steps(ctx, &ctx->g_greedy, key, [&](hipStream_t q) {
            return enqueue_step(ctx, pa, user, B, k, sweep, q);
        }, max_path_len, s);
    }
    for (int i = 0; i < max_path_len; ++i) // (steps behind the first may reuse the previous step's emission thresholds)
        if ((rc = enqueue_step(ctx, pa, user, B, k, sweep, s, i > 0))) return rc;
    return IRS_OK;
}

// The same search, stopped where it has arrived: a user is finished after the step that chose its target (seq[b][L - 1]).  Steps
// run on the live users only, compacted (stable order) into the workspace after every check_every-th step; the chosen item of a
// compacted row is scattered to the caller's row through the index map.  The batch size of a step is decided on the host from a
// 4-byte copy of the live count, so this loop is never captured.
extern "C" int irs_generate_paths_until(irs_ctx *ctx, int64_t *seq, const int64_t *user, int32_t *hep, int32_t B,
                                        int32_t max_path_len, int32_t k, int32_t sweep, int32_t sample, int32_t sample_k,
                                        uint64_t seed, int32_t check_every, float *paths, int32_t *status, int64_t *host_stats,
                                        void *stream) {
    int rc = check_search(ctx, "irs_generate_paths_until", seq && hep && paths && status, B, 0, max_path_len, k, sweep, sample, sample_k);
    if (rc) return rc;
    if (check_every < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_generate_paths_until: check_every must be >= 1");
    if (max_path_len > IRS_MAX_PATH)
        IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_generate_paths_until: max_path_len %d > %d", max_path_len, IRS_MAX_PATH);
    hipStream_t s = (hipStream_t)stream;
    const int P = max_path_len;
    if ((rc = irs_search_begin(ctx, status, B, s))) return rc;
    IRS_CHECK_HIP(ctx, hipMemsetAsync(ctx->un_fin, 0, sizeof(int32_t) * B, s));
    IRS_CHECK_HIP(ctx, hipMemsetAsync(ctx->un_status, 0, sizeof(int32_t) * B, s));
    if ((rc = irs_opt_zero_records(ctx, B, s))) return rc;
    // the first steps run in place on the caller's rows (identity map); the first compaction that removes a row moves the rest.
    // (the step writes stage[row][i]: it reads the index from the same device counter as irs_generate_paths' steps)
    irs_path_args pa = loop_path_args(ctx, seq, hep, ctx->un_stage, P, sample, sample_k, seed, ctx->un_status, paths);
    const int64_t *cuser = user;
    const int32_t *cmap = nullptr;
    int live = B, side = 0, carry = 0;
    int64_t steps = 0, row_steps = 0;
    // (an error below returns at once: host_stats unwritten, paths / status / seq / hep partly written -- see the header; the step
    //  counter pair is left wherever the last step put it, and every search loop resets it in irs_search_begin)
    for (int i = 0; i < P && live > 0; ++i) {
        if ((rc = enqueue_step(ctx, pa, cuser, live, k, sweep, s, carry, ctx->un_fin, cmap))) return rc;
        if ((rc = irs_launch_until_record(ctx, ctx->un_stage, P, i, cmap, pa.seq, live, ctx->un_fin, ctx->un_status, paths, status, s)))
            return rc;
        ++steps, row_steps += live, carry = 1;
        if ((i + 1) % check_every || i + 1 == P) continue; // no check due, or nothing left to decide after the last step
        int left;
        if ((rc = live_count(ctx, "irs_generate_paths_until", "rows", ctx->un_fin, live, &left, s))) return rc;
        if (left == live) continue;
        if (left > 0) {
            if ((rc = irs_launch_until_gather(ctx, ctx->un_dst, live, pa.seq, cuser, pa.hep, cmap, ctx->un_seq[side], ctx->un_user[side],
                                              ctx->un_hep[side], ctx->un_map[side], s)))
                return rc;
            pa.seq = ctx->un_seq[side], cuser = cuser ? ctx->un_user[side] : nullptr, pa.hep = ctx->un_hep[side], cmap = ctx->un_map[side];
            pa.ex.map = cmap; // (a compacted row keeps its user's list, and under no_repeat its row of the caller's paths)
            side ^= 1;
            IRS_CHECK_HIP(ctx, hipMemsetAsync(ctx->un_fin, 0, sizeof(int32_t) * left, s));
            // B <= 64 hands the step index over in a second word that larger batches do not keep: both words, from the host's count
            if ((rc = irs_launch_set_step(ctx, ctx->step_ctr, i + 1, s))) return rc;
        }
        live = left;
        carry = 0; // other rows, another M: the next top-k selects its thresholds afresh
    }
    if (host_stats) host_stats[0] = steps, host_stats[1] = row_steps;
    return IRS_OK;
}

// ------------------------------------------------------------------ beam search
// (a step only reads its input state: the public steps' const inputs go into the kernels' one state type)
static irs_beam_state beam_state(const int64_t *seq, const int32_t *hep, const double *cum, const float *paths, const int32_t *fin) {
    return irs_beam_state{(int64_t *)seq, (int32_t *)hep, (double *)cum, (float *)paths, (int32_t *)fin};
}

extern "C" int irs_beam_step(irs_ctx *ctx, const int64_t *seq_in, const int32_t *hep_in, const double *cum_in,
                             const float *paths_in, const float *val, const int64_t *ids0, const float *lse_max,
                             const float *lse_sum, int32_t B, int32_t W, int32_t k, int32_t step, int32_t P,
                             int64_t *seq_out, int32_t *hep_out, double *cum_out, float *paths_out, int32_t *status,
                             void *stream) {
    if (!ctx) return IRS_E_INVALID;
    if (!seq_in || !hep_in || !cum_in || !paths_in || !val || !ids0 || !seq_out || !hep_out || !cum_out || !paths_out ||
        !status || B < 1 || W < 1 || k < 1 || P < 1 || step < 0 || step >= P)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step: bad arguments");
    if (W > 1 && (!lse_max || !lse_sum)) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step: W > 1 needs the row log-sum-exp");
    const int rc = search_rules(ctx, "irs_beam_step", AT_BEAM_STEP, search_call{B, W, P, k, 0, 0, 0, true});
    if (rc) return rc;
    const irs_beam_cand cand{val, ids0, W > 1 ? lse_max : nullptr, W > 1 ? lse_sum : nullptr, k,
                             excl_args(ctx, W, nullptr, paths_in, P, 0, nullptr, step)};
    return irs_launch_beam_step(ctx, beam_state(seq_in, hep_in, cum_in, paths_in, nullptr), {seq_out, hep_out, cum_out, paths_out, nullptr},
                                cand, B, W, step, nullptr, P, status, nullptr, (hipStream_t)stream);
}

// The tail of every beam loop's step, the sharded one's too: the beam step from side `in` to the other on the lists in top_val /
// top_ids, then the step counter.  until == nullptr: the plain step
int irs_enqueue_beam_tail(irs_ctx *ctx, int in, const float *lse_max, const float *lse_sum, int B, int W, int k, int P, int32_t *status,
                          const irs_beam_until *until, hipStream_t s, const irs_excl *ex) {
    const irs_beam_cand cand{ctx->top_val, ctx->top_ids, lse_max, lse_sum, k, ex ? *ex : irs_excl{}};
    const int rc = irs_launch_beam_step(ctx, ctx->bm[in], ctx->bm[in ^ 1], cand, B, W, 0, ctx->step_ctr, P, status, until, s);
    return rc ? rc : irs_launch_inc(ctx, ctx->step_ctr, s);
}

// one beam step of B users on one device: decode -> top-k (+ log-sum-exp) of the B * W rows -> beam step -> step counter
static int enqueue_beam_step(irs_ctx *ctx, int in, const int64_t *user, int B, int W, int k, int sweep, int P, int32_t *status,
                             const irs_beam_until *until, hipStream_t s) {
    const int rows = B * W;
    float *const lmax = W > 1 ? ctx->lse_max : nullptr, *const lsum = W > 1 ? ctx->lse_sum : nullptr;
    int rc;
    if ((rc = irs_launch_decode(ctx, ctx->bm[in].seq, user, rows, nullptr, ctx->bm[in].hep, ctx->xrows, nullptr, s))) return rc;
    // W > 1: top-k and log-sum-exp out of one call (one pass over the float32 catalog on the swept path)
    if ((rc = launch_lists(ctx, ctx->xrows, rows, k, sweep, ctx->top_val, ctx->top_ids, ctx->row_status, s, lmax, lsum, 0))) return rc;
    // bound exclusions: a beam row's user through the loop's map, its path so far in the step's input state
    const irs_excl ex = excl_args(ctx, W, until ? until->map : nullptr, ctx->bm[in].paths, P, 0, ctx->step_ctr, 0);
    if (ctx->opt.surv.scratch) { // exact candidates: a live unfinished beam of a user that is not done sees its best W admissible items
        const irs_surv_args sa{ctx->xrows, ctx->bm[in].seq, ctx->bm[in].hep, rows, W, k, W, ctx->surv_rows, ctx->bm[in].cum,
                               until ? ctx->bm[in].fin : nullptr, until ? until->done : nullptr, ctx->top_val, ctx->top_ids, status,
                               until ? until->map : nullptr, ex};
        if ((rc = irs_launch_survivors(ctx, sa, ctx->opt.surv.scratch, s))) return rc;
    }
    const auto &bt = ctx->opt.btrace;
    if (!bt.on) return irs_enqueue_beam_tail(ctx, in, lmax, lsum, B, W, k, P, status, until, s, &ex);
    // A bound beam trace: how the target stands on every row of the step's INPUT state, before the step chooses (where the greedy
    // loop puts the same sweep); the linked step; the carry, at the caller's user rows; then the step counter.  The sweep writes
    // its partials to ctx->lse_part and its results to the bound scratch: of what the step still reads, lse_max / lse_sum were
    // reduced out of lse_part by the top-k call above, and top_val / top_ids / row_status are not the sweep's to write.
    irs_trace_rows tr;
    irs_beam_link lk;
    irs_beam_trace_layout(bt.scratch, bt.users * bt.W, &tr, &lk);
    if ((rc = irs_launch_target_trace(ctx, ctx->xrows, ctx->bm[in].seq, ctx->bm[in].hep, rows, tr, tr.mx, tr.sm, tr.ts, tr.rank, s))) return rc;
    const irs_beam_cand cand{ctx->top_val, ctx->top_ids, lmax, lsum, k, ex};
    // a beam rule: the ruled form of the linked step reads the sweep's four values where the sweep has just left them
    const auto &br = ctx->opt.brule;
    const auto &of = ctx->opt.offer;
    const irs_beam_rule ru{tr.mx, tr.sm, tr.ts, tr.rank, br.rank, br.lp, br.weight, ctx->dims.n_item, of.on ? of.ids : nullptr,
                           of.on ? (int)of.n : 0};
    if ((rc = irs_launch_beam_step(ctx, ctx->bm[in], ctx->bm[in ^ 1], cand, B, W, 0, ctx->step_ctr, P, status, until, s, &lk,
                                   br.on ? &ru : nullptr)))
        return rc;
    const irs_beam_carry_args ca{lk, tr.mx, tr.sm, tr.ts, tr.rank, W, bt.ld, 0, ctx->step_ctr, bt.item, bt.target, bt.rank,
                                 until ? until->map : nullptr};
    if ((rc = irs_launch_beam_trace_carry(ctx, ca, B, s))) return rc;
    return irs_launch_inc(ctx, ctx->step_ctr, s);
}

// a beam loop under a bound beam trace starts from zeros in rows [0, B) of the three arrays, all ld columns
static int beam_trace_zero(irs_ctx *ctx, int B, hipStream_t s) {
    const auto &bt = ctx->opt.btrace;
    if (!bt.on) return IRS_OK;
    const size_t n = (size_t)B * bt.W * bt.ld * 4;
    IRS_CHECK_HIP(ctx, hipMemsetAsync(bt.item, 0, n, s));
    IRS_CHECK_HIP(ctx, hipMemsetAsync(bt.target, 0, n, s));
    IRS_CHECK_HIP(ctx, hipMemsetAsync(bt.rank, 0, n, s));
    return IRS_OK;
}

extern "C" int irs_beam_search(irs_ctx *ctx, const int64_t *seq0, const int64_t *user, const int32_t *hep0, int32_t B,
                               int32_t W, int32_t P, int32_t k, int32_t sweep, int32_t use_graph, float *paths,
                               double *scores, int64_t *seq_final, int32_t *status, void *stream) {
    int rc = check_search(ctx, "irs_beam_search", seq0 && hep0 && paths && scores && status, B, W, P, k, sweep, 0, 0);
    if (rc) return rc;
    if (ctx->dims.mask_mode == IRS_MASK_IRN && !user) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_search: user is null");
    hipStream_t s = (hipStream_t)stream;
    int64_t *const usr = ctx->bm_side[0].user;
    if ((rc = irs_search_begin(ctx, status, B, s))) return rc;
    if ((rc = beam_trace_zero(ctx, B, s))) return rc;
    if ((rc = irs_launch_beam_init(ctx, seq0, user, hep0, B, W, P, ctx->bm[0], usr, s))) return rc;
    int done = 0;
    if (irs_may_capture(ctx, use_graph) && P >= 2) { // the two ping-pong steps per graph; an odd last step runs on the stream
        irs_step_key key = {}; // (the steps work on the context's beam buffers: of the caller's pointers only `status` is baked in)
        key.kind = IRS_STEP_BEAM, key.B = B, key.W = W, key.P = P, key.k = k, key.sweep = sweep, key.status = status;
        if ((rc = irs_replay_steps(ctx, &ctx->g_beam, key, [&](hipStream_t q) {
                int r = enqueue_beam_step(ctx, 0, usr, B, W, k, sweep, P, status, nullptr, q);
                return r ? r : enqueue_beam_step(ctx, 1, usr, B, W, k, sweep, P, status, nullptr, q);
            }, P / 2, s)))
            return rc;
        done = P / 2 * 2;
    }
    for (; done < P; ++done)
        if ((rc = enqueue_beam_step(ctx, done & 1, usr, B, W, k, sweep, P, status, nullptr, s))) return rc;
    return irs_beam_finish(ctx, (size_t)B * W, P, paths, scores, seq_final, s);
}

// ------------------------------------------------------------------ beam search with an end symbol
extern "C" int irs_beam_step_until(irs_ctx *ctx, const int64_t *seq_in, const int32_t *hep_in, const double *cum_in,
                                   const float *paths_in, const int32_t *fin_in, const float *val, const int64_t *ids0,
                                   const float *lse_max, const float *lse_sum, int32_t B, int32_t W, int32_t k, int32_t step,
                                   int32_t P, int32_t stop_rule, int64_t *seq_out, int32_t *hep_out, double *cum_out,
                                   float *paths_out, int32_t *fin_out, int32_t *done, int32_t *status, void *stream) {
    if (!ctx) return IRS_E_INVALID;
    if (!seq_in || !hep_in || !cum_in || !paths_in || !fin_in || !val || !ids0 || !seq_out || !hep_out || !cum_out ||
        !paths_out || !fin_out || !done || !status || B < 1 || W < 1 || k < 1 || P < 1 || step < 0 || step >= P)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_until: bad arguments");
    if (W > 1 && (!lse_max || !lse_sum)) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_until: W > 1 needs the row log-sum-exp");
    if (stop_rule != IRS_BEAM_STOP_ALL && stop_rule != IRS_BEAM_STOP_BEST)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_until: stop_rule %d (IRS_BEAM_STOP_ALL or IRS_BEAM_STOP_BEST)", stop_rule);
    const int rc = search_rules(ctx, "irs_beam_step_until", AT_BEAM_STEP, search_call{B, W, P, k, 0, 0, 0, true});
    if (rc) return rc;
    const irs_beam_cand cand{val, ids0, W > 1 ? lse_max : nullptr, W > 1 ? lse_sum : nullptr, k,
                             excl_args(ctx, W, nullptr, paths_in, P, 0, nullptr, step)};
    const irs_beam_until until{done, nullptr, stop_rule};
    return irs_launch_beam_step(ctx, beam_state(seq_in, hep_in, cum_in, paths_in, fin_in), {seq_out, hep_out, cum_out, paths_out, fin_out},
                                cand, B, W, step, nullptr, P, status, &until, (hipStream_t)stream);
}

// either beam step, with the link word and the chosen candidate's list value per output row (irs_beam_trace_carry's inputs);
// synchronous on the null stream, like the carry alone and the two lookahead kernels alone (look_run_sync)
extern "C" int irs_beam_step_linked(irs_ctx *ctx, const int64_t *seq_in, const int32_t *hep_in, const double *cum_in,
                                    const float *paths_in, const int32_t *fin_in, const float *val, const int64_t *ids0,
                                    const float *lse_max, const float *lse_sum, int32_t B, int32_t W, int32_t k, int32_t step,
                                    int32_t P, int32_t stop_rule, int64_t *seq_out, int32_t *hep_out, double *cum_out,
                                    float *paths_out, int32_t *fin_out, int32_t *done, int32_t *status, int32_t *link,
                                    float *link_val) {
    if (!ctx) return IRS_E_INVALID;
    if (!seq_in || !hep_in || !cum_in || !paths_in || !val || !ids0 || !seq_out || !hep_out || !cum_out || !paths_out || !status ||
        !link || !link_val || B < 1 || W < 1 || k < 1 || P < 1 || step < 0 || step >= P)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_linked: bad arguments");
    const bool until_form = fin_in && fin_out && done;
    if (!until_form && (fin_in || fin_out || done))
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_linked: dev_fin_in, dev_fin_out and dev_done go together");
    if (W > 1 && (!lse_max || !lse_sum)) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_linked: W > 1 needs the row log-sum-exp");
    if (until_form && stop_rule != IRS_BEAM_STOP_ALL && stop_rule != IRS_BEAM_STOP_BEST)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_linked: stop_rule %d (IRS_BEAM_STOP_ALL or IRS_BEAM_STOP_BEST)", stop_rule);
    const int rc = search_rules(ctx, "irs_beam_step_linked", AT_BEAM_STEP_LINKED, search_call{B, W, P, k, 0, 0, 0, true});
    if (rc) return rc;
    const irs_beam_cand cand{val, ids0, W > 1 ? lse_max : nullptr, W > 1 ? lse_sum : nullptr, k,
                             excl_args(ctx, W, nullptr, paths_in, P, 0, nullptr, step)};
    const irs_beam_until until{done, nullptr, stop_rule};
    const irs_beam_link lk{link, link_val};
    return look_run_sync(ctx, irs_launch_beam_step(ctx, beam_state(seq_in, hep_in, cum_in, paths_in, fin_in),
                                                   {seq_out, hep_out, cum_out, paths_out, fin_out}, cand, B, W, step, nullptr, P, status,
                                                   until_form ? &until : nullptr, nullptr, &lk));
}

// the linked step under a rule given as arguments (irs_hip.h, "beam rule"): what the loops launch while irs_set_beam_rule holds one
extern "C" int irs_beam_step_ruled(irs_ctx *ctx, const int64_t *seq_in, const int32_t *hep_in, const double *cum_in,
                                   const float *paths_in, const int32_t *fin_in, const float *val, const int64_t *ids0,
                                   const float *lse_max, const float *lse_sum, int32_t B, int32_t W, int32_t k, int32_t step,
                                   int32_t P, int32_t stop_rule, int64_t *seq_out, int32_t *hep_out, double *cum_out,
                                   float *paths_out, int32_t *fin_out, int32_t *done, int32_t *status, int32_t *link,
                                   float *link_val, const float *mx, const float *sm, const float *tscore, const int32_t *rank,
                                   int32_t rank_max, float lp_min, float target_weight) {
    if (!ctx) return IRS_E_INVALID;
    if (!seq_in || !hep_in || !cum_in || !paths_in || !val || !ids0 || !seq_out || !hep_out || !cum_out || !paths_out || !status ||
        !link || !link_val || !mx || !sm || !tscore || !rank || B < 1 || W < 1 || k < 1 || P < 1 || step < 0 || step >= P)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_ruled: bad arguments");
    const bool until_form = fin_in && fin_out && done;
    if (!until_form && (fin_in || fin_out || done))
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_ruled: dev_fin_in, dev_fin_out and dev_done go together");
    if (W > 1 && (!lse_max || !lse_sum)) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_ruled: W > 1 needs the row log-sum-exp");
    if (until_form && stop_rule != IRS_BEAM_STOP_ALL && stop_rule != IRS_BEAM_STOP_BEST)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_ruled: stop_rule %d (IRS_BEAM_STOP_ALL or IRS_BEAM_STOP_BEST)", stop_rule);
    if (rank_max < 0) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_ruled: rank_max must be >= 0 (0: the rank clause is off)");
    if (!beam_weight_ok(target_weight)) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_ruled: target_weight must be finite and >= 0 (0: ranking is off)");
    const bool lp_on = irs_arrival_lp_on(lp_min);
    if (rank_max == 0 && !lp_on && !(target_weight > 0.f)) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_step_ruled: all clauses are off");
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_beam_step_ruled needs the whole catalog on one device");
    const int rc = search_rules(ctx, "irs_beam_step_ruled", AT_BEAM_STEP_RULED, search_call{B, W, P, k, 0, 0, 0, true});
    if (rc) return rc;
    const irs_beam_cand cand{val, ids0, W > 1 ? lse_max : nullptr, W > 1 ? lse_sum : nullptr, k,
                             excl_args(ctx, W, nullptr, paths_in, P, 0, nullptr, step)};
    const irs_beam_until until{done, nullptr, stop_rule};
    const irs_beam_link lk{link, link_val};
    const auto &of = ctx->opt.offer;
    const irs_beam_rule ru{mx, sm, tscore, rank, rank_max, lp_on ? lp_min : __builtin_nanf(""), target_weight, ctx->dims.n_item,
                           of.on ? of.ids : nullptr, of.on ? (int)of.n : 0};
    return look_run_sync(ctx, irs_launch_beam_step(ctx, beam_state(seq_in, hep_in, cum_in, paths_in, fin_in),
                                                   {seq_out, hep_out, cum_out, paths_out, fin_out}, cand, B, W, step, nullptr, P, status,
                                                   until_form ? &until : nullptr, nullptr, &lk, &ru));
}

// The loop.  The beam state of the live users sits in side `cur` of ctx->bm; a step reads it and writes side cur ^ 1, a compaction
// reads THAT and writes the side the step has just freed.  user / done / map (`sd`) move at compactions only, between the two
// sides of ctx->bm_side and un_map.  The buffers and the step counter are the ones a cached beam graph bakes in: irs_beam_search
// re-initialises all of them.
extern "C" int irs_beam_search_until(irs_ctx *ctx, const int64_t *seq0, const int64_t *user, const int32_t *hep0, int32_t B,
                                     int32_t W, int32_t P, int32_t k, int32_t sweep, int32_t stop_rule, int32_t check_every,
                                     float *paths, double *scores, int32_t *fin, int64_t *seq_final, int32_t *status,
                                     int64_t *host_stats, void *stream) {
    int rc = check_search(ctx, "irs_beam_search_until", seq0 && hep0 && paths && scores && status, B, W, P, k, sweep, 0, 0);
    if (rc) return rc;
    if (ctx->dims.mask_mode == IRS_MASK_IRN && !user) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_search_until: user is null");
    if (stop_rule != IRS_BEAM_STOP_ALL && stop_rule != IRS_BEAM_STOP_BEST)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_search_until: stop_rule %d (IRS_BEAM_STOP_ALL or IRS_BEAM_STOP_BEST)", stop_rule);
    if (check_every < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_beam_search_until: check_every must be >= 1");
    hipStream_t s = (hipStream_t)stream;
    irs_beam_side sd = ctx->bm_side[0]; // (its map is null: the identity until the first compaction)
    const irs_beam_out res{paths, scores, fin, seq_final};
    if ((rc = irs_search_begin(ctx, status, B, s))) return rc;
    if ((rc = beam_trace_zero(ctx, B, s))) return rc;
    if ((rc = irs_launch_beam_init(ctx, seq0, user, hep0, B, W, P, ctx->bm[0], sd.user, s))) return rc;
    IRS_CHECK_HIP(ctx, hipMemsetAsync(ctx->bm[0].fin, 0, sizeof(int32_t) * B * W, s));
    IRS_CHECK_HIP(ctx, hipMemsetAsync(sd.done, 0, sizeof(int32_t) * B, s));
    int live = B, cur = 0, aux = 0;
    int64_t steps = 0, window_steps = 0;
    for (int i = 0; i < P; ++i) {
        const irs_beam_until until{sd.done, sd.map, stop_rule};
        if ((rc = enqueue_beam_step(ctx, cur, sd.user, live, W, k, sweep, P, status, &until, s))) return rc;
        cur ^= 1, ++steps, window_steps += live * W;
        if ((i + 1) % check_every || i + 1 == P) continue; // no check due, or the last step: whoever is left leaves below
        int left;
        if ((rc = live_count(ctx, "irs_beam_search_until", "users", sd.done, live, &left, s))) return rc;
        if (left == live) continue;
        aux ^= 1; // the survivors move to the side the step has just read (free), and to the other side of user / done / map
        const irs_beam_side to{ctx->bm_side[aux].user, ctx->bm_side[aux].done, ctx->un_map[aux]};
        if ((rc = irs_launch_beam_retire(ctx, ctx->un_dst, live, W, P, ctx->bm[cur], sd, ctx->bm[cur ^ 1], to, res, s))) return rc;
        cur ^= 1, sd = to, live = left;
        if (live == 0) break;
    }
    if (live > 0 && (rc = irs_launch_beam_retire(ctx, nullptr, live, W, P, ctx->bm[cur], sd, {}, {}, res, s))) return rc;
    if (host_stats) host_stats[0] = steps, host_stats[1] = window_steps;
    return IRS_OK;
}

// ------------------------------------------------------------------ profiling hooks
void irs_prof_begin(irs_ctx *ctx, int family, hipStream_t s) {
    if (ctx->prof_family != family) return;
    if (ctx->prof_n == ctx->prof_cap) {
        int ncap = ctx->prof_cap ? ctx->prof_cap * 2 : 256;
        irs_prof_ev *n = (irs_prof_ev *)realloc(ctx->prof_ev, sizeof(irs_prof_ev) * ncap);
        if (!n) return;
        for (int i = ctx->prof_cap; i < ncap; ++i) {
            hipEventCreate(&n[i].a);
            hipEventCreate(&n[i].b);
        }
        ctx->prof_ev = n;
        ctx->prof_cap = ncap;
    }
    hipEventRecord(ctx->prof_ev[ctx->prof_n].a, s);
}

void irs_prof_end(irs_ctx *ctx, int family, hipStream_t s, double flops, double bytes) {
    if (ctx->prof_family != family) return;
    if (ctx->prof_n >= ctx->prof_cap) return;
    hipEventRecord(ctx->prof_ev[ctx->prof_n].b, s);
    ctx->prof_n++;
    ctx->prof_flops += flops;
    ctx->prof_bytes += bytes;
}

extern "C" int irs_prof_enable(irs_ctx *ctx, int32_t family) {
    if (!ctx) return IRS_E_INVALID;
    ctx->prof_family = family;
    ctx->prof_n = 0;
    ctx->prof_flops = 0;
    ctx->prof_bytes = 0;
    return IRS_OK;
}

extern "C" int irs_prof_read(irs_ctx *ctx, int32_t *launches, double *total_ms, double *total_flops, double *total_bytes) {
    if (!ctx) return IRS_E_INVALID;
    double ms = 0;
    for (int i = 0; i < ctx->prof_n; ++i) {
        IRS_CHECK_HIP(ctx, hipEventSynchronize(ctx->prof_ev[i].b));
        float t = 0;
        IRS_CHECK_HIP(ctx, hipEventElapsedTime(&t, ctx->prof_ev[i].a, ctx->prof_ev[i].b));
        ms += t;
    }
    if (launches) *launches = ctx->prof_n;
    if (total_ms) *total_ms = ms;
    if (total_flops) *total_flops = ctx->prof_flops;
    if (total_bytes) *total_bytes = ctx->prof_bytes;
    ctx->prof_n = 0;
    ctx->prof_flops = 0;
    ctx->prof_bytes = 0;
    return IRS_OK;
}
