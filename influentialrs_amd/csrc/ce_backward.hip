// Backward of projection + cross entropy without dL/dlogits (include/irs_hip.h: irs_ce_backward; reference
// influentialRS.py:278-310 and evaluator.py:53-68, the autograd of nn.Linear + nn.CrossEntropyLoss).
//
//   G[m][j] = scale * (exp(logit_mj - lse[m]) - [j == label[m]]),   dx = G W,   dw (+)= G^T X,   db (+)= colsum G
//
// G is never stored: two passes over (rows x items) each recompute the logits tile they need on v_mfma_f32_32x32x2f32,
// turn it into G in registers and feed those registers straight back into the matrix pipe.
//
// One kernel serves both passes.  A wave OWNS a 32-index tile of one side (its operand fragments and its [32, d] output
// tile stay in registers for the whole walk) and WALKS 32-index tiles of the other side, which the workgroup's four
// waves share through a double-buffered row-major LDS image:
//   ITEM = true   owns items, walks rows:  out = dw tile, db is the column sum of the same G registers
//   ITEM = false  owns rows, walks items:  out = dx tile
// Per walked tile:
//   1. logits D[walk][own] = Q P^T (+ bias): A = the walked rows from LDS, B = the owned fragments.  Lane (r, h) of the
//      result holds own index r and walk indices (i & 3) + 8 (i >> 2) + 4 h in register i.
//   2. G in place (the per-own-index terms are per lane, the per-walk-index terms come from LDS).
//   3. out[own][c] += sum_walk G[walk][own] Q[walk][c]: register i of G IS a valid A operand of the 32x32x2 form with
//      k = walk index -- lane (own r, half h) supplies k = h, i.e. walk indices w_i and w_i + 4 -- against
//      B = Q[w_i + 4 h][32 ct + r] read from the same LDS image.  Sixteen matrix instructions per 32 output columns;
//      the k pairing fixes a summation order and nothing else.
// When the owned side has too few tiles to fill the device the walk is split over a fixed number of groups (a function
// of the shape alone), each group writes a partial output to the caller's scratch and k_ce_bwd_sum adds the partials in
// group order.  No atomics: two identical calls give identical bits.
#include "irs_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct CeBwdArgs {
    const float *own;       // [n_own, d]  ITEM: project.weight, else the rows
    const float *walk;      // [n_walk, d] the other one
    const float *bias;      // [n_local]
    const float *lse;       // [M]
    const int64_t *labels0; // [M] global 0-based, < 0: row ignored
    int64_t n_own, n_walk, n_local, item_lo;
    int d;
    int tiles_per_group; // walked tiles per group
    int groups;
    int accumulate;      // groups == 1: add to out / out_b instead of overwriting them
    float scale;
    float *out;          // groups == 1: [n_own, d]; else partials [groups][n_own, d]
    float *out_b;        // ITEM: db [n_local] or partials [groups][n_local]
};

// label of a row as a local column (or -1: matches none) and the row's log-sum-exp (+inf: ignored row, exp() = 0)
__device__ __forceinline__ void ce_row_terms(const CeBwdArgs &a, int64_t row, int64_t n_rows, float &lse, int &lab) {
    lse = INFINITY;
    lab = -1;
    if (row < n_rows) {
        const int64_t l = a.labels0[row];
        if (l >= 0) {
            lse = a.lse[row];
            const int64_t ll = l - a.item_lo;
            if (ll >= 0 && ll < a.n_local) lab = (int)ll;
        }
    }
}

template <int DP, bool ITEM, bool V4>
__global__ void __launch_bounds__(256, DP > 128 ? 1 : 2) k_ce_bwd(CeBwdArgs a) {
    constexpr int QN = DP / 8;   // float4 k groups per row
    constexpr int CT = DP / 32;  // 32-column tiles of the output
    constexpr int LD = DP + 4;   // LDS row pitch (floats)
    constexpr int VW = V4 ? 4 : 2;
    constexpr int NV = 32 * DP / VW / 256; // staging loads per thread
    static_assert(NV >= 1, "tile smaller than the workgroup");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *tile = reinterpret_cast<float *>(smem);          // [2][32][LD]
    float *aux_f = tile + 2 * 32 * LD;                      // [2][32] ITEM: lse of the walked rows; else bias of the walked items
    int *aux_i = reinterpret_cast<int *>(aux_f + 64);       // [2][32] ITEM: local label of the walked rows

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int group = blockIdx.y;
    const int64_t n_walk_tiles = (a.n_walk + 31) / 32;
    const int64_t t0 = (int64_t)group * a.tiles_per_group;
    const int64_t t1 = min(t0 + (int64_t)a.tiles_per_group, n_walk_tiles);
    const int64_t own0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
    const int64_t own_r = own0 + r;

    // owned fragments: lane (r, h) holds k = 8 q + 4 h .. + 3 of its index (the same pairing of k on both operands)
    float4 pf[QN];
#pragma unroll
    for (int q = 0; q < QN; ++q) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const int k = 8 * q + 4 * h;
        if (own_r < a.n_own) {
            const float *p = a.own + (size_t)own_r * a.d;
            if (k < a.d) v.x = p[k];
            if (k + 1 < a.d) v.y = p[k + 1];
            if (k + 2 < a.d) v.z = p[k + 2];
            if (k + 3 < a.d) v.w = p[k + 3];
        }
        pf[q] = v;
    }
    // the per-lane terms of G
    float own_f; // ITEM: bias of the item (-inf beyond the catalog: exp() = 0); else lse of the row
    int own_i;   // ITEM: local item index; else local label of the row
    if (ITEM) {
        own_f = own_r < a.n_local ? a.bias[own_r] : -INFINITY;
        own_i = (int)own_r;
    } else {
        ce_row_terms(a, own_r, a.n_own, own_f, own_i);
    }

    f32x16 oacc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[ct][i] = 0.f;
    float bsum = 0.f;

    // staging of one walked tile: global -> registers -> LDS image [32][LD] (zeros beyond d and beyond n_walk)
    float4 pre4[V4 ? NV : 1];
    float2 pre2[V4 ? 1 : NV];
    float pre_f = 0.f;
    int pre_i = -1;
    auto fetch = [&](int64_t t) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int idx = tid + 256 * j;
            const int row = idx / (DP / VW), k = (idx % (DP / VW)) * VW;
            const int64_t g = t * 32 + row;
            const bool ok = g < a.n_walk && k < a.d;
            const float *p = a.walk + (size_t)(ok ? g : 0) * a.d + (ok ? k : 0);
            if (V4) {
                float4 v = *reinterpret_cast<const float4 *>(p);
                pre4[j] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                float2 v = *reinterpret_cast<const float2 *>(p);
                pre2[j] = ok ? v : make_float2(0.f, 0.f);
            }
        }
        if (tid < 32) {
            const int64_t g = t * 32 + tid;
            if (ITEM) ce_row_terms(a, g, a.n_walk, pre_f, pre_i);
            else pre_f = g < a.n_local ? a.bias[g] : -INFINITY;
        }
    };
    auto stage = [&](int buf) {
        float *dst = tile + buf * 32 * LD;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int idx = tid + 256 * j;
            const int row = idx / (DP / VW), k = (idx % (DP / VW)) * VW;
            if (V4) *reinterpret_cast<float4 *>(dst + row * LD + k) = pre4[j];
            else *reinterpret_cast<float2 *>(dst + row * LD + k) = pre2[j];
        }
        if (tid < 32) {
            aux_f[buf * 32 + tid] = pre_f;
            if (ITEM) aux_i[buf * 32 + tid] = pre_i;
        }
    };

    if (t0 < t1) {
        fetch(t0);
        stage(0);
    }
    __syncthreads();
    const bool live = __builtin_amdgcn_readfirstlane(own0 < a.n_own ? 1 : 0) != 0; // a wave without a tile only helps staging
    for (int64_t t = t0; t < t1; ++t) {
        const int cur = (int)(t - t0) & 1;
        const bool more = t + 1 < t1;
        if (more) fetch(t + 1);
        const float *q_ = tile + cur * 32 * LD;
        if (live) {
        // 1. logits, seeded with the bias
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = ITEM ? own_f : aux_f[cur * 32 + (i & 3) + 8 * (i >> 2) + 4 * h];
#pragma unroll
        for (int q = 0; q < QN; ++q) {
            const float4 av = *reinterpret_cast<const float4 *>(q_ + r * LD + 8 * q + 4 * h);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, pf[q].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, pf[q].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, pf[q].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, pf[q].w, acc, 0, 0, 0);
        }
        // 2. G in place
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int wi = (i & 3) + 8 * (i >> 2) + 4 * h; // walked index within the tile
            float p;
            bool hit;
            if (ITEM) {
                p = __expf(acc[i] - aux_f[cur * 32 + wi]);
                hit = aux_i[cur * 32 + wi] == own_i;
            } else {
                p = __expf(acc[i] - own_f);
                hit = (int)(t * 32) + wi == own_i;
            }
            acc[i] = a.scale * (p - (hit ? 1.f : 0.f));
        }
        if (ITEM) {
#pragma unroll
            for (int i = 0; i < 16; ++i) bsum += acc[i];
        }
        // 3. out[own][c] += sum_walk G[walk][own] Q[walk][c]
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int wi = (i & 3) + 8 * (i >> 2) + 4 * h;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const float bq = q_[wi * LD + 32 * ct + r];
                oacc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[i], bq, oacc[ct], 0, 0, 0);
            }
        }
        }
        if (more) stage(cur ^ 1);
        __syncthreads();
    }

    // the owned output tile: register i of column tile ct is out[own0 + (i & 3) + 8 (i >> 2) + 4 h][32 ct + r]
    float *out = a.out + (a.groups > 1 ? (size_t)group * (size_t)a.n_own * a.d : 0);
    const bool add = a.groups == 1 && a.accumulate;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int col = 32 * ct + r;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t row = own0 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (row < a.n_own && col < a.d) {
                float *dst = out + (size_t)row * a.d + col;
                *dst = add ? *dst + oacc[ct][i] : oacc[ct][i];
            }
        }
    }
    if (ITEM) {
        const float tot = bsum + __shfl_xor(bsum, 32, 64); // rows 4 h + .. of both halves; a + b is the same on both lanes
        if (h == 0 && own_r < a.n_local) {
            float *dst = a.out_b + (a.groups > 1 ? (size_t)group * (size_t)a.n_local : 0) + own_r;
            *dst = add ? *dst + tot : tot;
        }
    }
}

// out[i] (+)= part[0][i] + part[1][i] + ..., in group order
__global__ void __launch_bounds__(256) k_ce_bwd_sum(const float *__restrict__ part, int groups, int64_t n, int accumulate,
                                                    float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int g = 1; g < groups; ++g) s += part[(size_t)g * n + i];
    out[i] = accumulate ? out[i] + s : s;
}

// ---- plan: how the two walks are split and where their partials live in the scratch.  A function of (M, n_local, d) alone.
#define CE_BWD_TARGET_WGS 512          // workgroups a pass aims for (two per CU)
#define CE_BWD_PART_BYTES (31u << 20)  // partials of one pass; both passes + alignment stay below 64 MiB
struct CeBwdPlan {
    int groups_w, tpg_w; // item-owned pass: row-tile groups
    int groups_x, tpg_x; // row-owned pass: item-tile groups
    size_t off_dw, off_db, off_dx, bytes;
};

static void ce_bwd_split(int64_t n_own, int64_t n_walk, size_t bytes_per_group, int *groups, int *tpg) {
    const int64_t wgs = ((n_own + 31) / 32 + 3) / 4, walk_tiles = (n_walk + 31) / 32;
    int64_t g = CE_BWD_TARGET_WGS / wgs;
    if (g > walk_tiles) g = walk_tiles;
    if (g > (int64_t)(CE_BWD_PART_BYTES / bytes_per_group)) g = (int64_t)(CE_BWD_PART_BYTES / bytes_per_group);
    if (g < 2) g = 1;
    int64_t per = (walk_tiles + g - 1) / g;
    g = (walk_tiles + per - 1) / per; // no empty group
    *groups = (int)g;
    *tpg = (int)per;
}

static CeBwdPlan ce_bwd_plan(const irs_ctx *ctx, int M) {
    CeBwdPlan p;
    const int d = ctx->dims.d;
    const int64_t N = ctx->n_local;
    ce_bwd_split(N, M, (size_t)N * (d + 1) * 4, &p.groups_w, &p.tpg_w);
    ce_bwd_split(M, N, (size_t)M * d * 4, &p.groups_x, &p.tpg_x);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    p.off_dw = o;
    o += p.groups_w > 1 ? up((size_t)p.groups_w * N * d * 4) : 0;
    p.off_db = o;
    o += p.groups_w > 1 ? up((size_t)p.groups_w * N * 4) : 0;
    p.off_dx = o;
    o += p.groups_x > 1 ? up((size_t)p.groups_x * M * d * 4) : 0;
    p.bytes = o ? o : 256;
    return p;
}

template <int DP, bool ITEM>
static int ce_bwd_launch(irs_ctx *ctx, const CeBwdArgs &a, hipStream_t s) {
    const bool v4 = (a.d & 3) == 0 && ((((uintptr_t)a.own) | ((uintptr_t)a.walk)) & 15) == 0;
    const size_t smem = (size_t)(2 * 32 * (DP + 4) + 128) * 4;
    const dim3 grid((unsigned)(((a.n_own + 31) / 32 + 3) / 4), (unsigned)a.groups);
    if (v4) {
        IRS_ONCE_PER_DEVICE(IRS_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(k_ce_bwd<DP, ITEM, true>),
                                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)));
        hipLaunchKernelGGL((k_ce_bwd<DP, ITEM, true>), grid, dim3(256), smem, s, a);
    } else {
        IRS_ONCE_PER_DEVICE(IRS_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(k_ce_bwd<DP, ITEM, false>),
                                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)));
        hipLaunchKernelGGL((k_ce_bwd<DP, ITEM, false>), grid, dim3(256), smem, s, a);
    }
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

template <bool ITEM>
static int ce_bwd_pass(irs_ctx *ctx, const CeBwdArgs &a, hipStream_t s) {
    switch (ctx->d_pad) {
    case 16:
    case 32: return ce_bwd_launch<32, ITEM>(ctx, a, s);
    case 64: return ce_bwd_launch<64, ITEM>(ctx, a, s);
    case 128: return ce_bwd_launch<128, ITEM>(ctx, a, s);
    case 256: return ce_bwd_launch<256, ITEM>(ctx, a, s);
    default: IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "unsupported d_pad %d", ctx->d_pad);
    }
}

static int ce_bwd_sum(irs_ctx *ctx, const float *part, int groups, int64_t n, int accumulate, float *out, hipStream_t s) {
    hipLaunchKernelGGL(k_ce_bwd_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, groups, n, accumulate, out);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

size_t irs_ce_bwd_scratch(const irs_ctx *ctx, int M) { return ce_bwd_plan(ctx, M).bytes; }

extern "C" size_t irs_ce_backward_scratch_bytes(const irs_ctx *ctx, int32_t M) {
    if (!ctx || M < 1 || M > ctx->max_rows) return 0;
    return ce_bwd_plan(ctx, M).bytes;
}

extern "C" int irs_ce_backward(irs_ctx *ctx, const float *xrows, const int64_t *labels0, const float *lse, int32_t M,
                               float scale, int32_t accumulate, float *dx, float *dw, float *db, void *scratch,
                               size_t scratch_bytes, void *stream) {
    if (!ctx) return IRS_E_INVALID;
    if (ctx->shard.world != 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "irs_ce_backward needs the whole catalog on one device");
    if (!xrows || !labels0 || !lse || !dx || !dw || !db || !scratch) IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_backward: null arguments");
    if (M < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_backward: M=%d", M);
    if (M > ctx->max_rows) IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_backward: M=%d exceeds max_rows=%d", M, ctx->max_rows);
    const CeBwdPlan p = ce_bwd_plan(ctx, M);
    if (scratch_bytes < p.bytes) IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_backward: scratch too small: %zu < %zu", scratch_bytes, p.bytes);
    if (((uintptr_t)scratch) & 15) IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_backward: scratch must be 16-byte aligned");
    if (((uintptr_t)xrows) & 7) IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_backward: rows must be 8-byte aligned");
    if (!ctx->proj_w || !ctx->proj_b) IRS_FAIL(ctx, IRS_E_STATE, "irs_ce_backward: project.weight / project.bias not bound");
    ctx->proj_stale = true; // as irs_ce_forward: the caller is about to move project.* under the bf16 catalog copy
    return irs_launch_ce_backward(ctx, xrows, labels0, lse, M, scale, accumulate, dx, dw, db, scratch, (hipStream_t)stream);
}

// the two passes over this context's shard (irs_ce_backward; irs_ce_backward_sharded over the gathered rows)
int irs_launch_ce_backward(irs_ctx *ctx, const float *xrows, const int64_t *labels0, const float *lse, int M, float scale,
                           int accumulate, float *dx, float *dw, float *db, void *scratch, hipStream_t s) {
    const CeBwdPlan p = ce_bwd_plan(ctx, M);
    char *sc = static_cast<char *>(scratch);
    int rc;
    CeBwdArgs a;
    a.bias = ctx->proj_b;
    a.lse = lse;
    a.labels0 = labels0;
    a.n_local = ctx->n_local;
    a.item_lo = ctx->shard.item_lo;
    a.d = ctx->dims.d;
    a.scale = scale;

    // item-owned pass: dw, db
    a.own = ctx->proj_w;
    a.walk = xrows;
    a.n_own = ctx->n_local;
    a.n_walk = M;
    a.groups = p.groups_w;
    a.tiles_per_group = p.tpg_w;
    a.accumulate = accumulate != 0;
    a.out = p.groups_w > 1 ? reinterpret_cast<float *>(sc + p.off_dw) : dw;
    a.out_b = p.groups_w > 1 ? reinterpret_cast<float *>(sc + p.off_db) : db;
    if ((rc = ce_bwd_pass<true>(ctx, a, s))) return rc;
    if (p.groups_w > 1) {
        if ((rc = ce_bwd_sum(ctx, a.out, p.groups_w, ctx->n_local * a.d, accumulate != 0, dw, s))) return rc;
        if ((rc = ce_bwd_sum(ctx, a.out_b, p.groups_w, ctx->n_local, accumulate != 0, db, s))) return rc;
    }
    // row-owned pass: dx
    a.own = xrows;
    a.walk = ctx->proj_w;
    a.n_own = M;
    a.n_walk = ctx->n_local;
    a.groups = p.groups_x;
    a.tiles_per_group = p.tpg_x;
    a.accumulate = 0;
    a.out = p.groups_x > 1 ? reinterpret_cast<float *>(sc + p.off_dx) : dx;
    a.out_b = nullptr;
    if ((rc = ce_bwd_pass<false>(ctx, a, s))) return rc;
    if (p.groups_x > 1 && (rc = ce_bwd_sum(ctx, a.out, p.groups_x, (int64_t)M * a.d, 0, dx, s))) return rc;
    return IRS_OK;
}
