// Offer set: the exact ranked top-k over a bound subset of the catalog (irs_bind_offer_set / irs_score_topk_offer,
// include/irs_hip.h).  The set is a strictly ascending array of C 0-based item ids, shared by all rows.  Three kernels:
//   k_offer_prepare  the binding's one launch: the caller's ids, sanitised, into the scratch.  An entry outside [0, n_item) or
//                    not greater than its predecessor becomes a hole (-1), the entries behind C up to the tile edge are holes
//                    that are not counted; int32 word 0 of the scratch holds the number of counted holes.  Integer compares
//                    only: every later kernel indexes project.* with a sanitised id and nothing else.
//   k_offer_scores   float32 scores of a pass of rows against the set, [rows][C_pad] in the scratch.  A workgroup gathers the
//                    project rows of its 64-id tile into LDS (k-padding zero), every wave takes 16 of them as the B operand of
//                    v_mfma_f32_16x16x4_f32 into registers, and walks the pass's rows in groups of RT 16-row tiles staged
//                    through LDS: RT independent accumulators per wave, seeded with the item's bias.  One such MFMA is
//                    fma(a3, b3, fma(a2, b2, fma(a1, b1, fma(a0, b0, C)))) over its four k, so k-steps issued in ascending order
//                    give irs_chain's value bit for bit (score.hip: k_sweep_f32 relies on the same fact for 32x32x2).
//   k_offer_select   one workgroup per row streams the row's scores and keeps the best k keys (irs_fkey of the score, local
//                    index ascending) in LDS; values and global ids leave through the sanitised id array.  Local order is id
//                    order because the set ascends.  A hole is never emitted.
// The launcher walks M in passes of the rows the scratch holds.  No float atomics, and nothing depends on which workgroup
// finishes first: two identical calls give identical bits.
// Known corner: a chain that ends at exactly -0 and then meets zero k-padding comes out +0; the order is unaffected (irs_fkey
// folds the two).
#include "irs_internal.h"

#define OFFER_TILE 64   // ids per workgroup of k_offer_scores: C_pad = C rounded up to it
#define OFFER_ROW_WGS 64 // workgroups that share a tile's row groups, at most
#define OFFER_BUF 2048  // keys of LDS per selection
#define OFFER_CHUNK 1024 // keys looked at between two looks at the held count: want <= OFFER_BUF - OFFER_CHUNK
static_assert(OFFER_BUF - OFFER_CHUNK >= 1024, "k_offer_select holds k <= 1024 (irs_create: max_k) between two compactions");
static_assert(OFFER_TILE == IRS_OFFER_TILE, "irs_offer_layout pads the id array to the score kernel's tile");

typedef float offer_f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ the binding's launch
__global__ void __launch_bounds__(256) k_offer_prepare(const int64_t *__restrict__ src, int64_t n_ids, int64_t c_pad, int64_t n_item,
                                                       int64_t *__restrict__ ids, int32_t *__restrict__ holes) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= c_pad) return;
    long long out = -1ll;
    if (i < n_ids) {
        const long long id = (long long)src[i];
        const bool ok = id >= 0 && id < (long long)n_item && (i == 0 || id > (long long)src[i - 1]);
        if (ok) out = id;
        else atomicAdd(holes, 1);
    }
    ids[i] = (int64_t)out;
}

// ------------------------------------------------------------------ scores of a pass
// KS: k-steps of four (d rounded up to 32 / 64 / 128 / 256, zero-padded); RT: 16-row tiles per row group
template <int KS, int RT>
__global__ void __launch_bounds__(256) k_offer_scores(const float *__restrict__ x, int rows, int d, const float *__restrict__ W,
                                                      const float *__restrict__ bias, const int64_t *__restrict__ ids, int64_t c_pad,
                                                      float *__restrict__ sc) {
    constexpr int DK = KS * 4, LD = DK + 4; // DK is a multiple of 32: LD = 4 (mod 8) spreads a fragment read over all banks
    constexpr int XR = RT * 16;
    extern __shared__ __attribute__((aligned(16))) float offer_smem[];
    float *ws = offer_smem;          // [OFFER_TILE][LD]
    float *xs = ws + OFFER_TILE * LD; // [XR][LD]
    float *bs = xs + XR * LD;        // [OFFER_TILE]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int64_t tile0 = (int64_t)blockIdx.x * OFFER_TILE;
    const bool vec = (d & 3) == 0 && (((uintptr_t)W) & 15) == 0 && (((uintptr_t)x) & 15) == 0;
    // the tile's project rows, gathered by sanitised id; zeros for a hole and behind d
    if (vec) {
        for (int e = tid; e < OFFER_TILE * (DK / 4); e += 256) {
            const int i = e / (DK / 4), k4 = e % (DK / 4);
            const int64_t id = ids[tile0 + i];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (id >= 0 && 4 * k4 < d) v = *reinterpret_cast<const float4 *>(W + (size_t)id * d + 4 * k4);
            *reinterpret_cast<float4 *>(ws + i * LD + 4 * k4) = v;
        }
    } else {
        for (int e = tid; e < OFFER_TILE * DK; e += 256) {
            const int i = e / DK, k = e % DK;
            const int64_t id = ids[tile0 + i];
            ws[i * LD + k] = (id >= 0 && k < d) ? W[(size_t)id * d + k] : 0.f;
        }
    }
    if (tid < OFFER_TILE) {
        const int64_t id = ids[tile0 + tid];
        bs[tid] = id >= 0 ? bias[id] : 0.f;
    }
    __syncthreads();
    // this wave's 16 items as B fragments: lane (c, q) holds W[item c][k = 4 s + q]
    float bw[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) bw[s] = ws[(wave * 16 + c) * LD + 4 * s + q];
    const float b0 = bs[wave * 16 + c];
    for (int r0 = blockIdx.y * XR; r0 < rows; r0 += gridDim.y * XR) {
        __syncthreads(); // (the previous group's fragment reads are done)
        if (vec) {
            for (int e = tid; e < XR * (DK / 4); e += 256) {
                const int r = e / (DK / 4), k4 = e % (DK / 4);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r0 + r < rows && 4 * k4 < d) v = *reinterpret_cast<const float4 *>(x + (size_t)(r0 + r) * d + 4 * k4);
                *reinterpret_cast<float4 *>(xs + r * LD + 4 * k4) = v;
            }
        } else {
            for (int e = tid; e < XR * DK; e += 256) {
                const int r = e / DK, k = e % DK;
                xs[r * LD + k] = (r0 + r < rows && k < d) ? x[(size_t)(r0 + r) * d + k] : 0.f;
            }
        }
        __syncthreads();
        offer_f32x4 acc[RT];
#pragma unroll
        for (int u = 0; u < RT; ++u) acc[u] = offer_f32x4{b0, b0, b0, b0};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int u = 0; u < RT; ++u) // A: lane (c, q) holds x[row c of tile u][k = 4 s + q]; D: item c on the lane, rows 4 q + i
                acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[(u * 16 + c) * LD + 4 * s + q], bw[s], acc[u], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < RT; ++u) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = r0 + u * 16 + q * 4 + i;
                if (row < rows) sc[(size_t)row * c_pad + tile0 + wave * 16 + c] = acc[u][i];
            }
        }
    }
}

// ------------------------------------------------------------------ selection
// bitonic sort of n (a power of two) keys in LDS by the whole workgroup, largest first
__device__ __forceinline__ void offer_bitonic(unsigned long long *a, int n) {
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < n / 2; i += blockDim.x) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const bool first = (lo & size) == 0; // this pair keeps its larger value first
                const unsigned long long u = a[lo], v = a[hi];
                if ((u < v) == first) {
                    a[lo] = v;
                    a[hi] = u;
                }
            }
        }
    }
    __syncthreads();
}

// One workgroup per row of the pass.  The pattern is survivors.hip's surv_select with a buffer for k <= 1024: at most OFFER_CHUNK
// keys are appended between two looks at the held count, and the buffer is compacted to the best k as soon as more than
// OFFER_BUF - OFFER_CHUNK are held, so a slot stays below OFFER_BUF.  A key of 0 is "no key" (a hole).
__global__ void __launch_bounds__(256) k_offer_select(const float *__restrict__ sc, const int64_t *__restrict__ ids, int64_t C, int64_t c_pad,
                                                      const int32_t *__restrict__ holes, int k, float *__restrict__ val,
                                                      int64_t *__restrict__ ids0, int32_t *__restrict__ status) {
    __shared__ unsigned long long buf[OFFER_BUF];
    __shared__ unsigned int s_n;
    __shared__ unsigned long long s_thr;
    const int tid = threadIdx.x, row = blockIdx.x;
    const float *src = sc + (size_t)row * c_pad;
    const bool any_hole = holes[0] != 0; // (a set without holes: the id array is not read in the stream)
    if (tid == 0) {
        s_n = 0;
        s_thr = 0ull;
    }
    __syncthreads();
    for (int64_t base = 0; base < C; base += OFFER_CHUNK) {
        const unsigned long long thr = s_thr;
#pragma unroll
        for (int i = 0; i < OFFER_CHUNK / 256; ++i) {
            const int64_t j = base + i * 256 + tid;
            if (j < C) {
                const unsigned long long key = ((unsigned long long)irs_fkey(src[j]) << 32) | (0xFFFFFFFFu - (unsigned int)j);
                if (key > thr && !(any_hole && ids[j] < 0)) buf[atomicAdd(&s_n, 1u)] = key;
            }
        }
        __syncthreads();
        const unsigned int n = s_n;
        __syncthreads();
        if (n > OFFER_BUF - OFFER_CHUNK) {
            for (int i = n + tid; i < OFFER_BUF; i += 256) buf[i] = 0ull;
            offer_bitonic(buf, OFFER_BUF);
            if (tid == 0) {
                s_n = (n < (unsigned int)k) ? n : k;
                if (n >= (unsigned int)k) s_thr = buf[k - 1];
            }
            __syncthreads();
        }
    }
    unsigned int n = s_n;
    int n2 = 2; // the last sort: the held keys, up to a power of two (a small set costs a small sort)
    while (n2 < (int)n) n2 <<= 1;
    for (int i = n + tid; i < n2; i += 256) buf[i] = 0ull;
    offer_bitonic(buf, n2);
    if (n > (unsigned int)k) n = k;
    for (int i = tid; i < k; i += 256) {
        const unsigned long long kk = buf[i];
        const bool live = i < (int)n;
        val[(size_t)row * k + i] = live ? irs_unkey((unsigned int)(kk >> 32)) : -INFINITY;
        ids0[(size_t)row * k + i] = live ? ids[0xFFFFFFFFu - (unsigned int)kk] : (int64_t)-1;
    }
    if (tid == 0) status[row] = (int)n < k ? IRS_ROW_FEWER_THAN_K : 0;
}

// ------------------------------------------------------------------ host side
int irs_launch_offer_prepare(irs_ctx *ctx, const int64_t *ids0, int64_t n_ids, const irs_offer_rows &o, hipStream_t s) {
    IRS_CHECK_HIP(ctx, hipMemsetAsync(o.holes, 0, IRS_OFFER_HDR, s));
    hipLaunchKernelGGL(k_offer_prepare, dim3((unsigned int)((o.c_pad + 255) / 256)), dim3(256), 0, s, ids0, n_ids, o.c_pad, ctx->dims.n_item,
                       o.ids, o.holes);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

template <int KS, int RT>
static int offer_scores(irs_ctx *ctx, const float *x, int rows, const irs_offer_rows &o, hipStream_t s) {
    constexpr size_t lds = ((size_t)(OFFER_TILE + RT * 16) * (KS * 4 + 4) + OFFER_TILE) * sizeof(float);
    if (lds > 65536) {
        hipError_t attr = hipSuccess;
        IRS_ONCE_PER_DEVICE(attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_offer_scores<KS, RT>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        IRS_CHECK_HIP(ctx, attr);
    }
    const int64_t tiles = o.c_pad / OFFER_TILE;
    const int groups = (rows + RT * 16 - 1) / (RT * 16);
    // few tiles: the row groups are spread over up to OFFER_ROW_WGS workgroups as well (each gathers the tile again)
    int64_t ny = 2048 / tiles;
    ny = ny < 1 ? 1 : (ny > OFFER_ROW_WGS ? OFFER_ROW_WGS : ny);
    if (ny > groups) ny = groups;
    hipLaunchKernelGGL((k_offer_scores<KS, RT>), dim3((unsigned int)tiles, (unsigned int)ny), dim3(256), lds, s, x, rows, ctx->dims.d,
                       ctx->proj_w, ctx->proj_b, o.ids, o.c_pad, o.sc);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

int irs_launch_offer_scores(irs_ctx *ctx, const float *x, int rows, const irs_offer_rows &o, hipStream_t s) {
    const int d = ctx->dims.d;
    if (d <= 32) return offer_scores<8, 4>(ctx, x, rows, o, s);
    if (d <= 64) return offer_scores<16, 4>(ctx, x, rows, o, s);
    if (d <= 128) return offer_scores<32, 4>(ctx, x, rows, o, s);
    return offer_scores<64, 2>(ctx, x, rows, o, s);
}

int irs_launch_offer_topk(irs_ctx *ctx, const float *xrows, int M, int k, float *val, int64_t *ids0, int32_t *status, hipStream_t s) {
    const auto &b = ctx->opt.offer;
    irs_offer_rows o;
    irs_offer_layout(b.scratch, b.n, b.rows, &o);
    const int d = ctx->dims.d;
    for (int m0 = 0; m0 < M; m0 += b.rows) {
        const int rows = M - m0 < b.rows ? M - m0 : b.rows;
        const int rc = irs_launch_offer_scores(ctx, xrows + (size_t)m0 * d, rows, o, s);
        if (rc) return rc;
        hipLaunchKernelGGL(k_offer_select, dim3(rows), dim3(256), 0, s, o.sc, o.ids, b.n, o.c_pad, o.holes, k, val + (size_t)m0 * k,
                           ids0 + (size_t)m0 * k, status + m0);
        IRS_CHECK_HIP(ctx, hipGetLastError());
    }
    return IRS_OK;
}
