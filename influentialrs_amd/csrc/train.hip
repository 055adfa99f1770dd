// Native decoder trunk for training (include/irs_hip.h: irs_train_*): a forward that saves what the backward needs and a
// backward that produces every trunk parameter gradient, with the semantics of nn.TransformerDecoder in train mode as
// InfluentialNet._decoding_autograd / SampleNet._decoding_autograd call it (post-norm layers, additive IRN or causal mask plus
// key padding, cross-attention over the all-zero memory, dropout at every site torch applies it).
//
// Arithmetic: float32 operands, float32 accumulation, one rounding per product (k-ordered fma chains on the VALU: the same
// numerics as v_mfma_f32_*_f32); attention uses an online softmax and keeps the per-row log-sum-exp, the backward recomputes
// the probabilities.  No inference kernel is used or changed.
//
// Dropout masks: Philox4x32-10 keyed by the step's 64-bit seed, element e of (site, layer) is word (e & 3) of the block
// counter {lo32(e >> 2), hi32(e >> 2), layer, site}; it is kept iff (word >> 8) >= ceil(p * 2^24), and kept values are
// multiplied by 1 / (1 - p).  The forward and the backward regenerate the same masks.  The header lists the sites and their
// flat index layouts; tests/train_trunk_ref.py restates the generator in numpy.
//
// Determinism: no atomics.  Weight gradients are split-K partials summed in a fixed order, column sums are fixed row chunks
// summed in a fixed order, and every embedding row is summed by one thread over its positions in ascending order (a linear
// linking pass, k_emb_link, finds those positions).
#include "irs_internal.h"

namespace {

enum { DS_EMB = 0, DS_SELF = 1, DS_DROP1 = 2, DS_CROSS = 3, DS_DROP2 = 4, DS_FFN = 5, DS_DROP3 = 6 };

struct Drop {
    uint32_t k0, k1, thr;
    float scale;
    int on;
};

__device__ __forceinline__ uint32_t philox_word(uint32_t k0, uint32_t k1, uint64_t e, uint32_t layer, uint32_t site) {
    const uint64_t q = e >> 2;
    uint32_t c0 = (uint32_t)q, c1 = (uint32_t)(q >> 32), c2 = layer, c3 = site;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
    }
    const int s = (int)(e & 3);
    return s == 0 ? c0 : s == 1 ? c1 : s == 2 ? c2 : c3;
}

// multiplier of element e: 1 without dropout, else 0 or 1 / (1 - p)
__device__ __forceinline__ float drop_mul(const Drop &dp, uint64_t e, int layer, int site) {
    if (!dp.on) return 1.f;
    return (philox_word(dp.k0, dp.k1, e, (uint32_t)layer, (uint32_t)site) >> 8) >= dp.thr ? dp.scale : 0.f;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------ generic strided GEMM
// C(i, j) = sum_{k in chunk z} A(i, k) B(k, j),  A(i, k) = A[i sai + k sak],  B(k, j) = B[k sbk + j sbj]
// ep 0: C = acc (+ bias[j]) (+ add[i ldc + j]);  split-K chunks (gridDim.z > 1) write plain partials at C + z cz
// ep 1: v = max(acc + bias[j], 0); C = v; C2 = v * drop  (linear1 -> ReLU -> dropout; e = i Nc + j)
// ep 2: C = acc * drop * (aux[i ldc + j] > 0)              (backward of ep 1)
struct GemmArgs {
    const float *A;
    int64_t sai, sak;
    const float *B;
    int64_t sbk, sbj;
    float *C;
    int64_t ldc, cz;
    int Mr, Nc, K, kc;
    const float *bias, *add, *aux;
    float *C2;
    int ep, layer, site;
    Drop dp;
};

constexpr int GT = 64, GK = 16;

__global__ __launch_bounds__(256) void k_gemm(GemmArgs g) {
    __shared__ float As[GK][GT + 1], Bs[GK][GT + 1];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int i0 = blockIdx.x * GT, j0 = blockIdx.y * GT;
    const int kb = blockIdx.z * g.kc, ke = min(g.K, kb + g.kc);
    float acc[4][4] = {};
    for (int k0 = kb; k0 < ke; k0 += GK) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = t + 256 * q;
            int i, k;
            if (g.sak == 1) { i = idx >> 4; k = idx & 15; } else { k = idx >> 6; i = idx & 63; }
            const int gi = i0 + i, gk = k0 + k;
            As[k][i] = (gi < g.Mr && gk < ke) ? g.A[gi * g.sai + gk * g.sak] : 0.f;
            int j, kk;
            if (g.sbj == 1) { kk = idx >> 6; j = idx & 63; } else { j = idx >> 4; kk = idx & 15; }
            const int gj = j0 + j, gk2 = k0 + kk;
            Bs[kk][j] = (gj < g.Nc && gk2 < ke) ? g.B[gk2 * g.sbk + gj * g.sbj] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < GK; ++k) {
            float a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = As[k][ty + 16 * r];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = Bs[k][tx + 16 * c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = __fmaf_rn(a[r], b[c], acc[r][c]);
        }
        __syncthreads();
    }
    float *C = g.C + blockIdx.z * g.cz;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty + 16 * r;
        if (i >= g.Mr) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + tx + 16 * c;
            if (j >= g.Nc) continue;
            const int64_t o = (int64_t)i * g.ldc + j;
            float v = acc[r][c];
            if (g.ep == 0) {
                if (g.bias) v += g.bias[j];
                if (g.add) v += g.add[o];
                C[o] = v;
            } else if (g.ep == 1) {
                v = fmaxf(v + g.bias[j], 0.f);
                C[o] = v;
                g.C2[o] = v * drop_mul(g.dp, (uint64_t)i * g.Nc + j, g.layer, g.site);
            } else {
                C[o] = g.aux[o] > 0.f ? v * drop_mul(g.dp, (uint64_t)i * g.Nc + j, g.layer, g.site) : 0.f;
            }
        }
    }
}

// out[n] = sum_z part[z cz + n], z ascending
__global__ void k_sum_parts(const float *__restrict__ part, int nz, int64_t cz, int64_t n, float *__restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int z = 0; z < nz; ++z) s += part[z * cz + i];
    out[i] = s;
}

// column sums over fixed chunks of rows: p1[z][c] = sum_m A[m, c] W(m, c) (W(m, c) = w[m ldw + c / wdiv]; skipped when p1 is
// null), p2[z][c] = sum_m A[m, c] (skipped when p2 is null)
constexpr int CS_ROWS = 128;
__global__ void k_colsum_part(const float *__restrict__ A, int64_t lda, const float *__restrict__ w, int64_t ldw, int wdiv,
                              int M, int ncols, float *__restrict__ p1, float *__restrict__ p2) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.y;
    if (c >= ncols) return;
    const int m0 = z * CS_ROWS, m1 = min(M, m0 + CS_ROWS);
    float s1 = 0.f, s2 = 0.f;
    for (int m = m0; m < m1; ++m) {
        const float a = A[(int64_t)m * lda + c];
        if (p1) s1 = __fmaf_rn(a, w[(int64_t)m * ldw + c / wdiv], s1);
        s2 += a;
    }
    if (p1) p1[(int64_t)z * ncols + c] = s1;
    if (p2) p2[(int64_t)z * ncols + c] = s2;
}

// ------------------------------------------------------------------ embedding, layer norm, cross-attention constant
__global__ void k_emb_fwd(const int64_t *__restrict__ seq, const float *__restrict__ E, const float *__restrict__ pe,
                          float *__restrict__ x, int M, int L, int d, int64_t n_item, float sqrtd, Drop dp) {
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (idx >= (int64_t)M * d) return;
    const int m = (int)(idx / d), c = (int)(idx % d), i = m % L;
    int64_t tok = seq[m];
    tok = tok < 0 ? 0 : (tok > n_item ? n_item : tok);
    const float v = __fadd_rn(__fmul_rn(E[tok * d + c], sqrtd), pe[(int64_t)i * d + c]);
    x[idx] = v * drop_mul(dp, (uint64_t)idx, 0, DS_EMB);
}

// r = x + a * drop; y = LN(r) * g + b (one wave per row; d <= 256); st = {mean, rstd} per row
__global__ __launch_bounds__(256) void k_res_ln_fwd(const float *__restrict__ a, const float *__restrict__ x,
                                                     const float *__restrict__ g, const float *__restrict__ bt,
                                                     float *__restrict__ r, float *__restrict__ st, float *__restrict__ y,
                                                     int M, int d, Drop dp, int layer, int site) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= M) return;
    const int64_t o = (int64_t)m * d;
    float v[4], s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        v[k] = 0.f;
        if (c < d) {
            v[k] = x[o + c] + a[o + c] * drop_mul(dp, (uint64_t)(o + c), layer, site);
            r[o + c] = v[k];
            s += v[k];
        }
    }
    const float mean = wave_sum(s) / d;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (lane + 64 * k < d) q += (v[k] - mean) * (v[k] - mean);
    const float rstd = 1.f / sqrtf(wave_sum(q) / d + 1e-5f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c < d) y[o + c] = (v[k] - mean) * rstd * g[c] + bt[c];
    }
    if (lane == 0) {
        st[2 * (int64_t)m] = mean;
        st[2 * (int64_t)m + 1] = rstd;
    }
}

// backward of k_res_ln_fwd: xh = normalised r (for the gamma gradient), dres = dL/dr (the residual input's gradient),
// da = dL/da = dres * drop
__global__ __launch_bounds__(256) void k_ln_bwd(const float *__restrict__ dy, const float *__restrict__ r,
                                                 const float *__restrict__ st, const float *__restrict__ g,
                                                 float *__restrict__ xh, float *__restrict__ dres, float *__restrict__ da,
                                                 int M, int d, Drop dp, int layer, int site) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= M) return;
    const int64_t o = (int64_t)m * d;
    const float mean = st[2 * (int64_t)m], rstd = st[2 * (int64_t)m + 1];
    float xv[4], gx[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        xv[k] = gx[k] = 0.f;
        if (c < d) {
            xv[k] = (r[o + c] - mean) * rstd;
            gx[k] = dy[o + c] * g[c];
            xh[o + c] = xv[k];
            s1 += gx[k];
            s2 += gx[k] * xv[k];
        }
    }
    s1 = wave_sum(s1) / d;
    s2 = wave_sum(s2) / d;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c < d) {
            const float v = rstd * (gx[k] - s1 - xv[k] * s2);
            dres[o + c] = v;
            da[o + c] = v * drop_mul(dp, (uint64_t)(o + c), layer, site);
        }
    }
}

// cross-attention over the all-zero memory: uniform probabilities 1 / Lm, dropout on them, values all equal to bv:
// kap[m, h] = kept / (Lm (1 - p)), ca[m, h hd + e] = kap[m, h] bv[h hd + e]
__global__ void k_cross_fwd(const float *__restrict__ bv, float *__restrict__ kap, float *__restrict__ ca, int M, int L,
                            int H, int hd, int Lm, Drop dp, int layer) {
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (idx >= (int64_t)M * H) return;
    const int m = (int)(idx / H), h = (int)(idx % H), b = m / L, i = m % L;
    float k = 1.f;
    if (dp.on) {
        const uint64_t e0 = (((uint64_t)b * H + h) * L + i) * (uint64_t)Lm;
        int kept = 0;
        for (int j = 0; j < Lm; ++j) kept += drop_mul(dp, e0 + j, layer, DS_CROSS) != 0.f;
        k = (float)kept * dp.scale / (float)Lm;
    }
    kap[idx] = k;
    float *o = ca + (int64_t)m * H * hd + h * hd;
    for (int e = 0; e < hd; ++e) o[e] = k * bv[h * hd + e];
}

// ------------------------------------------------------------------ self-attention
// additive mask of (query i, key j) of sequence b before key padding: IRN = r_u on j <= i, -inf in the future, 1.0 on the last
// column; causal = 0 / -inf
__device__ __forceinline__ float mask_val(int mode, float ru, int i, int j, int L) {
    if (mode == IRS_MASK_IRN) return j == L - 1 ? 1.f : (j <= i ? ru : -INFINITY);
    return j <= i ? 0.f : -INFINITY;
}

struct AttnArgs {
    const float *qkv;   // [M, 3d]
    const int64_t *seq; // [B, L]
    const float *ru;    // [B]
    float *ao;          // [M, d]   forward out / backward in (o)
    float *lse;         // [B H L]
    const float *dao;   // [M, d]   backward in
    float *dqkv;        // [M, 3d]  backward out
    float *Dr;          // [B H L]  backward scratch: dO . o
    int L, H, hd, d, mode, layer;
    float scale;
    Drop dp;
};

// one thread per query row, 64 rows per workgroup, keys / values streamed through LDS in tiles of 64
template <int HDM>
__global__ __launch_bounds__(64) void k_attn_fwd(AttnArgs a) {
    __shared__ float Ks[64][HDM + 1], Vs[64][HDM + 1];
    __shared__ int padk[64];
    const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H, t = threadIdx.x, i = blockIdx.y * 64 + t;
    const int L = a.L, hd = a.hd, d3 = 3 * a.d;
    const bool act = i < L;
    const float ru = a.mode == IRS_MASK_IRN ? a.ru[b] : 0.f;
    float q[HDM], acc[HDM];
    const float *qr = a.qkv + ((int64_t)b * L + (act ? i : 0)) * d3 + h * hd;
#pragma unroll
    for (int e = 0; e < HDM; ++e) {
        q[e] = e < hd ? qr[e] : 0.f;
        acc[e] = 0.f;
    }
    float mx = -INFINITY, l = 0.f;
    const uint64_t erow = (((uint64_t)b * a.H + h) * L + i) * (uint64_t)L;
    for (int j0 = 0; j0 < L; j0 += 64) {
        __syncthreads();
        const int jl = j0 + t;
        if (jl < L) {
            const float *kr = a.qkv + ((int64_t)b * L + jl) * d3 + a.d + h * hd;
#pragma unroll
            for (int e = 0; e < HDM; ++e) {
                Ks[t][e] = e < hd ? kr[e] : 0.f;
                Vs[t][e] = e < hd ? kr[a.d + e] : 0.f;
            }
            padk[t] = a.seq[(int64_t)b * L + jl] == 0;
        }
        __syncthreads();
        if (!act) continue;
        const int nj = min(64, L - j0);
        for (int jj = 0; jj < nj; ++jj) {
            const int j = j0 + jj;
            const float mk = mask_val(a.mode, ru, i, j, L);
            if (padk[jj] || mk == -INFINITY) continue;
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < HDM; ++e) s = __fmaf_rn(q[e], Ks[jj][e], s);
            s = s * a.scale + mk;
            if (s > mx) {
                const float c = expf(mx - s);
                l *= c;
#pragma unroll
                for (int e = 0; e < HDM; ++e) acc[e] *= c;
                mx = s;
            }
            const float pe = expf(s - mx);
            l += pe;
            const float pz = pe * drop_mul(a.dp, erow + j, a.layer, DS_SELF);
#pragma unroll
            for (int e = 0; e < HDM; ++e) acc[e] = __fmaf_rn(pz, Vs[jj][e], acc[e]);
        }
    }
    if (!act) return;
    float *o = a.ao + ((int64_t)b * L + i) * a.d + h * hd;
    const float inv = 1.f / l;
#pragma unroll
    for (int e = 0; e < HDM; ++e)
        if (e < hd) o[e] = acc[e] * inv;
    a.lse[((int64_t)b * a.H + h) * L + i] = mx + logf(l);
}

// dQ: one thread per query row; D_i = dO_i . o_i is kept for the dK / dV pass
template <int HDM>
__global__ __launch_bounds__(64) void k_attn_bwd_q(AttnArgs a) {
    __shared__ float Ks[64][HDM + 1], Vs[64][HDM + 1];
    __shared__ int padk[64];
    const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H, t = threadIdx.x, i = blockIdx.y * 64 + t;
    const int L = a.L, hd = a.hd, d3 = 3 * a.d;
    const bool act = i < L;
    const float ru = a.mode == IRS_MASK_IRN ? a.ru[b] : 0.f;
    const int64_t row = (int64_t)b * L + (act ? i : 0);
    float q[HDM], g[HDM], dq[HDM], D = 0.f;
#pragma unroll
    for (int e = 0; e < HDM; ++e) {
        q[e] = e < hd ? a.qkv[row * d3 + h * hd + e] : 0.f;
        g[e] = e < hd ? a.dao[row * a.d + h * hd + e] : 0.f;
        D = __fmaf_rn(g[e], e < hd ? a.ao[row * a.d + h * hd + e] : 0.f, D);
        dq[e] = 0.f;
    }
    const int64_t r = ((int64_t)b * a.H + h) * L + (act ? i : 0);
    const float lse = a.lse[r];
    const uint64_t erow = (((uint64_t)b * a.H + h) * L + i) * (uint64_t)L;
    for (int j0 = 0; j0 < L; j0 += 64) {
        __syncthreads();
        const int jl = j0 + t;
        if (jl < L) {
            const float *kr = a.qkv + ((int64_t)b * L + jl) * d3 + a.d + h * hd;
#pragma unroll
            for (int e = 0; e < HDM; ++e) {
                Ks[t][e] = e < hd ? kr[e] : 0.f;
                Vs[t][e] = e < hd ? kr[a.d + e] : 0.f;
            }
            padk[t] = a.seq[(int64_t)b * L + jl] == 0;
        }
        __syncthreads();
        if (!act) continue;
        const int nj = min(64, L - j0);
        for (int jj = 0; jj < nj; ++jj) {
            const int j = j0 + jj;
            const float mk = mask_val(a.mode, ru, i, j, L);
            if (padk[jj] || mk == -INFINITY) continue;
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int e = 0; e < HDM; ++e) {
                s = __fmaf_rn(q[e], Ks[jj][e], s);
                dp = __fmaf_rn(g[e], Vs[jj][e], dp);
            }
            const float p = expf(s * a.scale + mk - lse);
            const float ds = p * (dp * drop_mul(a.dp, erow + j, a.layer, DS_SELF) - D);
#pragma unroll
            for (int e = 0; e < HDM; ++e) dq[e] = __fmaf_rn(ds, Ks[jj][e], dq[e]);
        }
    }
    if (!act) return;
    a.Dr[r] = D;
    float *o = a.dqkv + row * d3 + h * hd;
#pragma unroll
    for (int e = 0; e < HDM; ++e)
        if (e < hd) o[e] = dq[e] * a.scale;
}

// dK, dV: one thread per key row, query rows (q, dO, lse, D) streamed through LDS in tiles of 64; runs after k_attn_bwd_q
template <int HDM>
__global__ __launch_bounds__(64) void k_attn_bwd_kv(AttnArgs a) {
    __shared__ float Qs[64][HDM + 1], Gs[64][HDM + 1];
    __shared__ float Ls[64], Ds[64];
    const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H, t = threadIdx.x, j = blockIdx.y * 64 + t;
    const int L = a.L, hd = a.hd, d3 = 3 * a.d;
    const bool act = j < L;
    const float ru = a.mode == IRS_MASK_IRN ? a.ru[b] : 0.f;
    const int64_t row = (int64_t)b * L + (act ? j : 0);
    const bool padded = a.seq[row] == 0;
    float k[HDM], v[HDM], dk[HDM], dv[HDM];
#pragma unroll
    for (int e = 0; e < HDM; ++e) {
        k[e] = e < hd ? a.qkv[row * d3 + a.d + h * hd + e] : 0.f;
        v[e] = e < hd ? a.qkv[row * d3 + 2 * a.d + h * hd + e] : 0.f;
        dk[e] = dv[e] = 0.f;
    }
    const int64_t r0 = ((int64_t)b * a.H + h) * L;
    for (int i0 = 0; i0 < L; i0 += 64) {
        __syncthreads();
        const int il = i0 + t;
        if (il < L) {
            const int64_t qr = (int64_t)b * L + il;
#pragma unroll
            for (int e = 0; e < HDM; ++e) {
                Qs[t][e] = e < hd ? a.qkv[qr * d3 + h * hd + e] : 0.f;
                Gs[t][e] = e < hd ? a.dao[qr * a.d + h * hd + e] : 0.f;
            }
            Ls[t] = a.lse[r0 + il];
            Ds[t] = a.Dr[r0 + il];
        }
        __syncthreads();
        if (!act || padded) continue;
        const int ni = min(64, L - i0);
        for (int ii = 0; ii < ni; ++ii) {
            const int i = i0 + ii;
            const float mk = mask_val(a.mode, ru, i, j, L);
            if (mk == -INFINITY) continue;
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int e = 0; e < HDM; ++e) {
                s = __fmaf_rn(Qs[ii][e], k[e], s);
                dp = __fmaf_rn(Gs[ii][e], v[e], dp);
            }
            const float p = expf(s * a.scale + mk - Ls[ii]);
            const float z = drop_mul(a.dp, (uint64_t)(r0 + i) * L + j, a.layer, DS_SELF);
            const float pz = p * z, ds = p * (dp * z - Ds[ii]);
#pragma unroll
            for (int e = 0; e < HDM; ++e) {
                dv[e] = __fmaf_rn(pz, Gs[ii][e], dv[e]);
                dk[e] = __fmaf_rn(ds, Qs[ii][e], dk[e]);
            }
        }
    }
    if (!act) return;
    float *o = a.dqkv + row * d3 + a.d + h * hd;
#pragma unroll
    for (int e = 0; e < HDM; ++e)
        if (e < hd) {
            o[e] = dk[e] * a.scale;
            o[a.d + e] = dv[e];
        }
}

// ------------------------------------------------------------------ embedding gradient
// Deterministic and linear in the number of tokens M.  k_emb_link (ONE workgroup) walks the positions in ascending order, 256
// at a time, and links every position to the next position holding the same token: nxt[m] (-1 = last), first[m] = 1 for the
// first position of a token (pads and later positions 0).  last[] ([n_item + 1], -1 on entry) holds each token's latest
// position so far.  Per chunk every lane compares its token with the chunk's 256 (O(M) compares per lane in all).
// k_emb_sum: one workgroup per first position sums its token's rows along the chain, i.e. in ascending position order.
__device__ __forceinline__ int64_t clamp_tok(int64_t u, int64_t n_item) { return u < 0 ? 0 : (u > n_item ? n_item : u); }

__global__ __launch_bounds__(256) void k_emb_link(const int64_t *__restrict__ seq, int M, int64_t n_item,
                                                   int32_t *__restrict__ last, int32_t *__restrict__ nxt,
                                                   int32_t *__restrict__ first) {
    __shared__ int64_t tk[256];
    const int t = threadIdx.x;
    for (int c0 = 0; c0 < M; c0 += 256) {
        const int m = c0 + t, n = min(256, M - c0);
        const int64_t tok = m < M ? clamp_tok(seq[m], n_item) : 0;
        tk[t] = tok;
        if (m < M) nxt[m] = -1;
        __syncthreads();
        int prev_in = -1, later = 0;
        if (m < M && tok != 0) {
            for (int k = 0; k < n; ++k) {
                const bool eq = tk[k] == tok;
                if (k < t && eq) prev_in = k;
                if (k > t && eq) later = 1;
            }
        }
        const int prev = prev_in >= 0 ? c0 + prev_in : (m < M && tok != 0 ? last[tok] : -1);
        __syncthreads(); // every read of last[] for this chunk is done
        if (m < M) {
            first[m] = tok != 0 && prev < 0;
            if (tok != 0 && prev >= 0) nxt[prev] = m;
            if (tok != 0 && !later) last[tok] = m; // the chunk's last position of tok: one writer per token
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_emb_sum(const int64_t *__restrict__ seq, const int32_t *__restrict__ nxt,
                                                  const int32_t *__restrict__ first, const float *__restrict__ G,
                                                  float *__restrict__ dE, int d, int64_t n_item, float sqrtd, Drop dp) {
    const int m = blockIdx.x, t = threadIdx.x;
    if (!first[m] || t >= d) return;
    float acc = 0.f;
    for (int q = m; q >= 0; q = nxt[q]) {
        const int64_t o = (int64_t)q * d + t;
        acc = __fmaf_rn(G[o] * drop_mul(dp, (uint64_t)o, 0, DS_EMB), sqrtd, acc);
    }
    dE[clamp_tok(seq[m], n_item) * d + t] = acc;
}

} // namespace

// ------------------------------------------------------------------ host side
namespace {

inline size_t al(size_t v) { return (v + 63) / 64 * 64; } // floats -> 256-byte multiple

struct TrainPlan {
    // floats from the start of the saved arena
    size_t ru;
    size_t xin[IRS_MAX_LAYERS], qkv[IRS_MAX_LAYERS], lse[IRS_MAX_LAYERS], ao[IRS_MAX_LAYERS], r1[IRS_MAX_LAYERS],
        st1[IRS_MAX_LAYERS], y1[IRS_MAX_LAYERS], kap[IRS_MAX_LAYERS], ca[IRS_MAX_LAYERS], r2[IRS_MAX_LAYERS],
        st2[IRS_MAX_LAYERS], y2[IRS_MAX_LAYERS], hr[IRS_MAX_LAYERS], hdp[IRS_MAX_LAYERS], r3[IRS_MAX_LAYERS],
        st3[IRS_MAX_LAYERS];
    // scratch (forward temporaries, backward buffers)
    size_t T, TB, TC, G, G1, G2, XH, Dr, cs1, cs2, part, elast, enxt, efirst; // efirst .. : int32
    size_t total;
};

void splitk(int64_t N, int64_t K, int64_t M, int *S, int *kc) {
    const int64_t tiles = ((N + GT - 1) / GT) * ((K + GT - 1) / GT);
    int64_t s = 512 / tiles;
    s = s < 1 ? 1 : s;
    const int64_t smax = (M + 63) / 64;
    s = s > smax ? smax : s;
    int64_t c = (M + s - 1) / s;
    c = (c + GK - 1) / GK * GK;
    *kc = (int)c;
    *S = (int)((M + c - 1) / c);
}

TrainPlan plan_train(const irs_dims &D, int B, int L) {
    TrainPlan p{};
    const size_t M = (size_t)B * L, d = D.d, H = D.n_heads, F = D.ffn_dim;
    size_t o = 0;
    auto take = [&](size_t n) {
        size_t r = o;
        o += al(n);
        return r;
    };
    p.ru = take(B);
    for (int l = 0; l < D.n_layers; ++l) {
        p.xin[l] = take(M * d);
        p.qkv[l] = take(M * 3 * d);
        p.lse[l] = take((size_t)B * H * L);
        p.ao[l] = take(M * d);
        p.r1[l] = take(M * d);
        p.st1[l] = take(2 * M);
        p.y1[l] = take(M * d);
        p.kap[l] = take(M * H);
        p.ca[l] = take(M * d);
        p.r2[l] = take(M * d);
        p.st2[l] = take(2 * M);
        p.y2[l] = take(M * d);
        p.hr[l] = take(M * F);
        p.hdp[l] = take(M * F);
        p.r3[l] = take(M * d);
        p.st3[l] = take(2 * M);
    }
    p.T = take(M * d);
    p.TB = take(M * (F > d ? F : d));
    p.TC = take(M * 3 * d);
    p.G = take(M * d);
    p.G1 = take(M * d);
    p.G2 = take(M * d);
    p.XH = take(M * d);
    p.Dr = take((size_t)B * H * L);
    const size_t nz = (M + CS_ROWS - 1) / CS_ROWS, wc = 3 * d > F ? 3 * d : F;
    p.cs1 = take(nz * wc);
    p.cs2 = take(nz * wc);
    size_t pmax = 0;
    const int64_t shapes[4][2] = {{(int64_t)(3 * d), (int64_t)d}, {(int64_t)d, (int64_t)d}, {(int64_t)F, (int64_t)d}, {(int64_t)d, (int64_t)F}};
    for (auto &s : shapes) {
        int S, kc;
        splitk(s[0], s[1], (int64_t)M, &S, &kc);
        const size_t n = (size_t)S * s[0] * s[1];
        pmax = n > pmax ? n : pmax;
    }
    p.part = take(pmax);
    p.elast = take((size_t)D.n_item + 1);
    p.enxt = take(M);
    p.efirst = take(M);
    p.total = o;
    return p;
}

// gradient arena: the embedding, then per layer the 18 tensors in irs_bind_weight's order, each 256-byte aligned
const char *k_layer_names[18] = {"self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
                                 "self_attn.out_proj.bias", "multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias",
                                 "multihead_attn.out_proj.weight", "multihead_attn.out_proj.bias", "linear1.weight",
                                 "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias",
                                 "norm2.weight", "norm2.bias", "norm3.weight", "norm3.bias"};

size_t layer_numel(const irs_dims &D, int k) {
    const size_t d = D.d, F = D.ffn_dim;
    const size_t n[18] = {3 * d * d, 3 * d, d * d, d, 3 * d * d, 3 * d, d * d, d, F * d, F, d * F, d, d, d, d, d, d, d};
    return n[k];
}

size_t grad_off(const irs_dims &D, int layer, int k) { // layer -1: embedding
    size_t o = al((size_t)(D.n_item + 1) * D.d);
    if (layer < 0) return 0;
    for (int l = 0; l <= layer; ++l)
        for (int q = 0; q < 18; ++q) {
            if (l == layer && q == k) return o;
            o += al(layer_numel(D, q));
        }
    return o;
}

size_t grad_total(const irs_dims &D) { return grad_off(D, D.n_layers - 1, 17) + al(layer_numel(D, 17)); }

Drop make_drop(float p, uint64_t seed) {
    Drop r{};
    r.k0 = (uint32_t)seed;
    r.k1 = (uint32_t)(seed >> 32);
    r.on = p > 0.f;
    const double t = ceil((double)p * 16777216.0);
    r.thr = (uint32_t)t;
    r.scale = r.on ? 1.f / (1.f - p) : 1.f;
    return r;
}

struct Launcher {
    hipStream_t s;
    // Y[M, N] = X[M, K] W[N, K]^T + b (ep 0 / 1)
    void lin_fwd(const float *X, const float *W, const float *b, float *Y, int M, int N, int K, int ep = 0, float *Y2 = nullptr,
                 Drop dp = {}, int layer = 0, int site = 0) {
        GemmArgs g{};
        g.A = X; g.sai = K; g.sak = 1;
        g.B = W; g.sbk = 1; g.sbj = K;
        g.C = Y; g.ldc = N; g.Mr = M; g.Nc = N; g.K = K; g.kc = K;
        g.bias = b; g.ep = ep; g.C2 = Y2; g.dp = dp; g.layer = layer; g.site = site;
        launch(g, 1);
    }
    // dX[M, K] (= or +=) dY[M, N] W[N, K]  (ep 0: add = dX when accumulating; ep 2: dropout / ReLU backward against aux)
    void lin_dx(const float *dY, const float *W, float *dX, int M, int N, int K, const float *add, int ep = 0,
                const float *aux = nullptr, Drop dp = {}, int layer = 0, int site = 0) {
        GemmArgs g{};
        g.A = dY; g.sai = N; g.sak = 1;
        g.B = W; g.sbk = K; g.sbj = 1;
        g.C = dX; g.ldc = K; g.Mr = M; g.Nc = K; g.K = N; g.kc = N;
        g.add = add; g.ep = ep; g.aux = aux; g.dp = dp; g.layer = layer; g.site = site;
        launch(g, 1);
    }
    // dW[N, K] = dY[M, N]^T X[M, K]: split-K partials over M, summed in order
    void lin_dw(const float *dY, const float *X, float *dW, int M, int N, int K, float *part) {
        int S, kc;
        splitk(N, K, M, &S, &kc);
        GemmArgs g{};
        g.A = dY; g.sai = 1; g.sak = N;
        g.B = X; g.sbk = K; g.sbj = 1;
        g.C = part; g.ldc = K; g.cz = (int64_t)N * K; g.Mr = N; g.Nc = K; g.K = M; g.kc = kc;
        launch(g, S);
        const int64_t n = (int64_t)N * K;
        hipLaunchKernelGGL(k_sum_parts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, S, n, n, dW);
    }
    void launch(const GemmArgs &g, int S) {
        dim3 grid((g.Mr + GT - 1) / GT, (g.Nc + GT - 1) / GT, S);
        hipLaunchKernelGGL(k_gemm, grid, dim3(256), 0, s, g);
    }
    // out1[c] = sum_m A[m, c] W(m, c) (out1 may be null), out2[c] = sum_m A[m, c] (out2 may be null)
    void colsum(const float *A, int64_t lda, const float *w, int64_t ldw, int wdiv, int M, int ncols, float *out1, float *out2,
                float *p1, float *p2) {
        const int nz = (M + CS_ROWS - 1) / CS_ROWS;
        hipLaunchKernelGGL(k_colsum_part, dim3((ncols + 255) / 256, nz), dim3(256), 0, s, A, lda, w, ldw, wdiv, M, ncols,
                           out1 ? p1 : nullptr, out2 ? p2 : nullptr);
        if (out1) hipLaunchKernelGGL(k_sum_parts, dim3((ncols + 255) / 256), dim3(256), 0, s, p1, nz, (int64_t)ncols, (int64_t)ncols, out1);
        if (out2) hipLaunchKernelGGL(k_sum_parts, dim3((ncols + 255) / 256), dim3(256), 0, s, p2, nz, (int64_t)ncols, (int64_t)ncols, out2);
    }
};

template <int HDM>
void attn_launch(int which, const AttnArgs &a, int B, hipStream_t s) {
    dim3 grid(B * a.H, (a.L + 63) / 64);
    if (which == 0) hipLaunchKernelGGL(k_attn_fwd<HDM>, grid, dim3(64), 0, s, a);
    else if (which == 1) hipLaunchKernelGGL(k_attn_bwd_q<HDM>, grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL(k_attn_bwd_kv<HDM>, grid, dim3(64), 0, s, a);
}

void attn(int which, const AttnArgs &a, int B, hipStream_t s) {
    if (a.hd <= 8) attn_launch<8>(which, a, B, s);
    else if (a.hd <= 16) attn_launch<16>(which, a, B, s);
    else if (a.hd <= 32) attn_launch<32>(which, a, B, s);
    else attn_launch<64>(which, a, B, s);
}

int check_train(irs_ctx *ctx, const char *fn, const int64_t *seq, const int64_t *user, int B, int L, float p, const void *saved,
                size_t saved_bytes) {
    if (!ctx) return IRS_E_INVALID;
    const irs_dims &D = ctx->dims;
    if (!seq || !saved) IRS_FAIL(ctx, IRS_E_INVALID, "%s: null buffer", fn);
    if (B < 1) IRS_FAIL(ctx, IRS_E_INVALID, "%s: B=%d must be >= 1", fn, B);
    if (L < 1 || L > D.max_len) IRS_FAIL(ctx, IRS_E_INVALID, "%s: L=%d outside [1, max_len=%d]", fn, L, D.max_len);
    if ((int64_t)B * L > IRS_TRAIN_MAX_TOKENS) IRS_FAIL(ctx, IRS_E_INVALID, "%s: B*L=%lld tokens exceeds %d", fn, (long long)B * L, IRS_TRAIN_MAX_TOKENS);
    if (!(p >= 0.f && p < 1.f)) IRS_FAIL(ctx, IRS_E_INVALID, "%s: dropout p=%g outside [0, 1)", fn, (double)p);
    if (D.mask_mode == IRS_MASK_IRN && !user) IRS_FAIL(ctx, IRS_E_INVALID, "%s: user is null (IRN mask)", fn);
    if (((uintptr_t)saved) & 255) IRS_FAIL(ctx, IRS_E_INVALID, "%s: saved state must be 256-byte aligned", fn);
    const size_t need = plan_train(D, B, L).total * sizeof(float);
    if (saved_bytes < need) IRS_FAIL(ctx, IRS_E_INVALID, "%s: saved state too small: %zu < %zu", fn, saved_bytes, need);
    if (!ctx->item_emb || !ctx->pe) IRS_FAIL(ctx, IRS_E_STATE, "%s: embedding / pe not bound", fn);
    if (D.mask_mode == IRS_MASK_IRN && (!ctx->user_emb || !ctx->um_w || !ctx->um_b))
        IRS_FAIL(ctx, IRS_E_STATE, "%s: user weights not bound", fn);
    for (int l = 0; l < D.n_layers; ++l) {
        const irs_layer_w &w = ctx->layer[l];
        const float *all[] = {w.sa_in_w, w.sa_in_b, w.sa_out_w, w.sa_out_b, w.ca_in_b, w.ca_out_w, w.ca_out_b, w.l1_w,
                              w.l1_b, w.l2_w, w.l2_b, w.n1_w, w.n1_b, w.n2_w, w.n2_b, w.n3_w, w.n3_b};
        for (auto q : all)
            if (!q) IRS_FAIL(ctx, IRS_E_STATE, "%s: decoder layer %d weights not bound", fn, l);
    }
    return IRS_OK;
}

} // namespace

extern "C" size_t irs_train_saved_bytes(const irs_ctx *ctx, int32_t B, int32_t L) {
    if (!ctx || B < 1 || L < 1 || L > ctx->dims.max_len || (int64_t)B * L > IRS_TRAIN_MAX_TOKENS) return 0;
    return plan_train(ctx->dims, B, L).total * sizeof(float);
}

extern "C" size_t irs_train_grad_bytes(const irs_ctx *ctx) { return ctx ? grad_total(ctx->dims) * sizeof(float) : 0; }

extern "C" int64_t irs_train_grad_offset(const irs_ctx *ctx, const char *name) {
    if (!ctx || !name) return -1;
    if (strncmp(name, "module.", 7) == 0) name += 7;
    const irs_dims &D = ctx->dims;
    if (!strcmp(name, "item_embedder.weight") || !strcmp(name, "word_embedder.weight")) return 0;
    if (strncmp(name, "decoder.layers.", 15)) return -1;
    char *end = nullptr;
    const long l = strtol(name + 15, &end, 10);
    if (l < 0 || l >= D.n_layers || !end || *end != '.') return -1;
    for (int q = 0; q < 18; ++q)
        if (!strcmp(end + 1, k_layer_names[q])) return (int64_t)grad_off(D, (int)l, q);
    return -1;
}

extern "C" int irs_train_forward(irs_ctx *ctx, const int64_t *seq, const int64_t *user, int32_t B, int32_t L, float p,
                                 uint64_t seed, void *saved, size_t saved_bytes, float *x_out, void *stream) {
    int rc = check_train(ctx, "irs_train_forward", seq, user, B, L, p, saved, saved_bytes);
    if (rc) return rc;
    if (!x_out) IRS_FAIL(ctx, IRS_E_INVALID, "irs_train_forward: x_out is null");
    const irs_dims &D = ctx->dims;
    const hipStream_t s = (hipStream_t)stream;
    const TrainPlan P = plan_train(D, B, L);
    float *S = (float *)saved;
    const int M = B * L, d = D.d, H = D.n_heads, hd = d / H, F = D.ffn_dim, nl = D.n_layers;
    const Drop dp = make_drop(p, seed);
    Launcher ln{s};
    if ((rc = irs_launch_pif(ctx, user, B, S + P.ru, s)) != IRS_OK) return rc;
    const int64_t nmd = (int64_t)M * d;
    hipLaunchKernelGGL(k_emb_fwd, dim3((unsigned)((nmd + 255) / 256)), dim3(256), 0, s, seq, ctx->item_emb, ctx->pe,
                       S + P.xin[0], M, L, d, (int64_t)D.n_item, sqrtf((float)d), dp);
    for (int l = 0; l < nl; ++l) {
        const irs_layer_w &w = ctx->layer[l];
        float *xin = S + P.xin[l], *y3 = l + 1 < nl ? S + P.xin[l + 1] : x_out;
        ln.lin_fwd(xin, w.sa_in_w, w.sa_in_b, S + P.qkv[l], M, 3 * d, d);
        AttnArgs a{};
        a.qkv = S + P.qkv[l]; a.seq = seq; a.ru = S + P.ru; a.ao = S + P.ao[l]; a.lse = S + P.lse[l];
        a.L = L; a.H = H; a.hd = hd; a.d = d; a.mode = D.mask_mode; a.layer = l; a.scale = 1.f / sqrtf((float)hd); a.dp = dp;
        attn(0, a, B, s);
        ln.lin_fwd(S + P.ao[l], w.sa_out_w, w.sa_out_b, S + P.T, M, d, d);
        hipLaunchKernelGGL(k_res_ln_fwd, dim3((M + 3) / 4), dim3(256), 0, s, S + P.T, xin, w.n1_w, w.n1_b, S + P.r1[l],
                           S + P.st1[l], S + P.y1[l], M, d, dp, l, (int)DS_DROP1);
        hipLaunchKernelGGL(k_cross_fwd, dim3((unsigned)(((int64_t)M * H + 255) / 256)), dim3(256), 0, s, w.ca_in_b + 2 * d,
                           S + P.kap[l], S + P.ca[l], M, L, H, hd, D.max_len, dp, l);
        ln.lin_fwd(S + P.ca[l], w.ca_out_w, w.ca_out_b, S + P.T, M, d, d);
        hipLaunchKernelGGL(k_res_ln_fwd, dim3((M + 3) / 4), dim3(256), 0, s, S + P.T, S + P.y1[l], w.n2_w, w.n2_b,
                           S + P.r2[l], S + P.st2[l], S + P.y2[l], M, d, dp, l, (int)DS_DROP2);
        ln.lin_fwd(S + P.y2[l], w.l1_w, w.l1_b, S + P.hr[l], M, F, d, 1, S + P.hdp[l], dp, l, DS_FFN);
        ln.lin_fwd(S + P.hdp[l], w.l2_w, w.l2_b, S + P.T, M, d, F);
        hipLaunchKernelGGL(k_res_ln_fwd, dim3((M + 3) / 4), dim3(256), 0, s, S + P.T, S + P.y2[l], w.n3_w, w.n3_b,
                           S + P.r3[l], S + P.st3[l], y3, M, d, dp, l, (int)DS_DROP3);
    }
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

extern "C" int irs_train_backward(irs_ctx *ctx, const int64_t *seq, const int64_t *user, int32_t B, int32_t L, float p,
                                  uint64_t seed, void *saved, size_t saved_bytes, const float *dx, float *grads,
                                  size_t grad_bytes, void *stream) {
    int rc = check_train(ctx, "irs_train_backward", seq, user, B, L, p, saved, saved_bytes);
    if (rc) return rc;
    const irs_dims &D = ctx->dims;
    if (!dx || !grads) IRS_FAIL(ctx, IRS_E_INVALID, "irs_train_backward: null buffer");
    if (((uintptr_t)grads) & 255) IRS_FAIL(ctx, IRS_E_INVALID, "irs_train_backward: grads must be 256-byte aligned");
    const size_t gneed = grad_total(D) * sizeof(float);
    if (grad_bytes < gneed) IRS_FAIL(ctx, IRS_E_INVALID, "irs_train_backward: grads too small: %zu < %zu", grad_bytes, gneed);
    const hipStream_t s = (hipStream_t)stream;
    const TrainPlan P = plan_train(D, B, L);
    float *S = (float *)saved;
    const int M = B * L, d = D.d, H = D.n_heads, hd = d / H, F = D.ffn_dim, nl = D.n_layers;
    const Drop dp = make_drop(p, seed);
    Launcher ln{s};
    float *G = S + P.G, *G1 = S + P.G1, *G2 = S + P.G2, *T = S + P.T, *TB = S + P.TB, *TC = S + P.TC, *XH = S + P.XH;
    float *p1 = S + P.cs1, *p2 = S + P.cs2, *part = S + P.part;
    IRS_CHECK_HIP(ctx, hipMemcpyAsync(G, dx, (size_t)M * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    // the whole arena, alignment gaps included, is defined on return: zero it (the dead cross-attention gradients, row 0 and
    // the embedding rows of absent items stay 0)
    IRS_CHECK_HIP(ctx, hipMemsetAsync(grads, 0, gneed, s));
    auto gp = [&](int l, int k) { return grads + grad_off(D, l, k); };
    for (int l = nl - 1; l >= 0; --l) {
        const irs_layer_w &w = ctx->layer[l];
        const float *xin = S + P.xin[l];
        // norm3 <- dropout3 <- linear2 <- dropout <- ReLU <- linear1
        hipLaunchKernelGGL(k_ln_bwd, dim3((M + 3) / 4), dim3(256), 0, s, G, S + P.r3[l], S + P.st3[l], w.n3_w, XH, G2, T, M, d,
                           dp, l, (int)DS_DROP3);
        ln.colsum(G, d, XH, d, 1, M, d, gp(l, 16), gp(l, 17), p1, p2);
        ln.colsum(T, d, nullptr, 0, 1, M, d, nullptr, gp(l, 11), p1, p2);
        ln.lin_dw(T, S + P.hdp[l], gp(l, 10), M, d, F, part);
        ln.lin_dx(T, w.l2_w, TB, M, d, F, nullptr, 2, S + P.hr[l], dp, l, DS_FFN);
        ln.colsum(TB, F, nullptr, 0, 1, M, F, nullptr, gp(l, 9), p1, p2);
        ln.lin_dw(TB, S + P.y2[l], gp(l, 8), M, F, d, part);
        ln.lin_dx(TB, w.l1_w, G2, M, F, d, G2);
        // norm2 <- dropout2 <- cross-attention out_proj <- kap * bv
        hipLaunchKernelGGL(k_ln_bwd, dim3((M + 3) / 4), dim3(256), 0, s, G2, S + P.r2[l], S + P.st2[l], w.n2_w, XH, G1, T, M,
                           d, dp, l, (int)DS_DROP2);
        ln.colsum(G2, d, XH, d, 1, M, d, gp(l, 14), gp(l, 15), p1, p2);
        ln.colsum(T, d, nullptr, 0, 1, M, d, nullptr, gp(l, 7), p1, p2);
        ln.lin_dw(T, S + P.ca[l], gp(l, 6), M, d, d, part);
        ln.lin_dx(T, w.ca_out_w, TB, M, d, d, nullptr);
        ln.colsum(TB, d, S + P.kap[l], H, hd, M, d, gp(l, 5) + 2 * d, nullptr, p1, p2);
        // norm1 <- dropout1 <- self-attention out_proj <- attention <- in_proj
        hipLaunchKernelGGL(k_ln_bwd, dim3((M + 3) / 4), dim3(256), 0, s, G1, S + P.r1[l], S + P.st1[l], w.n1_w, XH, G, T, M, d,
                           dp, l, (int)DS_DROP1);
        ln.colsum(G1, d, XH, d, 1, M, d, gp(l, 12), gp(l, 13), p1, p2);
        ln.colsum(T, d, nullptr, 0, 1, M, d, nullptr, gp(l, 3), p1, p2);
        ln.lin_dw(T, S + P.ao[l], gp(l, 2), M, d, d, part);
        ln.lin_dx(T, w.sa_out_w, TB, M, d, d, nullptr);
        AttnArgs a{};
        a.qkv = S + P.qkv[l]; a.seq = seq; a.ru = S + P.ru; a.ao = S + P.ao[l]; a.lse = S + P.lse[l]; a.dao = TB; a.dqkv = TC;
        a.Dr = S + P.Dr; a.L = L; a.H = H; a.hd = hd; a.d = d; a.mode = D.mask_mode; a.layer = l;
        a.scale = 1.f / sqrtf((float)hd); a.dp = dp;
        attn(1, a, B, s);
        attn(2, a, B, s);
        ln.colsum(TC, 3 * d, nullptr, 0, 1, M, 3 * d, nullptr, gp(l, 1), p1, p2);
        ln.lin_dw(TC, xin, gp(l, 0), M, 3 * d, d, part);
        ln.lin_dx(TC, w.sa_in_w, G, M, 3 * d, d, G);
    }
    int32_t *elast = (int32_t *)(S + P.elast), *enxt = (int32_t *)(S + P.enxt), *efirst = (int32_t *)(S + P.efirst);
    IRS_CHECK_HIP(ctx, hipMemsetAsync(elast, 0xFF, ((size_t)D.n_item + 1) * sizeof(int32_t), s)); // -1
    hipLaunchKernelGGL(k_emb_link, dim3(1), dim3(256), 0, s, seq, M, (int64_t)D.n_item, elast, enxt, efirst);
    hipLaunchKernelGGL(k_emb_sum, dim3(M), dim3(256), 0, s, seq, enxt, efirst, G, grads, d, (int64_t)D.n_item,
                       sqrtf((float)d), dp);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}
