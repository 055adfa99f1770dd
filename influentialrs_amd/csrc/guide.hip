// The Rec2Inf choice rule of the greedy path step (include/irs_hip.h: irs_bind_guide), gfx950.
//
// Replaces the per-user, per-step Python of the reference's get_path (main_baselines.py:93-121): among the recommender's
// best k_c items the user has not seen, offer the one whose feature vector lies nearest to the target's (utils.py:202-206,
// cal_fv_dist: Hamming distance on binary vectors, Euclidean on float vectors).  Here the ranked list, the admissibility test
// (window + bound exclusions + path), the record and the window update are the greedy step's; only the choice among the first
// k_c survivors is new.  Launched only while a guide is bound: irs_path_step_row and its kernels are untouched.
#include "irs_internal.h"

size_t irs_guide_scratch(int64_t n_item, int kind, int F) {
    if (kind != IRS_GUIDE_BINARY) return 0;
    const size_t words = (size_t)(F + 31) / 32;
    return ((size_t)(n_item + 1) * words * sizeof(uint32_t) + 255) / 256 * 256;
}

// uint8 [rows][F] (nonzero = 1) -> words [rows][ceil(F / 32)], feature f in bit f % 32 of word f / 32; the bits behind F are zero.
// One thread per word.
__global__ void __launch_bounds__(256) k_guide_pack_bits(const uint8_t *__restrict__ table, int64_t rows, int F, int words,
                                                         uint32_t *__restrict__ packed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * words) return;
    const int64_t r = i / words;
    const int f0 = (int)(i - r * words) * 32;
    const uint8_t *src = table + r * F;
    uint32_t w = 0;
    for (int b = 0; b < 32 && f0 + b < F; ++b) w |= (src[f0 + b] != 0 ? 1u : 0u) << b;
    packed[i] = w;
}

int irs_launch_guide_pack(irs_ctx *ctx, const uint8_t *table, int64_t rows, int F, uint32_t *packed, hipStream_t s) {
    const int words = (F + 31) / 32;
    const int64_t n = rows * words;
    hipLaunchKernelGGL(k_guide_pack_bits, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, table, rows, F, words, packed);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

// The order of two distances: does `d` replace the current best `best`?  Strictly smaller only, so that a tie stays with the
// better rank; a NaN never replaces anything, and anything that is not a NaN replaces a NaN (np.argsort puts NaN last).
__device__ __forceinline__ bool irs_guide_closer(float d, float best) { return d < best || (best != best && d == d); }
__device__ __forceinline__ bool irs_guide_closer(unsigned int d, unsigned int best) { return d < best; }

// Squared Euclidean distance of two table rows as ONE float32 chain: acc = fmaf(t_f - c_f, t_f - c_f, acc), f ascending, acc
// starting at 0.  The loads go 16 bytes at a time where the rows allow it; the chain is the same either way.
__device__ __forceinline__ float irs_guide_dist_float(const float *__restrict__ t, const float *__restrict__ c, int F) {
    float acc = 0.f;
    if ((F & 3) == 0 && ((((uintptr_t)t) | ((uintptr_t)c)) & 15) == 0) {
        const float4 *t4 = reinterpret_cast<const float4 *>(t), *c4 = reinterpret_cast<const float4 *>(c);
        for (int f = 0; f < (F >> 2); ++f) {
            const float4 a = t4[f], b = c4[f];
            float df = a.x - b.x;
            acc = __fmaf_rn(df, df, acc);
            df = a.y - b.y;
            acc = __fmaf_rn(df, df, acc);
            df = a.z - b.z;
            acc = __fmaf_rn(df, df, acc);
            df = a.w - b.w;
            acc = __fmaf_rn(df, df, acc);
        }
    } else {
        for (int f = 0; f < F; ++f) {
            const float df = t[f] - c[f];
            acc = __fmaf_rn(df, df, acc);
        }
    }
    return acc;
}

// One wave per row, four rows per workgroup, like k_path_step.  Survivor i of the row (rank order, i < k_c <= 32) lives in lane i:
// the lane keeps its item and walks its own table row against the target's.
// EXCL / SLOTS as in k_path_step; KIND: IRS_GUIDE_BINARY or IRS_GUIDE_FLOAT.
template <bool EXCL, int SLOTS, int KIND>
__global__ void __launch_bounds__(256) k_path_step_guided(const irs_path_args p_, const irs_guide g, int B,
                                                          const float *__restrict__ val, const int64_t *__restrict__ ids0, int k) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    const int L = p_.L, path_ld = p_.path_ld;
    const int step = p_.step_ptr ? p_.step_ptr[0] : p_.step_arg;
    if (p_.step_next && row == 0 && lane == 0) p_.step_next[0] = step + 1; // (the merged small-batch loop: see irs_path_step_row)
    int64_t *w = p_.seq + (size_t)row * L;
    const int he = p_.hep[row];
    irs_window<SLOTS> win;
    win.load(w, he, L, lane);
    // 1. the first min(k_c, available) survivors in rank order, 64 candidates per round, one per lane
    irs_excl_view ev = {};
    if constexpr (EXCL) ev = irs_excl_open(p_.ex, row, lane, step);
    const int want = g.k_c;
    int found = 0;
    int64_t mine = 0; // survivor `lane`, as an item
    bool more = true;
    for (int c0 = 0; c0 < k && found < want && more; c0 += 64) {
        const int cl = c0 + lane;
        const int64_t cid = cl < k ? ids0[(size_t)row * k + cl] : (int64_t)-1;
        unsigned long long listed = 0ull;
        if constexpr (EXCL) listed = __ballot(irs_excl_listed(ev.list, ev.n, cid));
        for (int c = 0; c < 64 && c0 + c < k && found < want; ++c) {
            const int64_t id0 = __shfl(cid, c, 64);
            if (id0 < 0) {
                more = false;
                break;
            }
            const int64_t item = id0 + 1;
            bool hit = false;
            if constexpr (EXCL) hit = (ev.pth == item);
            hit = win.holds(item, hit);
            if (!__any(hit) && !((listed >> c) & 1ull)) {
                if (lane == found) mine = item;
                ++found;
            }
        }
    }
    // 2. the choice: the first survivor without a target, else the nearest one (ties: the better rank)
    int64_t chosen = 0;
    if (found > 0) {
        const int64_t t = w[L - 1];
        int best = 0;
        if (t >= 1 && t < g.rows && found > 1) {
            const bool in_table = lane < found && mine >= 1 && mine < g.rows; // (an item outside the table is never read: farthest)
            if constexpr (KIND == IRS_GUIDE_BINARY) {
                unsigned int d = 0xFFFFFFFFu;
                if (in_table) {
                    const uint32_t *tab = (const uint32_t *)g.table;
                    const uint32_t *tr = tab + (size_t)t * g.words, *cr = tab + (size_t)mine * g.words;
                    d = 0;
                    for (int i = 0; i < g.words; ++i) d += __popc(tr[i] ^ cr[i]);
                }
                unsigned int bd = __shfl(d, 0, 64);
                for (int i = 1; i < found; ++i) {
                    const unsigned int di = __shfl(d, i, 64);
                    if (irs_guide_closer(di, bd)) bd = di, best = i;
                }
            } else {
                float d = __uint_as_float(0x7FC00000u);
                if (in_table) {
                    const float *tab = (const float *)g.table;
                    d = irs_guide_dist_float(tab + (size_t)t * g.F, tab + (size_t)mine * g.F, g.F);
                }
                float bd = __shfl(d, 0, 64);
                for (int i = 1; i < found; ++i) {
                    const float di = __shfl(d, i, 64);
                    if (irs_guide_closer(di, bd)) bd = di, best = i;
                }
            }
        }
        chosen = __shfl(mine, best, 64);
    } else if (lane == 0) {
        p_.status[row] |= IRS_ROW_NO_CANDIDATE;
    }
    // 3. record, then grow or shift the window: the greedy step's tail (irs_path_step_row), a second copy so that its
    //    instantiations stay what they are
    if (lane == 0 && step < path_ld) p_.paths[(size_t)row * path_ld + step] = (float)chosen;
    if (found == 0) return;
    if (he < L - 2) {
        if (lane == 0) {
            w[he + 1] = chosen;
            p_.hep[row] = he + 1;
        }
    } else {
        int64_t nv[SLOTS];
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int p = lane + 64 * i;
            nv[i] = (p + 1 <= L - 2) ? w[p + 1] : 0;
        }
        // (all loads of the wave are complete before the stores: slot p is read by one lane and written by another)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int p = lane + 64 * i;
            if (p < L - 2) w[p] = nv[i];
        }
        if (lane == 0) w[L - 2] = chosen;
    }
}

template <int KIND>
static auto guided_kernel(bool excl, bool slots_short) {
    constexpr int S4 = IRS_WIN_SLOTS_SHORT, S16 = IRS_WIN_SLOTS_LONG;
    return slots_short ? (excl ? k_path_step_guided<true, S4, KIND> : k_path_step_guided<false, S4, KIND>)
                       : (excl ? k_path_step_guided<true, S16, KIND> : k_path_step_guided<false, S16, KIND>);
}

int irs_launch_path_step_guided(irs_ctx *ctx, const irs_path_args &pa, int B, const float *val, const int64_t *ids0, int k,
                                hipStream_t s) {
    const bool s4 = irs_window_slots(ctx) == IRS_WIN_SLOTS_SHORT;
    const auto kern = ctx->opt.guide.g.kind == IRS_GUIDE_BINARY ? guided_kernel<IRS_GUIDE_BINARY>(pa.ex.on, s4)
                                                          : guided_kernel<IRS_GUIDE_FLOAT>(pa.ex.on, s4);
    hipLaunchKernelGGL(kern, dim3((B + 3) / 4), dim3(256), 0, s, pa, ctx->opt.guide.g, B, val, ids0, k);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}
