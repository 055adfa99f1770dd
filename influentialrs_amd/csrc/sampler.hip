// The bound sampler's choice (irs_bind_sampler / irs_sampler_choose, include/irs_hip.h): between the ranking and the path step a
// live row draws one of its first top_k admissible candidates -- temperature, nucleus, a draw keyed by the caller's row and the
// step -- and its list is rewritten to that candidate alone, as k_arrival_offer and the lookahead's choose step rewrite it.  The
// unchanged step kernel, trace record and until loop do the rest.
//   WALK: k_recommend_take's.  The window is the register image of irs_window<SLOTS> (the ONE membership test) spilled per wave
//   into LDS; every lane owns one candidate of a 64-entry round and scans the image for it with broadcast reads; the exclusion
//   list is searched per lane with irs_excl_listed; under no_repeat the wave's path entries (irs_excl_open's, one per lane) are
//   spilled and scanned the same way.  One ballot per round; the output slot is taken + the popcount below the lane.  The first
//   n <= top_k <= 256 admissible candidates go to LDS as (value, position in the list), in list order: 2 KB per wave.
//   WEIGH: lane l owns candidates 4 l .. 4 l + 3 (weight 0 from n on).  w = expf((v - v_0) * inv_T); the lane's own prefix sums
//   serially, the lanes' totals by a Hillis-Steele scan over the wave (six shuffles): the order of the additions depends on
//   nothing but the index, so two calls give the same bits.  "The smallest m with S_m >= x" is a ballot per owned slot and the
//   first set bit.
//   DRAW: splitmix64 of (seed, caller's row, step), the stock sampled step's expression.
// No atomics, no host reads, nothing allocated.  A row writes entries 0 and 1 of its own list and its own record cells only.
#include "irs_internal.h"

#define SAMPLER_PER_LANE (IRS_MAX_SAMPLER_K / 64)

// this lane's x[idx & 3] of lane idx >> 2 (idx is the same in every lane)
__device__ __forceinline__ float sampler_pick(const float (&x)[SAMPLER_PER_LANE], int idx) {
    float t = x[0];
#pragma unroll
    for (int j = 1; j < SAMPLER_PER_LANE; ++j) t = (idx & (SAMPLER_PER_LANE - 1)) == j ? x[j] : t;
    return __shfl(t, idx / SAMPLER_PER_LANE, 64);
}

// the smallest index i < m with x_i >= bound (strict: x_i > bound), m if there is none; x_i is x[i & 3] of lane i >> 2.  The prefix
// sums of two lanes come from different addition trees and need not be monotone in the last bit, so this is a search for the
// first, not a count
__device__ __forceinline__ int sampler_first(const float (&x)[SAMPLER_PER_LANE], int base, int m, float bound, bool strict) {
    int first = m;
#pragma unroll
    for (int j = 0; j < SAMPLER_PER_LANE; ++j) {
        const unsigned long long hit = __ballot(base + j < m && (strict ? x[j] > bound : x[j] >= bound));
        const int i = hit ? (__ffsll((long long)hit) - 1) * SAMPLER_PER_LANE + j : m;
        first = i < first ? i : first;
    }
    return first;
}

template <bool EXCL, int SLOTS>
__global__ void __launch_bounds__(256) k_sampler_choose(const irs_sampler_args a) {
    __shared__ __attribute__((aligned(16))) long long s_win[4][64 * SLOTS]; // (read two slots, 16 bytes, at a time)
    __shared__ __attribute__((aligned(16))) long long s_pth[4][EXCL ? 64 : 2];
    __shared__ float s_v[4][IRS_MAX_SAMPLER_K];
    __shared__ int s_pos[4][IRS_MAX_SAMPLER_K];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    const int step = a.step_ptr ? a.step_ptr[0] : a.step_arg;
    const int k = a.k;
    bool live = row < a.M;
    if (live && a.fin && a.fin[row]) live = false; // a finished row of the until loop: nothing is written
    const int rid = live ? (a.row_ids ? a.row_ids[row] : row) : 0;
    const bool rec_ok = live && rid >= 0 && rid < a.rec_users && step >= 0 && step < a.rec_ld;
    const size_t rec_at = rec_ok ? (size_t)rid * a.rec_ld + step : 0;
    bool walk = live;
    if (live && (a.status[row] & IRS_ROW_OFFERED)) { // the arrival rule has chosen at this step: the list is the offer's
        const int64_t t0 = a.seq[(size_t)row * a.L + a.L - 1] - 1;
        if (a.ids0[(size_t)row * k] == t0 && (k == 1 || a.ids0[(size_t)row * k + 1] < 0)) walk = false;
    }
    long long *img = s_win[wave];
    int wl = 0, pl = 0, n = 0; // slots [0, wl) can hold a window item, [0, pl) a path entry; candidates kept
    if (walk) {
        irs_window<SLOTS> win;
        const int he = a.hep[row];
        win.load(a.seq + (size_t)row * a.L, he, a.L, lane);
        wl = he < 0 ? 0 : (he < a.L ? he + 1 : a.L);
        wl = (wl + 1) & ~1; // (two slots per read: slot wl of an odd window holds -1)
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) img[lane + 64 * i] = (long long)win.v[i];
    }
    irs_excl_view ev = {};
    if constexpr (EXCL) {
        if (walk) {
            ev = irs_excl_open(a.ex, row, lane, step);
            s_pth[wave][lane] = (long long)ev.pth;
            pl = step < 64 ? (step < 0 ? 0 : step) : 64;
            pl = (pl + 1) & ~1; // (entry pl of an odd path holds -1: lane >= step)
        }
    }
    __syncthreads();
    if (walk) {
        const float *val = a.val + (size_t)row * k;
        const int64_t *ids0 = a.ids0 + (size_t)row * k;
        const int top_k = a.top_k < IRS_MAX_SAMPLER_K ? a.top_k : IRS_MAX_SAMPLER_K;
        for (int c0 = 0; c0 < k && n < top_k; c0 += 64) {
            const int c = c0 + lane;
            const long long cid = c < k ? (long long)ids0[c] : -1ll;
            const unsigned long long neg = __ballot(cid < 0); // (a lane beyond k ends the list as a negative id does)
            const bool valid = neg ? lane < __ffsll((long long)neg) - 1 : true;
            const long long item = cid + 1;
            bool hit = false;
            for (int p = 0; p < wl; p += 2) {
                const longlong2 w2 = *reinterpret_cast<const longlong2 *>(img + p);
                hit |= (w2.x == item) | (w2.y == item);
            }
            if constexpr (EXCL) {
                for (int p = 0; p < pl; p += 2) {
                    const longlong2 p2 = *reinterpret_cast<const longlong2 *>(s_pth[wave] + p);
                    hit |= (p2.x == item) | (p2.y == item);
                }
                hit |= irs_excl_listed(ev.list, ev.n, (int64_t)cid);
            }
            const bool adm = valid && !hit;
            const unsigned long long got = __ballot(adm);
            const int slot = n + __popcll(got & ((1ull << lane) - 1ull));
            if (adm && slot < top_k) {
                s_v[wave][slot] = val[c];
                s_pos[wave][slot] = c;
            }
            n += __popcll(got);
            if (neg) break;
        }
        if (n > top_k) n = top_k;
    }
    __syncthreads();
    if (!live) return;
    if (!walk || n == 0) { // offered: (0, 0, 1); no admissible candidate: zeros, and the step reports it
        if (lane == 0 && rec_ok) {
            if (a.rec_u) a.rec_u[rec_at] = 0.f;
            if (a.rec_lq) a.rec_lq[rec_at] = 0.f;
            if (a.rec_support) a.rec_support[rec_at] = walk ? 0 : 1;
        }
        return;
    }
    // the draw: the stock sampled step's counter RNG, keyed by the caller's row
    unsigned long long z = a.seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)rid * 1315423911ull + (unsigned long long)step + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    const float u = (float)(z >> 40) * (1.0f / 16777216.0f);
    float v[SAMPLER_PER_LANE], w[SAMPLER_PER_LANE], P[SAMPLER_PER_LANE];
    const int base = lane * SAMPLER_PER_LANE;
#pragma unroll
    for (int j = 0; j < SAMPLER_PER_LANE; ++j) v[j] = base + j < n ? s_v[wave][base + j] : -INFINITY;
    const float v0 = __shfl(v[0], 0, 64);
    int chosen = 0, support = 1;
    float lq = 0.f;
    if (v0 - v0 == 0.f) { // v_0 is finite
        float run = 0.f;
#pragma unroll
        for (int j = 0; j < SAMPLER_PER_LANE; ++j) {
            w[j] = base + j < n ? expf((v[j] - v0) * a.inv_t) : 0.f; // (v = -inf: expf(-inf) = 0)
            run += w[j];
            P[j] = run; // the lane's own prefix sums
        }
        float incl = run; // inclusive scan of the lanes' totals
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        const float excl = __shfl_up(incl, 1, 64);
#pragma unroll
        for (int j = 0; j < SAMPLER_PER_LANE; ++j) P[j] = lane ? excl + P[j] : P[j]; // P[j] = S_(base + j + 1)
        const float s_n = sampler_pick(P, n - 1);
        const float thr = a.top_p * s_n;
        support = sampler_first(P, base, n, thr, false) + 1; // (S_n >= top_p * S_n: one exists)
        if (support > n) support = n;
        const float s_m = sampler_pick(P, support - 1);
        const float t = u * s_m;
        chosen = sampler_first(P, base, support, t, true);
        if (chosen > support - 1) chosen = support - 1;
        lq = logf(sampler_pick(w, chosen) / s_m);
    }
    const int pos = s_pos[wave][chosen];
    const float cv = sampler_pick(v, chosen);
    const int64_t cid = a.ids0[(size_t)row * k + pos]; // (every lane reads it before lanes 0 and 1 write entries 0 and 1)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_s_waitcnt(0);
    if (lane == 0) {
        a.val[(size_t)row * k] = cv;
        a.ids0[(size_t)row * k] = cid;
        if (rec_ok) {
            if (a.rec_u) a.rec_u[rec_at] = u;
            if (a.rec_lq) a.rec_lq[rec_at] = lq;
            if (a.rec_support) a.rec_support[rec_at] = support;
        }
    } else if (lane == 1 && k > 1) {
        a.val[(size_t)row * k + 1] = -INFINITY;
        a.ids0[(size_t)row * k + 1] = -1;
    }
}

int irs_launch_sampler_choose(irs_ctx *ctx, const irs_sampler_args &a, hipStream_t s) {
    constexpr int S4 = IRS_WIN_SLOTS_SHORT, S16 = IRS_WIN_SLOTS_LONG;
    static_assert(IRS_MAX_SAMPLER_K == 64 * SAMPLER_PER_LANE && (SAMPLER_PER_LANE & (SAMPLER_PER_LANE - 1)) == 0,
                  "a lane owns a power of two of the candidates");
    static_assert(4 * 64 * S16 * sizeof(long long) + 4 * 64 * 8 + 4 * IRS_MAX_SAMPLER_K * 8 <= 65536, "the LDS of a workgroup");
    const auto kern = irs_window_slots(ctx) == S4 ? (a.ex.on ? k_sampler_choose<true, S4> : k_sampler_choose<false, S4>)
                                                  : (a.ex.on ? k_sampler_choose<true, S16> : k_sampler_choose<false, S16>);
    hipLaunchKernelGGL(kern, dim3((a.M + 3) / 4), dim3(256), 0, s, a);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}
