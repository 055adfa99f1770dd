// The slate of a row: the first n admissible entries of its ranked list (irs_recommend_take / irs_recommend, include/irs_hip.h).
// An entry is ADMISSIBLE when its item is not in the row's window seq[row, 0 .. hep[row]] and not in the bound user's exclusion
// list -- the path step's own test without a path.  The step kernels walk a list one candidate at a time (one __any each), which
// is written for at most IRS_MAX_SAMPLE_K survivors; a slate takes up to IRS_MAX_RECOMMEND of up to max_k entries, so here every
// lane owns one candidate of a 64-entry round:
//   the window is the register image of irs_window<SLOTS> (the ONE membership test), spilled once per wave into LDS: slot
//   lane + 64 i of the wave's image is register i of that lane, -1 beyond the window's last live slot.  A lane scans slots
//   [0, hep + 1) for its own item -- every lane reads the same address, which the LDS broadcasts -- so "some slot equals the item"
//   is what __any(win.holds(item)) answers for that item;
//   the exclusion list is searched per lane with irs_excl_listed, as in the step;
//   one ballot; the output slot is taken + the popcount of the ballot below the lane, so a round's stores are contiguous.
// Scanned, not sorted.  A round's scan is (hep + 1) / 2 broadcast reads of 16 bytes per lane; a list of k entries has ceil(k / 64)
// rounds, two at the k = 100 every front end uses.  A bitonic sort of the image by ONE wave (k_surv_strips sorts with four) is
// log2(S) (log2(S) + 1) / 2 stages of S / 128 compare-exchanges per lane, two reads and two writes each: 288 LDS accesses at
// S = 256 against 200 for two scans of a full 200-item window, 1760 at S = 1024 against 1000.  The sort would win from about four
// rounds over a long window on (k >= 256 with max_len 1024); that form is not built (counts only: profiles/recommend/README.md).
// LDS: the four waves' images, 8 KB (SLOTS = 4) or 32 KB (SLOTS = 16).  No scratch, no atomics.
#include "irs_internal.h"

struct irs_take_args {
    const int64_t *seq;  // [M][L] or null: no window
    const int32_t *hep;  // [M] (with seq)
    int M, L, k, n;
    const float *val;    // [M][k]
    const int64_t *ids0; // [M][k]
    const float *mx, *sm; // [M] or null (with out_lp)
    float *out_val;      // [M][n]
    int64_t *out_ids0;   // [M][n]
    float *out_lp;       // [M][n] or null
    int32_t *out_count;  // [M]
    irs_excl ex;         // bound exclusions (zero: none; never a path)
};

template <bool EXCL, int SLOTS>
__global__ void __launch_bounds__(256) k_recommend_take(const irs_take_args a) {
    __shared__ __attribute__((aligned(16))) long long s_win[4][64 * SLOTS]; // (read two slots, 16 bytes, at a time)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    const bool live = row < a.M;
    long long *img = s_win[wave];
    int wl = 0; // slots [0, wl) can hold a window item
    {
        irs_window<SLOTS> win;
        int he = -1;
        if (live && a.seq) he = a.hep[row];
        if (he >= 0) {
            win.load(a.seq + (size_t)row * a.L, he, a.L, lane);
            wl = he < a.L ? he + 1 : a.L;
        } else {
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) win.v[i] = (int64_t)-1;
        }
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) img[lane + 64 * i] = (long long)win.v[i];
    }
    __syncthreads();
    if (!live) return;
    const int k = a.k, n = a.n;
    const double lse = a.out_lp ? (double)a.mx[row] + log((double)a.sm[row]) : 0.0;
    irs_excl_view ev = {};
    if constexpr (EXCL) ev = irs_excl_open(a.ex, row, lane, 0);
    const float *val = a.val + (size_t)row * k;
    const int64_t *ids0 = a.ids0 + (size_t)row * k;
    int taken = 0;
    for (int c0 = 0; c0 < k && taken < n; c0 += 64) {
        const int c = c0 + lane;
        const long long cid = c < k ? (long long)ids0[c] : -1ll;
        const unsigned long long neg = __ballot(cid < 0); // (a lane beyond k ends the list as a negative id does)
        const bool valid = neg ? lane < __ffsll((long long)neg) - 1 : true;
        const long long item = cid + 1;
        bool hit = false;
        for (int p = 0; p < wl; p += 2) { // (wl <= 64 SLOTS, which is even: slot p + 1 exists, and holds -1 beyond the window)
            const longlong2 w2 = *reinterpret_cast<const longlong2 *>(img + p);
            hit |= (w2.x == item) | (w2.y == item);
        }
        if constexpr (EXCL) hit |= irs_excl_listed(ev.list, ev.n, (int64_t)cid);
        const bool adm = valid && !hit;
        const unsigned long long got = __ballot(adm);
        const int slot = taken + __popcll(got & ((1ull << lane) - 1ull));
        if (adm && slot < n) {
            const float v = val[c];
            a.out_val[(size_t)row * n + slot] = v;
            a.out_ids0[(size_t)row * n + slot] = (int64_t)cid;
            if (a.out_lp) a.out_lp[(size_t)row * n + slot] = (float)((double)v - lse);
        }
        taken += __popcll(got);
        if (neg) break;
    }
    if (taken > n) taken = n;
    for (int i = taken + lane; i < n; i += 64) {
        a.out_val[(size_t)row * n + i] = -INFINITY;
        a.out_ids0[(size_t)row * n + i] = (int64_t)-1;
        if (a.out_lp) a.out_lp[(size_t)row * n + i] = -INFINITY;
    }
    if (lane == 0) a.out_count[row] = taken;
}

int irs_launch_recommend_take(irs_ctx *ctx, const int64_t *seq, const int32_t *hep, int M, const float *val, const int64_t *ids0, int k,
                              const float *mx, const float *sm, int n, float *out_val, int64_t *out_ids0, float *out_lp,
                              int32_t *out_count, const irs_excl &ex, hipStream_t s) {
    const irs_take_args a{seq, hep, M, ctx->dims.max_len, k, n, val, ids0, mx, sm, out_val, out_ids0, out_lp, out_count, ex};
    constexpr int S4 = IRS_WIN_SLOTS_SHORT, S16 = IRS_WIN_SLOTS_LONG;
    static_assert((64 * S4) % 2 == 0 && 4 * 64 * S16 * sizeof(long long) <= 32768, "the window images: two slots per read, 32 KB of LDS");
    const auto kern = irs_window_slots(ctx) == S4 ? (ex.on ? k_recommend_take<true, S4> : k_recommend_take<false, S4>)
                                                  : (ex.on ? k_recommend_take<true, S16> : k_recommend_take<false, S16>);
    hipLaunchKernelGGL(kern, dim3((M + 3) / 4), dim3(256), 0, s, a);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}
