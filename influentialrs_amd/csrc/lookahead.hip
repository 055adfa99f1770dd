// The one-step lookahead choice of the greedy search loops (include/irs_hip.h: irs_bind_lookahead), gfx950.
//
// Among a row's first k_c admissible candidates the loops offer the one under which the target's log-probability at the NEXT step
// is highest.  Two kernels frame the inner decode / log-sum-exp / gather that the loops already own: k_lookahead_expand writes
// the k_c child windows of a row (the parent window after irs_path_step would have chosen each candidate), k_lookahead_choose
// compares the children's target log-probabilities and rewrites the row's list to the chosen candidate alone, as
// irs_arrival_offer does, so that the unchanged path step and trace record carry the choice through.  The ranked list, the
// admissibility test (window + bound exclusions + path) and the window update are the greedy step's.
#include "irs_internal.h"

// One wave per row, four rows per workgroup, like k_path_step.  Survivor i of the row (rank order, i < k_c <= 32) lives in lane i.
// EXCL / SLOTS as in k_path_step.  No LDS, no atomics.
template <bool EXCL, int SLOTS>
__global__ void __launch_bounds__(256) k_lookahead_expand(const irs_look_expand_args a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= a.M) return;
    const int L = a.L, k = a.k, k_c = a.k_c;
    const int step = a.step_ptr ? a.step_ptr[0] : a.step_arg;
    const int64_t *w = a.seq + (size_t)row * L;
    const int he = a.hep[row];
    irs_window<SLOTS> win;
    win.load(w, he, L, lane);
    // 1. the first min(k_c, available) survivors in rank order, 64 candidates per round, one per lane (k_path_step_guided's walk)
    irs_excl_view ev = {};
    if constexpr (EXCL) ev = irs_excl_open(a.ex, row, lane, step);
    const bool live = !(a.fin && a.fin[row]);
    int found = 0;
    int64_t mine = 0; // survivor `lane`, as an item
    float mval = -INFINITY;
    bool more = live;
    for (int c0 = 0; c0 < k && found < k_c && more; c0 += 64) {
        const int cl = c0 + lane;
        const int64_t cid = cl < k ? a.ids0[(size_t)row * k + cl] : (int64_t)-1;
        const float cval = cl < k ? a.val[(size_t)row * k + cl] : -INFINITY;
        unsigned long long listed = 0ull;
        if constexpr (EXCL) listed = __ballot(irs_excl_listed(ev.list, ev.n, cid));
        for (int c = 0; c < 64 && c0 + c < k && found < k_c; ++c) {
            const int64_t id0 = __shfl(cid, c, 64);
            if (id0 < 0) {
                more = false;
                break;
            }
            const int64_t item = id0 + 1;
            bool hit = false;
            if constexpr (EXCL) hit = (ev.pth == item);
            hit = win.holds(item, hit);
            const float v = __shfl(cval, c, 64);
            if (!__any(hit) && !((listed >> c) & 1ull)) {
                if (lane == found) mine = item, mval = v;
                ++found;
            }
        }
    }
    // 2. the row's candidates and the children's scalars: child row * k_c + lane
    const size_t c_base = (size_t)row * k_c;
    if (lane < k_c) {
        const bool have = lane < found;
        a.c_ids0[c_base + lane] = have ? mine - 1 : (int64_t)-1;
        a.c_val[c_base + lane] = have ? mval : -INFINITY;
        a.c_hep[c_base + lane] = (have && he < L - 2) ? he + 1 : he;
        a.c_user[c_base + lane] = a.user ? a.user[row] : (int64_t)0;
        a.c_tgt0[c_base + lane] = w[L - 1] - 1;
    }
    // 3. the child windows: the parent's slots once into registers (slot p and slot p + 1 of lane + 64 i), then k_c windows of
    //    8-byte stores with the lanes along L
    int64_t cur[SLOTS], nxt[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        const int p = lane + 64 * i;
        cur[i] = p < L ? w[p] : 0;
        nxt[i] = p + 1 < L ? w[p + 1] : 0;
    }
    const bool grow = he < L - 2;
    for (int j = 0; j < k_c; ++j) {
        const int64_t item = __shfl(mine, j, 64);
        const bool have = j < found;
        int64_t *cw = a.c_seq + (c_base + j) * (size_t)L;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int p = lane + 64 * i;
            if (p >= L) continue;
            int64_t v = cur[i];
            if (have) {
                if (grow) {
                    if (p == he + 1) v = item;
                } else if (p < L - 2) { // shift left by one, keep the target last
                    v = nxt[i];
                } else if (p == L - 2) {
                    v = item;
                }
            }
            cw[p] = v;
        }
    }
}

int irs_launch_lookahead_expand(irs_ctx *ctx, const irs_look_expand_args &a, hipStream_t s) {
    constexpr int S4 = IRS_WIN_SLOTS_SHORT, S16 = IRS_WIN_SLOTS_LONG;
    const auto kern = irs_window_slots(ctx) == S4 ? (a.ex.on ? k_lookahead_expand<true, S4> : k_lookahead_expand<false, S4>)
                                                  : (a.ex.on ? k_lookahead_expand<true, S16> : k_lookahead_expand<false, S16>);
    hipLaunchKernelGGL(kern, dim3((a.M + 3) / 4), dim3(256), 0, s, a);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

// The order of two log-probabilities: does `v` replace the current best `best`?  Strictly greater only, so that a tie stays with
// the better rank; a NaN never replaces anything, and anything that is not a NaN replaces a NaN (irs_guide_closer, mirrored).
__device__ __forceinline__ bool irs_look_better(float v, float best) { return v > best || (best != best && v == v); }

// One wave per row, four rows per workgroup; candidate j of the row in lane j.  No LDS, no atomics.
__global__ void __launch_bounds__(256) k_lookahead_choose(const irs_look_choose_args a) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= a.M) return;
    const int k_c = a.k_c, k = a.k;
    const size_t c_base = (size_t)row * k_c;
    const int64_t t = a.seq[(size_t)row * a.L + a.L - 1];
    const bool live = !(a.fin && a.fin[row]);
    int64_t id0 = -1;
    float cv = -INFINITY, lp = -INFINITY;
    if (lane < k_c) {
        id0 = a.c_ids0[c_base + lane];
        cv = a.c_val[c_base + lane];
        // (the path trace's expression: k_trace_record)
        if (id0 >= 0) lp = (float)((double)a.ts[c_base + lane] - ((double)a.mx[c_base + lane] + log((double)a.sm[c_base + lane])));
    }
    const unsigned long long have = __ballot(id0 >= 0); // (the survivors fill the slots from 0)
    const int found = live ? __popcll(have) : 0;
    int best = -1;
    if (found > 0) {
        const unsigned long long is_t = __ballot(id0 >= 0 && id0 + 1 == t) & ((1ull << found) - 1ull);
        if (is_t) { // the target itself is offered: the arrival
            best = __ffsll((long long)is_t) - 1;
        } else {
            best = 0;
            float bv = __shfl(lp, 0, 64);
            for (int i = 1; i < found; ++i) {
                const float vi = __shfl(lp, i, 64);
                if (irs_look_better(vi, bv)) bv = vi, best = i;
            }
        }
    }
    if (lane < k_c) a.lp[c_base + lane] = lp;
    if (lane == 0) a.choice[row] = best;
    if (live && a.rec_item && lane < k_c) { // the record: the caller's row, this step's column
        const int step = a.rec_step[0];
        if (step < a.rec_ld) {
            const size_t at = ((size_t)(a.rec_map ? a.rec_map[row] : row) * a.rec_ld + step) * k_c + lane;
            a.rec_item[at] = id0 >= 0 ? (int32_t)(id0 + 1) : 0;
            a.rec_lp[at] = lp;
        }
    }
    if (best < 0) return;
    const int64_t bid = __shfl(id0, best, 64);
    const float bval = __shfl(cv, best, 64);
    if (lane == 0) {
        a.val[(size_t)row * k] = bval;
        a.ids0[(size_t)row * k] = bid;
    } else if (lane == 1 && k > 1) {
        a.val[(size_t)row * k + 1] = -INFINITY;
        a.ids0[(size_t)row * k + 1] = -1;
    }
}

int irs_launch_lookahead_choose(irs_ctx *ctx, const irs_look_choose_args &a, hipStream_t s) {
    hipLaunchKernelGGL(k_lookahead_choose, dim3((a.M + 3) / 4), dim3(256), 0, s, a);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}
