// Admissible rank: where the target stands among what a step may OFFER (include/irs_hip.h: "admissible rank";
// irs_score_target_rank_admissible, irs_bind_trace_admissible).  One kernel behind the trace sweep (score.hip:
// irs_launch_trace_sweep), which leaves per row the target's chain score `ts`, its 0-based id `refid` (-1: no target) and `count`,
// the items of the whole catalog that rank before it.  The sweep's count is corrected, exactly:
//   no offer set   rank_adm = 1 + count - #{distinct j in H, j != refid, before the target}
//   an offer set   rank_adm = 1 + #{j in U, j != refid, before the target} - #{distinct j in H and U, j != refid, before the target}
// H = the non-pad window items seq[row][0 .. hep], the user's bound exclusion list and the non-zero path entries [0, step);
// U = the sanitised ids of the bound offer set.  "Before" is the trace's order: score descending, id ascending, -0 == +0.
//
// One 256-thread workgroup per row.  The x row and the window lie in LDS (as in k_trace_rank: any max_len, no SLOTS form).  The
// DISTINCT union of H is compacted into LDS -- the list without adjacent repeats (k_excl_prepare sorts it, so repeats are
// adjacent), then the window items that are not in the list (irs_excl_listed) nor in an earlier slot, then the path items in
// neither nor in an earlier entry: at most 4096 + 1024 + 64 ids -- so that afterwards every lane scores: each member's score is
// irs_chain's, bit for bit what k_trace_rank compares for the window.  With an offer set the count over U reads the scores of the
// step's score pass (k_offer_scores: irs_chain's bits, offer_set.hip), and a union member counts when it is in the set.
// The order in which the union is compacted varies from run to run; nothing but its SIZE and its members' comparisons is used, and
// all sums are integers: two identical calls give identical bits.  No float atomics.
#include "irs_internal.h"

#define ADM_UNION (IRS_MAX_EXCL + IRS_MAX_LEN_LONG + IRS_MAX_PATH)

// (score, id) ranks before the target (rs, rid): the comparison of k_trace_rank
__device__ __forceinline__ bool adm_before(float e, int64_t j, float rs, int64_t rid) { return e > rs || (e == rs && j < rid); }

// every lane of a wave comes here together: the lanes with `keep` append v behind *n (one LDS atomic per wave)
__device__ __forceinline__ void adm_push(bool keep, int64_t v, int64_t *un, int *n, int lane) {
    const unsigned long long m = __ballot(keep);
    if (m == 0ull) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(n, __popcll(m));
    base = __shfl(base, 0, 64);
    if (keep) un[base + __popcll(m & ((1ull << lane) - 1ull))] = v;
}

__device__ __forceinline__ unsigned int adm_block_sum(unsigned int v, unsigned int *red, int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads(); // (the previous sum has been read)
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// EXCL: a list or a path is given (a.ex); OFFER: an offer set is bound (a.oids).  Neither: the window alone, k_trace_rank's value.
template <bool EXCL, bool OFFER>
__global__ void __launch_bounds__(256) k_trace_rank_adm(const irs_adm_args a, int d, const float *__restrict__ W,
                                                        const float *__restrict__ bias, int64_t n_local, int L) {
    __shared__ float xs[256];
    __shared__ int64_t wl[IRS_MAX_LEN_LONG];
    __shared__ int64_t un[ADM_UNION];
    __shared__ unsigned int red[4];
    __shared__ int s_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x;
    if (row >= a.M) return;
    const int64_t rid = a.refid[row];
    int32_t rank = 0;
    if (rid >= 0) { // (the whole workgroup takes the same side: the row's values)
        const float rs = a.ts[row];
        const float *x = a.xrows + (size_t)row * d;
        unsigned long long head = OFFER ? 0ull : a.count[row];
        if constexpr (OFFER) { // the items of the set before the target, from the score pass of this row
            const float *sc = a.osc + (size_t)row * a.oc_pad;
            unsigned int mine = 0;
            for (int64_t i = tid; i < a.on; i += 256) {
                const int64_t j = a.oids[i];
                if (j >= 0 && j != rid && adm_before(sc[i], j, rs, rid)) ++mine;
            }
            head = adm_block_sum(mine, red, tid);
        }
        rank = 1;
        if (head != 0ull) { // (nothing before the target: rank 1, and nothing is scored)
            for (int i = tid; i < d; i += 256) xs[i] = x[i];
            const int n = min(a.hep[row] + 1, L);
            for (int p = tid; p < n; p += 256) wl[p] = a.seq[(size_t)row * L + p];
            if (tid == 0) s_n = 0;
            __syncthreads();
            const int64_t *list = nullptr;
            int nl = 0;
            if constexpr (EXCL) {
                const irs_excl_view ev = irs_excl_open(a.ex, row, lane, a.ex.step_ptr ? a.ex.step_ptr[0] : a.ex.step_arg);
                list = ev.list, nl = ev.n;
                for (int i0 = wave * 64; i0 < nl; i0 += 256) { // the list: ascending, repeats adjacent
                    const int i = i0 + lane;
                    const int64_t j = i < nl ? list[i] : (int64_t)-1;
                    adm_push(i < nl && j != rid && j < n_local && (i == 0 || list[i - 1] != j), j, un, &s_n, lane);
                }
                if (wave == 0) { // the path so far: entry `lane` of the row, 1-based, -1 for none
                    const int64_t j = ev.pth - 1;
                    bool keep = ev.pth >= 1 && j < n_local && j != rid;
                    for (int q = 0; q < 64; ++q) {
                        const int64_t other = __shfl(ev.pth, q, 64);
                        keep &= !(q < lane && other == ev.pth);
                    }
                    bool in_win = false;
                    for (int q = 0; q < n; ++q) in_win |= (wl[q] == ev.pth);
                    keep = keep && !in_win && !irs_excl_listed(list, nl, j);
                    adm_push(keep, j, un, &s_n, lane);
                }
            }
            for (int p0 = wave * 64; p0 < n; p0 += 256) { // the window: a slot counts when no earlier slot holds its item
                const int p = p0 + lane;
                const int64_t item = p < n ? wl[p] : (int64_t)0, j = item - 1;
                bool keep = p < n && j >= 0 && j < n_local && j != rid;
                if (keep) {
                    bool dup = false;
                    for (int q = 0; q < p; ++q) dup |= (wl[q] == item);
                    keep = !dup;
                    if constexpr (EXCL) keep = keep && !irs_excl_listed(list, nl, j);
                }
                adm_push(keep, j, un, &s_n, lane);
            }
            __syncthreads();
            const int total = s_n;
            unsigned int sub = 0;
            const bool holes = OFFER && a.oholes[0] != 0;
            for (int i = tid; i < total; i += 256) {
                const int64_t j = un[i];
                unsigned int times = 1;
                if constexpr (OFFER) {
                    if (!holes) times = irs_excl_listed(a.oids, (int)a.on, j) ? 1u : 0u;
                    else { // a set with holes need not ascend: every entry is looked at, and an id counts as often as the set holds it
                        times = 0;
                        for (int64_t q = 0; q < a.on; ++q) times += (a.oids[q] == j) ? 1u : 0u;
                    }
                    if (times == 0) continue;
                }
                const float e = irs_chain(xs, W + (size_t)j * d, bias[j], d);
                if (adm_before(e, j, rs, rid)) sub += times;
            }
            sub = adm_block_sum(sub, red, tid);
            rank = (int32_t)(1ull + head - (unsigned long long)sub);
        }
    }
    if (tid == 0) {
        a.out[row] = rank;
        if (a.rec && !(a.rec_fin && a.rec_fin[row]))
            a.rec[(size_t)(a.rec_map ? a.rec_map[row] : row) * a.rec_ld + a.rec_step[0]] = rank;
    }
}

int irs_launch_trace_rank_adm(irs_ctx *ctx, const irs_adm_args &a, hipStream_t s) {
    const bool ex = a.ex.on != 0, of = a.oids != nullptr;
    const auto kern = of ? (ex ? k_trace_rank_adm<true, true> : k_trace_rank_adm<false, true>)
                         : (ex ? k_trace_rank_adm<true, false> : k_trace_rank_adm<false, false>);
    hipLaunchKernelGGL(kern, dim3(a.M), dim3(256), 0, s, a, ctx->dims.d, ctx->proj_w, ctx->proj_b, ctx->n_local, ctx->dims.max_len);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}
