// Path replay (include/irs_hip.h, "path replay"): every step of saved paths as one batch of teacher-forced windows.
// k_replay_windows builds the window of a row (user b, after i forced items) from the start window and the path by the layout's
// closed form -- no row waits for another; k_replay_target takes k_trace_target's place in front of the trace sweep (a FULL
// window has no target slot, and the forced item's score rides along); k_replay_record forms the three values of a row.
#include "irs_internal.h"

// One wave per row, four rows per workgroup.  The lanes stride over the L slots: 8-byte loads and stores, coalesced on both
// sides (a slot's source is the start row or the path at the slot's own offset).  Every index is formed only after the row's
// user and step have been checked, so an invalid row reads its fallback window and nothing else.
__global__ void __launch_bounds__(256) k_replay_windows(const irs_replay_args a) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= a.R) return;
    const int L = a.L;
    const int b = a.row_user[r], i = a.row_step[r];
    const bool b_ok = b >= 0 && b < a.B;
    bool ok = b_ok && i >= 0 && i <= a.P;
    const int bs = b_ok ? b : 0; // whose start window an invalid row gets
    const int64_t *s0 = a.seq0 + (size_t)bs * L;
    const int64_t *path = a.paths + (size_t)bs * a.path_ld;
    int n0 = L, h0 = 0;
    if (a.layout == IRS_REPLAY_FULL) { // the first 0 of the start row: a ballot per 64 slots
        for (int c0 = 0; c0 < L; c0 += 64) {
            const unsigned long long z = __ballot(c0 + lane < L && s0[c0 + lane] == 0);
            if (z) {
                n0 = c0 + __ffsll((long long)z) - 1;
                break;
            }
        }
    } else {
        h0 = a.hep0[bs];
        if (h0 < 0 || h0 > L - 2) {
            ok = false;
            h0 = h0 < 0 ? 0 : L - 2;
        }
    }
    if (ok) { // path[b][0 .. i) inside the catalog (i <= P <= path_ld)
        bool bad = false;
        for (int q = lane; q < i; q += 64) {
            const int64_t v = path[q];
            bad |= v < 1 || v > a.n_item;
        }
        ok = !__any(bad);
    }
    if (a.layout == IRS_REPLAY_FULL && ok && n0 + i == 0) ok = false;
    int64_t *w = a.seq_out + (size_t)r * L;
    int hep;
    if (a.layout == IRS_REPLAY_FULL) {
        if (ok) {
            const long long n = (long long)n0 + i, s = n > L ? n - L : 0; // entry q of seq0[0 .. n0) ++ path[0 .. i), shifted by s
            for (int p = lane; p < L; p += 64) {
                const long long q = p + s;
                w[p] = q < n0 ? s0[q] : (q < n ? path[q - n0] : (int64_t)0);
            }
            hep = (int)(n < L ? n : L) - 1;
        } else {
            for (int p = lane; p < L; p += 64) w[p] = p < n0 ? s0[p] : (int64_t)((n0 == 0 && p == 0) ? 1 : 0);
            hep = (n0 > 0 ? n0 : 1) - 1;
        }
    } else {
        const int g = L - 2 - h0; // steps that still grow
        if (ok && i > g) {
            const long long s = (long long)i - g; // entry p + s of seq0[0 .. h0] ++ path[0 .. i); the target stays
            for (int p = lane; p < L; p += 64) {
                const long long q = p + s;
                w[p] = p == L - 1 ? s0[p] : (q <= h0 ? s0[q] : path[q - h0 - 1]);
            }
            hep = L - 2;
        } else {
            const int n = ok ? i : 0;
            for (int p = lane; p < L; p += 64) w[p] = (p > h0 && p <= h0 + n) ? path[p - h0 - 1] : s0[p];
            hep = h0 + n;
        }
    }
    if (lane == 0) {
        a.hep_out[r] = hep;
        a.status[r] = ok ? IRS_ROW_OK : IRS_ROW_NO_CANDIDATE;
        if (a.user_out && a.user) a.user_out[r] = a.user[bs];
        if (a.item_out) a.item_out[r] = (ok && i < a.P) ? path[i] : (int64_t)0;
        if (a.target_out) a.target_out[r] = ok ? (a.layout == IRS_REPLAY_FULL ? a.target[b] : s0[L - 1]) : (int64_t)0;
    }
}

int irs_launch_replay_windows(irs_ctx *ctx, const irs_replay_args &a, hipStream_t s) {
    hipLaunchKernelGGL(k_replay_windows, dim3((a.R + 3) / 4), dim3(256), 0, s, a);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

// k_trace_target for replay rows: the target comes from the row's own word, not from slot L-1, and lane 1 takes the forced
// item's chain beside lane 0's (both k_gather's arithmetic).  -inf: no target / no item inside the catalog.
__global__ void __launch_bounds__(64) k_replay_target(const float *__restrict__ x, int d, const float *__restrict__ W,
                                                      const float *__restrict__ bias, int64_t n_local, const int64_t *__restrict__ target,
                                                      const int64_t *__restrict__ item, float *__restrict__ tscore,
                                                      float *__restrict__ iscore, int64_t *__restrict__ refid,
                                                      unsigned long long *__restrict__ count) {
    __shared__ float xs[256];
    const int row = blockIdx.x;
    for (int i = threadIdx.x; i < d; i += 64) xs[i] = x[(size_t)row * d + i];
    __syncthreads();
    if (threadIdx.x < 2) {
        const int64_t j = (threadIdx.x == 0 ? target[row] : item[row]) - 1;
        const bool ok = j >= 0 && j < n_local;
        const float e = ok ? irs_chain(xs, W + (size_t)j * d, bias[j], d) : -INFINITY;
        if (threadIdx.x == 0) {
            tscore[row] = e;
            refid[row] = ok ? j : -1;
            count[row] = 0ull;
        } else {
            iscore[row] = e;
        }
    }
}

// the three values of a row, k_trace_record's expressions; an invalid row records zeros
__global__ void __launch_bounds__(256) k_replay_record(const float *__restrict__ mx, const float *__restrict__ sm,
                                                       const float *__restrict__ ts, const float *__restrict__ is,
                                                       const int32_t *__restrict__ rank, const int64_t *__restrict__ item,
                                                       int64_t n_local, const int32_t *__restrict__ status, int M,
                                                       float *__restrict__ lp_item, float *__restrict__ lp_target,
                                                       int32_t *__restrict__ rank_out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= M) return;
    float lpi = 0.f, lpt = 0.f;
    int rk = 0;
    if (status[r] == IRS_ROW_OK) {
        const double lse = (double)mx[r] + log((double)sm[r]);
        const int64_t c = item[r];
        rk = rank[r];
        if (c >= 1 && c <= n_local) lpi = (float)((double)is[r] - lse);
        if (rk) lpt = (float)((double)ts[r] - lse);
    }
    lp_item[r] = lpi;
    lp_target[r] = lpt;
    rank_out[r] = rk;
}

int irs_launch_replay_score(irs_ctx *ctx, const irs_replay_rows &sc, int M, const int32_t *status, float *lp_item, float *lp_target,
                            int32_t *rank, hipStream_t s) {
    hipLaunchKernelGGL(k_replay_target, dim3(M), dim3(64), 0, s, sc.x, ctx->dims.d, ctx->proj_w, ctx->proj_b, ctx->n_local, sc.target,
                       sc.item, sc.tr.ts, sc.iscore, sc.tr.refid, sc.tr.count);
    const int rc = irs_launch_trace_sweep(ctx, sc.x, sc.seq, sc.hep, M, sc.tr, sc.tr.mx, sc.tr.sm, sc.tr.ts, sc.tr.rank, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_replay_record, dim3((M + 255) / 256), dim3(256), 0, s, sc.tr.mx, sc.tr.sm, sc.tr.ts, sc.iscore, sc.tr.rank, sc.item,
                       ctx->n_local, status, M, lp_item, lp_target, rank);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}
