// Beam trace (irs_bind_beam_trace, irs_beam_trace_carry), gfx950: the recorded columns of a beam follow the beam.
//
// A beam step reorders the beams of a user: output beam t is a child of input beam p, a whole copy of a finished input beam p, or
// dead.  The linked step (path.hip: k_beam_step<.., irs_beam_link>) says which, per output row, and hands over the list value of
// the candidate a child chose.  This kernel applies that to the caller's three [users][W][ld] arrays IN PLACE: every input row is
// read into LDS first, one barrier, then every output slot is written from LDS -- so that a slot may be the parent of any other.
// Column `step` of a child is formed here, from the trace sweep's float32 results on the PARENT's row (the step's input state)
// with k_trace_record's expression; the columns behind it are zeros, as the beam step writes its path.
// One workgroup per user, one wave per beam row at a time, lanes along the columns: row r of an LDS image starts at float
// r * 64, lane c reads and writes r * 64 + c -- 64 consecutive dwords, no two lanes of a 32-lane group on one bank.
// No atomics, no float reductions: identical calls give identical bits.
#include "irs_internal.h"

#define CARRY_MAXW 32
static_assert(IRS_MAX_PATH <= 64, "a wave holds a row's columns, one per lane");

__global__ void __launch_bounds__(512) k_beam_trace_carry(const irs_beam_carry_args a) {
    __shared__ float s_item[CARRY_MAXW * 64];
    __shared__ float s_tgt[CARRY_MAXW * 64];
    __shared__ int32_t s_rank[CARRY_MAXW * 64];
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwave = blockDim.x >> 6;
    const int W = a.W, ld = a.ld;
    const int step = a.step_ptr ? a.step_ptr[0] : a.step_arg;
    const size_t base = (size_t)(a.map ? a.map[b] : b) * W * ld; // the caller's user row
    // every lane < W holds one output slot's link word: what a row must deliver is asked of all of them at once
    const int lk = lane < W ? a.lk.link[b * W + lane] : IRS_BEAM_LINK_DEAD;
    for (int p = wave; p < W; p += nwave) { // input row p: columns [0, step) for its children, all of them for a whole copy
        const bool whole = __any(lk == (IRS_BEAM_LINK_COPY | p));
        const int n = whole ? ld : (step < ld ? step : ld);
        if (lane < n) {
            const size_t at = base + (size_t)p * ld + lane;
            s_item[p * 64 + lane] = a.lp_item[at];
            s_tgt[p * 64 + lane] = a.lp_target[at];
            s_rank[p * 64 + lane] = a.rank_target[at];
        }
    }
    __syncthreads();
    for (int t = wave; t < W; t += nwave) { // output slot t
        const int l = __shfl(lk, t, 64);
        if (l == (IRS_BEAM_LINK_COPY | t)) continue; // a copy of itself (a done user's every beam): not written
        float vi = 0.f, vt = 0.f;
        int32_t vr = 0;
        const int p = l & (IRS_BEAM_LINK_COPY - 1);
        if (l >= 0 && p < W) { // (any other word reads as dead)
            const bool whole = (l & IRS_BEAM_LINK_COPY) != 0;
            if (whole || lane < step) {
                vi = s_item[p * 64 + lane], vt = s_tgt[p * 64 + lane], vr = s_rank[p * 64 + lane];
            } else if (lane == step) { // the new column: how the target stood on the parent's row, and the item the child took
                const int prow = b * W + p;
                const double lse = (double)a.mx[prow] + log((double)a.sm[prow]);
                const int rk = a.rank[prow];
                vi = (float)((double)a.lk.val[b * W + t] - lse);
                vt = rk ? (float)((double)a.ts[prow] - lse) : 0.f;
                vr = rk;
            }
        }
        if (lane < ld) {
            const size_t at = base + (size_t)t * ld + lane;
            a.lp_item[at] = vi;
            a.lp_target[at] = vt;
            a.rank_target[at] = vr;
        }
    }
}

int irs_launch_beam_trace_carry(irs_ctx *ctx, const irs_beam_carry_args &a, int B, hipStream_t s) {
    const int waves = a.W < 4 ? 4 : (a.W > 8 ? 8 : a.W);
    hipLaunchKernelGGL(k_beam_trace_carry, dim3(B), dim3(64 * waves), 0, s, a);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}
