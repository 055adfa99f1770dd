// Projection + cross entropy over an item-sharded catalog (include/irs_hip.h: irs_ce_forward_sharded /
// irs_ce_backward_sharded; reference influentialRS.py:252-310 and evaluator.py:53-92, nn.Linear + nn.CrossEntropyLoss on ONE
// device).  Rows are data-parallel, the catalog is item-sharded, as in the sharded search loops (comm.hip): every rank
// gathers the world's rows, runs the single-device kernels over ITS shard for all of them, and what crosses the links is
// per row -- d floats of the row, 8 bytes of (log-sum-exp, label score) per shard, d floats of dL/dx per shard -- never
// anything of order rows x items.  Everything is one stream-ordered sequence on the caller's stream; buffers come from the
// context's workspace and the caller's scratch.
#include "irs_internal.h"

// ---- forward: the world's per-shard (lse, label score) of every row -> the row's log-sum-exp over the whole catalog and
// its label score.  pairs [world][2][R]: shard r's lse of row i at [r][0][i], its label score at [r][1][i] (-inf where the
// label is not in the shard).  Ranks are visited in rank order, so every rank computes the same bits.  One shard:
// exp(0) = 1, log(1) = 0 -- the shard's own values come back unchanged.
__global__ void __launch_bounds__(256) k_ce_shard_combine(const float *__restrict__ pairs, int world, int R, int own0, int B,
                                                          float *__restrict__ lse_all, float *__restrict__ lab_all,
                                                          float *__restrict__ lse_own, float *__restrict__ lab_own) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const size_t ld = (size_t)2 * R;
    float m = pairs[i], lab = pairs[R + i];
    for (int r = 1; r < world; ++r) {
        m = fmaxf(m, pairs[r * ld + i]);
        const float s = pairs[r * ld + R + i];
        if (s != -INFINITY) lab = s; // the one shard that holds the label
    }
    float sum = 0.f;
    for (int r = 0; r < world; ++r) sum += expf(pairs[r * ld + i] - m);
    const float lse = m + logf(sum);
    lse_all[i] = lse;
    lab_all[i] = lab;
    if (i >= own0 && i < own0 + B) {
        lse_own[i - own0] = lse;
        lab_own[i - own0] = lab;
    }
}

// ---- backward: dx of this rank's rows = the world's partials (one per shard, [world][n]) added in rank order
template <typename V>
__global__ void __launch_bounds__(256) k_ce_shard_sum_dx(const V *__restrict__ part, int world, int64_t n, V *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    V s = part[i];
    for (int r = 1; r < world; ++r) s += part[(size_t)r * n + i];
    out[i] = s;
}

static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// scratch of the sharded backward: [the fused backward's own scratch at R rows][dx partial R x d][exchanged partials R x d]
struct CeShardScratch {
    size_t off_part, off_recv, bytes;
};
static CeShardScratch ce_shard_scratch(const irs_ctx *ctx, int R) {
    CeShardScratch p;
    p.off_part = up256(irs_ce_bwd_scratch(ctx, R));
    p.off_recv = p.off_part + up256((size_t)R * ctx->dims.d * 4);
    p.bytes = p.off_recv + up256((size_t)R * ctx->dims.d * 4);
    return p;
}

extern "C" int irs_ce_forward_sharded(irs_ctx *ctx, irs_comm *comm, const float *xrows_local, const int64_t *labels0_local,
                                      int32_t B, float *lse, float *label_score, double *loss, void *stream) {
    int rc = irs_comm_check(ctx, comm, "irs_ce_forward_sharded");
    if (rc) return rc;
    if (!xrows_local || !labels0_local || !lse || !label_score || !loss)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_forward_sharded: null arguments");
    if (B < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_forward_sharded: B=%d", B);
    const int world = ctx->shard.world;
    if ((int64_t)B * world > ctx->max_rows)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_forward_sharded: B=%d needs max_rows >= world * B = %lld, it is %d", B,
                 (long long)B * world, ctx->max_rows);
    if (!ctx->finalized) IRS_FAIL(ctx, IRS_E_STATE, "weights not finalized (irs_finalize_weights)");
    if (!ctx->ws) IRS_FAIL(ctx, IRS_E_STATE, "workspace not bound (irs_bind_workspace)");
    hipStream_t s = (hipStream_t)stream;
    const int R = B * world, d = ctx->dims.d;
    ctx->proj_stale = true;
    int64_t *labels_all = ctx->top_ids;                      // [R]
    float *send = reinterpret_cast<float *>(ctx->keys_send); // [2][R]: this shard's lse | label score of every row
    if ((rc = irs_comm_allgather(ctx, comm, xrows_local, ctx->xrows, (size_t)B * d * sizeof(float), s))) return rc;
    if ((rc = irs_comm_allgather(ctx, comm, labels0_local, labels_all, (size_t)B * sizeof(int64_t), s))) return rc;
    if ((rc = irs_launch_refresh_bias(ctx, s))) return rc;
    if ((rc = irs_launch_lse(ctx, ctx->xrows, R, ctx->lse_max, ctx->lse_sum, s))) return rc;
    if ((rc = irs_launch_lse_combine(ctx, ctx->lse_max, ctx->lse_sum, send, R, s))) return rc;
    if ((rc = irs_launch_gather(ctx, ctx->xrows, R, labels_all, 1, send + R, s))) return rc;
    if ((rc = irs_comm_allgather(ctx, comm, send, ctx->ce_pairs, (size_t)2 * R * sizeof(float), s))) return rc;
    hipLaunchKernelGGL(k_ce_shard_combine, dim3((R + 255) / 256), dim3(256), 0, s, ctx->ce_pairs, world, R, ctx->shard.rank * B, B,
                       ctx->lse_max, ctx->lse_sum, lse, label_score);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    // the world's rows in gathered order through the single-device reduction: the same triple on every rank
    return irs_launch_ce_reduce(ctx, ctx->lse_max, ctx->lse_sum, labels_all, R, loss, s);
}

extern "C" size_t irs_ce_backward_sharded_scratch_bytes(const irs_ctx *ctx, int32_t B) {
    if (!ctx || B < 1 || (int64_t)B * ctx->shard.world > ctx->max_rows) return 0;
    return ce_shard_scratch(ctx, B * ctx->shard.world).bytes;
}

extern "C" int irs_ce_backward_sharded(irs_ctx *ctx, irs_comm *comm, const float *xrows_local, const int64_t *labels0_local,
                                       const float *lse, int32_t B, float scale, int32_t accumulate, float *dx, float *dw,
                                       float *db, void *scratch, size_t scratch_bytes, void *stream) {
    int rc = irs_comm_check(ctx, comm, "irs_ce_backward_sharded");
    if (rc) return rc;
    if (!xrows_local || !labels0_local || !lse || !dx || !dw || !db || !scratch)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_backward_sharded: null arguments");
    if (B < 1) IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_backward_sharded: B=%d", B);
    const int world = ctx->shard.world;
    if ((int64_t)B * world > ctx->max_rows)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_backward_sharded: B=%d needs max_rows >= world * B = %lld, it is %d", B,
                 (long long)B * world, ctx->max_rows);
    const int R = B * world, d = ctx->dims.d;
    const CeShardScratch p = ce_shard_scratch(ctx, R);
    if (scratch_bytes < p.bytes)
        IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_backward_sharded: scratch too small: %zu < %zu", scratch_bytes, p.bytes);
    if (((uintptr_t)scratch) & 15) IRS_FAIL(ctx, IRS_E_INVALID, "irs_ce_backward_sharded: scratch must be 16-byte aligned");
    if (!ctx->ws) IRS_FAIL(ctx, IRS_E_STATE, "workspace not bound (irs_bind_workspace)");
    if (!ctx->proj_w || !ctx->proj_b) IRS_FAIL(ctx, IRS_E_STATE, "irs_ce_backward_sharded: project.weight / project.bias not bound");
    hipStream_t s = (hipStream_t)stream;
    ctx->proj_stale = true;
    char *sc = static_cast<char *>(scratch);
    float *part = reinterpret_cast<float *>(sc + p.off_part), *recv = reinterpret_cast<float *>(sc + p.off_recv);
    int64_t *labels_all = ctx->top_ids; // [R]
    float *lse_all = ctx->lse_gmax;     // [R]
    if ((rc = irs_comm_allgather(ctx, comm, xrows_local, ctx->xrows, (size_t)B * d * sizeof(float), s))) return rc;
    if ((rc = irs_comm_allgather(ctx, comm, labels0_local, labels_all, (size_t)B * sizeof(int64_t), s))) return rc;
    if ((rc = irs_comm_allgather(ctx, comm, lse, lse_all, (size_t)B * sizeof(float), s))) return rc;
    // dw / db of the shard are complete after this; the dx partial of all R rows goes to `part`
    if ((rc = irs_launch_ce_backward(ctx, ctx->xrows, labels_all, lse_all, R, scale, accumulate, part, dw, db, sc, s))) return rc;
    // slice j of `part` (the rows of rank j) goes to rank j: this rank receives the world's partials of its own B rows
    if ((rc = irs_comm_alltoall(ctx, comm, part, recv, (size_t)B * d * sizeof(float), s))) return rc;
    const int64_t n = (int64_t)B * d;
    if ((n & 3) == 0 && (((uintptr_t)dx) & 15) == 0)
        hipLaunchKernelGGL(k_ce_shard_sum_dx<float4>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<const float4 *>(recv), world, n / 4, reinterpret_cast<float4 *>(dx));
    else
        hipLaunchKernelGGL(k_ce_shard_sum_dx<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, recv, world, n, dx);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}
