// Persuasion-path search step and the cross-shard top-k merge, gfx950.
//
// Replaces the per-row Python body of IRSNN.get_seq_in_batch
// (/root/reference model/influentialRS.py:419-450): window filter of the top-100,
// greedy / top-sample_k choice, path record, window grow / shift.  Runs entirely
// on the device so that one step can be captured into a hipGraph
// (no .item() host round trips; the reference pays B x 20 of them per batch).
#include "irs_internal.h"

// One wave per row (the row body lives in irs_internal.h: the one-launch small-shard top-k runs it in its tail).
// EXCL: with a bound exclusion set (irs_bind_exclusions); launched only while one is bound.
// SLOTS: the window image (irs_window): 4 registers per lane at max_len <= 256, 16 for long windows.
template <bool EXCL, int SLOTS>
__global__ void __launch_bounds__(256) k_path_step(const irs_path_args pa, int B, const float *__restrict__ val,
                                                   const int64_t *__restrict__ ids0, int k) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    irs_path_step_row<EXCL, SLOTS>(pa, row, lane, val, ids0, k);
}

__global__ void k_inc(int32_t *ctr) {
    if (threadIdx.x == 0 && blockIdx.x == 0) ctr[0] += 1;
}

// merge W lists of k entries per row: one workgroup per row, bitonic sort of <= 2048 keys.
// PACKED: the lists arrive as the exchange step's 64-bit keys (irs_hip.h: irs_pack_topk).
__device__ __forceinline__ unsigned long long irs_topk_key(float v, int64_t id) {
    return id >= 0 ? (((unsigned long long)irs_fkey(v) << 32) | (0xFFFFFFFFu - (unsigned int)id)) : 0ull;
}

__global__ void __launch_bounds__(256) k_pack_topk(const float *__restrict__ val, const int64_t *__restrict__ ids, int64_t n,
                                                   unsigned long long *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = irs_topk_key(val[i], ids[i]);
}

template <bool PACKED>
__global__ void __launch_bounds__(256) k_merge(const float *__restrict__ val_in, const int64_t *__restrict__ ids_in,
                                               const unsigned long long *__restrict__ keys_in, int W, int M, int k,
                                               float *__restrict__ val, int64_t *__restrict__ ids) {
    __shared__ unsigned long long keys[2048];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int n = W * k;
    int n2 = 2;
    while (n2 < n) n2 <<= 1;
    for (int i = tid; i < n2; i += 256) {
        unsigned long long key = 0ull;
        if (i < n) {
            const int w = i / k, c = i % k;
            const size_t at = ((size_t)w * M + row) * k + c;
            key = PACKED ? keys_in[at] : irs_topk_key(val_in[at], ids_in[at]);
        }
        keys[i] = key;
    }
    for (int size = 2; size <= n2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = tid; i < n2 / 2; i += 256) {
                int lo = 2 * i - (i & (stride - 1));
                int hi = lo + stride;
                bool desc = ((lo & size) == 0);
                unsigned long long a = keys[lo], b = keys[hi];
                if ((a < b) == desc) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < k; i += 256) {
        unsigned long long kk = (i < n2) ? keys[i] : 0ull;
        if (kk != 0ull) {
            val[(size_t)row * k + i] = irs_unkey((unsigned int)(kk >> 32));
            ids[(size_t)row * k + i] = (int64_t)(0xFFFFFFFFu - (unsigned int)kk);
        } else {
            val[(size_t)row * k + i] = -INFINITY;
            ids[(size_t)row * k + i] = -1;
        }
    }
}

// ------------------------------------------------------------------ beam search step
// BUILD-DEFINED extension (the reference has no beam search; BASELINE config 5).
// Per user: W beams, each a window + cumulative log-probability.  One step:
//   for every live beam j: survivors = its top-k candidates (descending) not present in its
//   window; the first W survivors become candidates with score cum[j] + log p(item | beam j),
//   log p = e - max - log(sumexp) (row-wise log-softmax over the whole catalog);
//   the best W candidates by (score desc, parent beam asc, rank within parent asc) become the
//   new beams: window grown / shifted exactly like the greedy step, path extended.
// W == 1 reduces to the greedy step of k_path_step bit for bit (the single live beam's first
// survivor wins whatever its score; lse_* may then be null).
// One workgroup (one wave per beam, at most 16 waves) per user; state is ping-ponged (in -> out).
// A beam's candidates are taken 64 at a time into registers (one per lane) before the survivor scan, so the
// scan is a chain of v_readlane + ballot, not of dependent global loads; the W best of the W*W candidates are ordered
// by rank counting (no barriers) instead of a full sort.
//
// UNTIL (irs_beam_step_until / irs_beam_search_until): the target of a window, seq[L - 1], is the search's end symbol.  A beam
// that has chosen it is FINISHED (fin = 1): it is no longer expanded, it competes with its final score as ONE candidate
// (index parent * W + 0; its val / ids0 / lse rows are never read and it never sets IRS_ROW_NO_CANDIDATE) and, when it survives,
// it is copied whole (window, hep, cum, all P path entries).  A user is DONE when no output beam is both live and unfinished
// (IRS_BEAM_STOP_ALL), or already when output beam 0 is finished (IRS_BEAM_STOP_BEST); a user that is done on entry is copied
// through, so a search gives the same result however rarely the host looks at `done`.
// Why BEST may stop there: a step adds log p(item | beam) <= 0 to an unfinished beam (val <= max and sum exp >= 1, the maximum's
// own term), so no later candidate scores above its unfinished ancestor of this step, all of which rank behind beam 0; a
// candidate that ties beam 0 loses by index, because a finished beam 0 re-enters as index 0 * W + 0, the smallest there is.  So
// beam 0 would stay beam 0 to the last step.  The float caveat: val, max and sum exp are float32 results of separate
// reductions.  Where a row's `max` is not the exact maximum of the scores its `val` were taken from (another summation order,
// a max taken over rounded scores), val - max can exceed 0 by an ulp of the score, and an unfinished beam within that ulp
// behind beam 0 could still overtake it under IRS_BEAM_STOP_ALL; BEST then returns the earlier answer.
// The instantiation without UNTIL is the kernel as it was: every addition sits behind `if constexpr`.
// EXCL (irs_bind_exclusions): a beam's survivors are its candidates outside window + the user's bound list + (no_repeat) the
// beam's own path so far, in.paths[row, 0 .. step): the parent's path of whatever it becomes.  All beams of a user read one list.
// A finished beam and a dead beam open nothing.  Without EXCL the kernel is, again, the one it was.
// LK (irs_beam_step_linked, the loops under irs_bind_beam_trace): a trailing irs_beam_link argument makes the LINKED form, which
// keeps every candidate's float32 list value beside its score and stores, per output beam row, the link word (irs_hip.h) and the
// chosen candidate's list value: what the carry kernel (beam_trace.hip) needs to move a beam's recorded columns along.  The link
// is a parameter PACK so that the forms without it keep their kernel arguments -- the offsets of the hidden ones behind them
// included -- and with them their instructions: every addition sits behind `if constexpr (LINK)`.
// RULED (irs_beam_step_ruled, the loops under irs_set_beam_rule): a second trailing argument, irs_beam_rule, makes the ruled form
// of the linked step; again a member of the pack, and every addition sits behind `if constexpr (RULED)`.
//   phase 1: a live unfinished beam reads its row's four sweep values once (the same address in every lane) and forms lpt, the
//     expression the beam trace stores as lp_target.  If the arrival test holds -- a clause, and the target admissible under the
//     walk's own test: a catalog item outside the window, the user's list, (no_repeat) the beam's path, and inside a bound offer set
//     (k_arrival_offer's search) -- the target is the beam's ONE candidate, with its sweep score as list value, and the list is not
//     walked; IRS_ROW_OFFERED goes to the user's status word.  Otherwise the walk, as ever.  Beside every score a KEY is kept in
//     LDS: score + (double)weight * (double)lpt of the parent (0 without a target, at a NaN lpt, for a finished beam, and at
//     weight == 0, so that 0 * -inf is never formed).
//   phase 2 ranks by (key desc, index asc); at weight == 0 the key has the score's bits and the order is the linked step's.
//   phase 3 is the linked step's: out.cum is the SCORE.  The end-symbol test makes the child of a fired beam finished.
// LDS: 8 + 8 + 4 + 8 KB of candidate arrays (28 KB of the 64 KB a workgroup may take); no float atomics.
#define BEAM_MAXW 32
template <typename T, typename... R>
__device__ __forceinline__ const T &irs_pack_first(const T &t, const R &...) { return t; }
template <typename T, typename U>
__device__ __forceinline__ const U &irs_pack_second(const T &, const U &u) { return u; }
// the ruled key's two operations, each rounded on its own as irs_hip.h states them: s + (double)lambda * (double)bonus is never
// contracted into one fused multiply-add, so that a replay in plain float64 forms the same bits
__device__ __forceinline__ double irs_beam_bonus(float weight, float lpt) {
#pragma clang fp contract(off)
    return (double)weight * (double)lpt;
}
__device__ __forceinline__ double irs_beam_key(double score, double add) {
#pragma clang fp contract(off)
    return score + add;
}
template <bool UNTIL, bool EXCL, int SLOTS, typename... LK>
__global__ void __launch_bounds__(1024) k_beam_step(const irs_beam_state in, const irs_beam_state out, const irs_beam_cand cand,
                                                    int W, int L, int step_arg, const int32_t *__restrict__ step_ptr, int P,
                                                    int32_t *__restrict__ status, const irs_beam_until until, const LK... lk) {
    constexpr bool LINK = sizeof...(LK) != 0, RULED = sizeof...(LK) == 2;
    __shared__ double c_score[BEAM_MAXW * BEAM_MAXW];
    __shared__ int64_t c_item[BEAM_MAXW * BEAM_MAXW];
    __shared__ float c_val[LINK ? BEAM_MAXW * BEAM_MAXW : 1]; // (LINK only: never referenced otherwise)
    __shared__ double c_key[RULED ? BEAM_MAXW * BEAM_MAXW : 1]; // (RULED only, likewise)
    __shared__ int c_order[BEAM_MAXW];
    __shared__ int s_flags[2]; // UNTIL: [0] some output beam is live and unfinished, [1] output beam 0 is finished
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwave = nthr >> 6;
    const int step = step_ptr ? step_ptr[0] : step_arg;
    const int WW = W * W, k = cand.k;
    if constexpr (UNTIL) {
        if (until.done[b]) { // (the same for the whole workgroup) a user that is done: every beam goes from in to out as it is
            for (int j = wave; j < W; j += nwave) {
                const size_t row = (size_t)b * W + j;
                for (int p = lane; p < L; p += 64) out.seq[row * L + p] = in.seq[row * L + p];
                for (int p = lane; p < P; p += 64) out.paths[row * P + p] = in.paths[row * P + p];
                if (lane == 0) {
                    out.hep[row] = in.hep[row];
                    out.cum[row] = in.cum[row];
                    out.fin[row] = in.fin[row];
                    if constexpr (LINK) {
                        const irs_beam_link &l = irs_pack_first(lk...);
                        l.link[row] = IRS_BEAM_LINK_COPY | j, l.val[row] = 0.f;
                    }
                }
            }
            return;
        }
        if (tid < 2) s_flags[tid] = 0;
    }
    for (int i = tid; i < WW; i += nthr) {
        c_score[i] = -INFINITY;
        c_item[i] = 0;
    }
    if (tid < BEAM_MAXW) c_order[tid] = WW; // "no candidate of this rank"
    __syncthreads();
    // phase 1: survivors of every live beam (one wave per beam)
    for (int j = wave; j < W; j += nwave) {
        const int row = b * W + j;
        const double cj = in.cum[row];
        int found = 0;
        if constexpr (UNTIL) {
            if (in.fin[row]) { // a finished beam: itself, with its final score; its lists are not read
                if (lane == 0 && cj > -INFINITY) {
                    c_score[j * W] = cj;
                    if constexpr (RULED) c_key[j * W] = cj; // (it has arrived: bonus 0, the largest lp_target there is)
                }
                continue;
            }
        }
        if (cj > -INFINITY) {
            const int64_t *w = in.seq + (size_t)row * L;
            irs_window<SLOTS> win;
            win.load(w, in.hep[row], L, lane);
            double norm = 0.0;
            if (cand.lse_max) norm = (double)cand.lse_max[row] + log((double)cand.lse_sum[row]);
            irs_excl_view ev = {};
            if constexpr (EXCL) ev = irs_excl_open(cand.ex, row, lane, step);
            bool more = true;
            double add = 0.0; // RULED: weight * lp_target of this row, the term every child of the beam carries in its key
            if constexpr (RULED) {
                const irs_beam_rule &ru = irs_pack_second(lk...);
                const int rk = ru.rank[row];
                if (rk != 0) {
                    const float tsv = ru.ts[row];
                    const float lpt = (float)((double)tsv - ((double)ru.mx[row] + log((double)ru.sm[row])));
                    if (ru.weight > 0.f && lpt == lpt) add = irs_beam_bonus(ru.weight, lpt);
                    // (a NaN lpt, or a NaN lp_min -- the clause is off --, never fires)
                    bool fire = (ru.rank_max >= 1 && rk <= ru.rank_max) || lpt >= ru.lp_min;
                    const int64_t t = w[L - 1];
                    fire = fire && t >= 1 && t <= ru.n_item;
                    if (fire && ru.oset) fire = irs_excl_listed(ru.oset, ru.on, t - 1); // (the same search in every lane)
                    if (fire) {
                        bool hit = false, listed = false;
                        if constexpr (EXCL) {
                            hit = (ev.pth == t);
                            listed = irs_excl_listed(ev.list, ev.n, t - 1); // (the same search in every lane)
                        }
                        hit = win.holds(t, hit);
                        if (!__any(hit) && !listed) { // the target alone: the list is not walked
                            if (lane == 0) {
                                const double sc = cj + ((double)tsv - norm);
                                c_score[j * W] = sc, c_key[j * W] = irs_beam_key(sc, add);
                                c_item[j * W] = t, c_val[j * W] = tsv;
                                atomicOr(&status[(UNTIL && until.map) ? until.map[b] : b], IRS_ROW_OFFERED);
                            }
                            found = 1, more = false;
                        }
                    }
                }
            }
            for (int c0 = 0; c0 < k && found < W && more; c0 += 64) { // 64 candidates per round, one per lane
                const int cl = c0 + lane;
                const int64_t cid = cl < k ? cand.ids0[(size_t)row * k + cl] : (int64_t)-1;
                const float cv = cl < k ? cand.val[(size_t)row * k + cl] : 0.f;
                unsigned long long listed = 0ull;
                if constexpr (EXCL) listed = __ballot(irs_excl_listed(ev.list, ev.n, cid));
                for (int c = 0; c < 64 && c0 + c < k && found < W; ++c) {
                    const int64_t id0 = __shfl(cid, c, 64);
                    if (id0 < 0) { // end of the list (fewer than k items on this shard / excluded)
                        more = false;
                        break;
                    }
                    const int64_t item = id0 + 1;
                    bool hit = false;
                    if constexpr (EXCL) hit = (ev.pth == item);
                    hit = win.holds(item, hit);
                    if constexpr (EXCL) hit |= (bool)((listed >> c) & 1ull);
                    if (!__any(hit)) {
                        const float v = __shfl(cv, c, 64);
                        if (lane == 0) {
                            c_score[j * W + found] = cj + ((double)v - norm);
                            c_item[j * W + found] = item;
                            if constexpr (LINK) c_val[j * W + found] = v;
                            if constexpr (RULED) c_key[j * W + found] = irs_beam_key(cj + ((double)v - norm), add);
                        }
                        ++found;
                    }
                }
            }
            if (found == 0 && lane == 0) atomicOr(&status[(UNTIL && until.map) ? until.map[b] : b], IRS_ROW_NO_CANDIDATE);
        }
    }
    __syncthreads();
    // phase 2: rank of every candidate by (score desc, index asc), index = parent * W + rank in parent; ranks < W survive
    for (int x = tid; x < WW; x += nthr) {
        const double sx = c_score[x];
        if (sx > -INFINITY) {
            int rank = 0;
            if constexpr (RULED) { // by key, among the slots that hold a candidate (a key may be -inf; a score of one is not)
                const double kx = c_key[x];
                for (int y = 0; y < WW; ++y) {
                    const double ky = c_key[y];
                    rank += (c_score[y] > -INFINITY && (ky > kx || (ky == kx && y < x))) ? 1 : 0;
                }
            } else {
                for (int y = 0; y < WW; ++y) {
                    const double sy = c_score[y];
                    rank += (sy > sx || (sy == sx && y < x)) ? 1 : 0;
                }
            }
            if (rank < W) c_order[rank] = x;
        }
    }
    __syncthreads();
    // phase 3: materialise the new beams (one wave per new beam)
    for (int t = wave; t < W; t += nwave) {
        const int ci = c_order[t];
        const double sc = ci < WW ? c_score[ci] : -INFINITY;
        const int orow = b * W + t;
        int64_t *wo = out.seq + (size_t)orow * L;
        float *po = out.paths + (size_t)orow * P;
        if (!(sc > -INFINITY)) { // dead beam: keep a well-formed (copied) window, never selected again
            const int64_t *wi = in.seq + (size_t)(b * W) * L;
            for (int p = lane; p < L; p += 64) wo[p] = wi[p];
            for (int p = lane; p < P; p += 64) po[p] = 0.f;
            if (lane == 0) {
                out.cum[orow] = -INFINITY;
                out.hep[orow] = in.hep[b * W];
                if constexpr (UNTIL) out.fin[orow] = 0;
                if constexpr (LINK) {
                    const irs_beam_link &l = irs_pack_first(lk...);
                    l.link[orow] = IRS_BEAM_LINK_DEAD, l.val[orow] = 0.f;
                }
            }
            continue;
        }
        const int parent = ci / W;
        const int prow = b * W + parent;
        const int64_t item = c_item[ci];
        const int64_t *wi = in.seq + (size_t)prow * L;
        const float *pi = in.paths + (size_t)prow * P;
        const int he = in.hep[prow];
        if constexpr (UNTIL) {
            if (in.fin[prow]) { // a finished beam that survived: copied whole
                for (int p = lane; p < L; p += 64) wo[p] = wi[p];
                for (int p = lane; p < P; p += 64) po[p] = pi[p];
                if (lane == 0) {
                    out.hep[orow] = he;
                    out.cum[orow] = sc;
                    out.fin[orow] = 1;
                    if (t == 0) s_flags[1] = 1;
                    if constexpr (LINK) {
                        const irs_beam_link &l = irs_pack_first(lk...);
                        l.link[orow] = IRS_BEAM_LINK_COPY | parent, l.val[orow] = 0.f;
                    }
                }
                continue;
            }
        }
        if (he < L - 2) { // grow
            for (int p = lane; p < L; p += 64) wo[p] = (p == he + 1) ? item : wi[p];
            if (lane == 0) out.hep[orow] = he + 1;
        } else { // shift, target stays last
            for (int p = lane; p < L; p += 64) wo[p] = (p < L - 2) ? wi[p + 1] : (p == L - 2 ? item : wi[L - 1]);
            if (lane == 0) out.hep[orow] = he;
        }
        for (int p = lane; p < P; p += 64) po[p] = (p < step) ? pi[p] : (p == step ? (float)item : 0.f);
        if (lane == 0) out.cum[orow] = sc;
        if constexpr (LINK) {
            if (lane == 0) {
                const irs_beam_link &l = irs_pack_first(lk...);
                l.link[orow] = parent, l.val[orow] = c_val[ci];
            }
        }
        if constexpr (UNTIL) {
            const int f = item == wi[L - 1] ? 1 : 0; // the end symbol: the parent window's target
            if (lane == 0) {
                out.fin[orow] = f;
                if (!f) atomicOr(&s_flags[0], 1);
                if (f && t == 0) s_flags[1] = 1;
            }
        }
    }
    if constexpr (UNTIL) {
        __syncthreads();
        if (tid == 0) until.done[b] = (!s_flags[0] || (until.stop_rule == IRS_BEAM_STOP_BEST && s_flags[1])) ? 1 : 0;
    }
}

// beam state initialisation: beam 0 = the input window with score 0, others dead copies
__global__ void k_beam_init(const int64_t *__restrict__ seq0, const int64_t *__restrict__ user0,
                            const int32_t *__restrict__ hep0, int B, int W, int L, int P, const irs_beam_state st,
                            int64_t *__restrict__ user) {
    const int row = blockIdx.x; // b * W + j
    const int b = row / W, j = row % W;
    for (int p = threadIdx.x; p < L; p += blockDim.x) st.seq[(size_t)row * L + p] = seq0[(size_t)b * L + p];
    for (int p = threadIdx.x; p < P; p += blockDim.x) st.paths[(size_t)row * P + p] = 0.f;
    if (threadIdx.x == 0) {
        user[row] = user0 ? user0[b] : 0;
        st.hep[row] = hep0[b];
        st.cum[row] = (j == 0) ? 0.0 : -INFINITY;
    }
}

int irs_launch_beam_init(irs_ctx *ctx, const int64_t *seq0, const int64_t *user0, const int32_t *hep0, int B, int W, int P,
                         const irs_beam_state &st, int64_t *user, hipStream_t s) {
    hipLaunchKernelGGL(k_beam_init, dim3(B * W), dim3(64), 0, s, seq0, user0, hep0, B, W, ctx->dims.max_len, P, st, user);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

int irs_launch_beam_step(irs_ctx *ctx, const irs_beam_state &in, const irs_beam_state &out, const irs_beam_cand &cand, int B, int W,
                         int step, const int32_t *step_ptr, int P, int32_t *status, const irs_beam_until *until, hipStream_t s,
                         const irs_beam_link *link, const irs_beam_rule *rule) {
    if (W < 1 || W > BEAM_MAXW) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "beam width %d outside [1, %d]", W, BEAM_MAXW);
    const int waves = W < 4 ? 4 : (W > 16 ? 16 : W);
    constexpr int S4 = IRS_WIN_SLOTS_SHORT, S16 = IRS_WIN_SLOTS_LONG;
    if (link && rule) { // the ruled forms: the link and the rule as the trailing arguments
        using LK = irs_beam_link;
        using RU = irs_beam_rule;
        const auto kern = irs_window_slots(ctx) == S4
                              ? (cand.ex.on ? (until ? k_beam_step<true, true, S4, LK, RU> : k_beam_step<false, true, S4, LK, RU>)
                                            : (until ? k_beam_step<true, false, S4, LK, RU> : k_beam_step<false, false, S4, LK, RU>))
                              : (cand.ex.on ? (until ? k_beam_step<true, true, S16, LK, RU> : k_beam_step<false, true, S16, LK, RU>)
                                            : (until ? k_beam_step<true, false, S16, LK, RU> : k_beam_step<false, false, S16, LK, RU>));
        hipLaunchKernelGGL(kern, dim3(B), dim3(64 * waves), 0, s, in, out, cand, W, ctx->dims.max_len, step, step_ptr, P, status,
                           until ? *until : irs_beam_until{}, *link, *rule);
        IRS_CHECK_HIP(ctx, hipGetLastError());
        return IRS_OK;
    }
    if (link) { // the linked forms: the same choice of UNTIL / EXCL / SLOTS, the link as the trailing argument
        using LK = irs_beam_link;
        const auto kern = irs_window_slots(ctx) == S4
                              ? (cand.ex.on ? (until ? k_beam_step<true, true, S4, LK> : k_beam_step<false, true, S4, LK>)
                                            : (until ? k_beam_step<true, false, S4, LK> : k_beam_step<false, false, S4, LK>))
                              : (cand.ex.on ? (until ? k_beam_step<true, true, S16, LK> : k_beam_step<false, true, S16, LK>)
                                            : (until ? k_beam_step<true, false, S16, LK> : k_beam_step<false, false, S16, LK>));
        hipLaunchKernelGGL(kern, dim3(B), dim3(64 * waves), 0, s, in, out, cand, W, ctx->dims.max_len, step, step_ptr, P, status,
                           until ? *until : irs_beam_until{}, *link);
        IRS_CHECK_HIP(ctx, hipGetLastError());
        return IRS_OK;
    }
    const auto kern = irs_window_slots(ctx) == S4
                          ? (cand.ex.on ? (until ? k_beam_step<true, true, S4> : k_beam_step<false, true, S4>)
                                        : (until ? k_beam_step<true, false, S4> : k_beam_step<false, false, S4>))
                          : (cand.ex.on ? (until ? k_beam_step<true, true, S16> : k_beam_step<false, true, S16>)
                                        : (until ? k_beam_step<true, false, S16> : k_beam_step<false, false, S16>));
    hipLaunchKernelGGL(kern, dim3(B), dim3(64 * waves), 0, s, in, out, cand, W, ctx->dims.max_len, step, step_ptr, P, status,
                       until ? *until : irs_beam_until{});
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

// After a step of irs_beam_search_until: a done user's W beams leave for the caller's outputs at user row map[r]; a live user's
// beams move to user slot dst[r] of the OTHER state set (never in place: the step's input set is free by then), with its map entry
// and a cleared done flag.  dst is k_until_scan's over `done` (-1: done); dst == nullptr: every user leaves (the last step).
// One wave per beam row.
__global__ void __launch_bounds__(256) k_beam_retire(const int32_t *__restrict__ dst, int B, int W, int L, int P,
                                                     const irs_beam_state in, const irs_beam_side side_in, const irs_beam_state out,
                                                     const irs_beam_side side_out, const irs_beam_out res) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B * W) return;
    const int r = row / W, j = row - r * W;
    const int t = dst ? dst[r] : -1;
    if (t < 0) {
        const size_t orow = (size_t)(side_in.map ? side_in.map[r] : r) * W + j;
        for (int p = lane; p < P; p += 64) res.paths[orow * P + p] = in.paths[(size_t)row * P + p];
        if (res.seq)
            for (int p = lane; p < L; p += 64) res.seq[orow * L + p] = in.seq[(size_t)row * L + p];
        if (lane == 0) {
            res.scores[orow] = in.cum[row];
            if (res.fin) res.fin[orow] = in.fin[row];
        }
        return;
    }
    const size_t trow = (size_t)t * W + j;
    for (int p = lane; p < L; p += 64) out.seq[trow * L + p] = in.seq[(size_t)row * L + p];
    for (int p = lane; p < P; p += 64) out.paths[trow * P + p] = in.paths[(size_t)row * P + p];
    if (lane == 0) {
        side_out.user[trow] = side_in.user[row];
        out.hep[trow] = in.hep[row];
        out.cum[trow] = in.cum[row];
        out.fin[trow] = in.fin[row];
        if (j == 0) {
            side_out.map[t] = side_in.map ? side_in.map[r] : r;
            side_out.done[t] = 0;
        }
    }
}

int irs_launch_beam_retire(irs_ctx *ctx, const int32_t *dst, int B, int W, int P, const irs_beam_state &in,
                           const irs_beam_side &side_in, const irs_beam_state &out, const irs_beam_side &side_out,
                           const irs_beam_out &res, hipStream_t s) {
    hipLaunchKernelGGL(k_beam_retire, dim3((B * W + 3) / 4), dim3(256), 0, s, dst, B, W, ctx->dims.max_len, P, in, side_in, out,
                       side_out, res);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

int irs_launch_merge(irs_ctx *ctx, const float *val_in, const int64_t *ids_in, int W, int M, int k, float *val,
                     int64_t *ids0, hipStream_t s) {
    if (W * k > 2048) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "merge of %d x %d entries exceeds 2048", W, k);
    hipLaunchKernelGGL(k_merge<false>, dim3(M), dim3(256), 0, s, val_in, ids_in, (const unsigned long long *)nullptr, W, M, k, val, ids0);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

int irs_launch_merge_keys(irs_ctx *ctx, const uint64_t *keys_in, int W, int M, int k, float *val, int64_t *ids0, hipStream_t s) {
    if (W * k > 2048) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "merge of %d x %d entries exceeds 2048", W, k);
    hipLaunchKernelGGL(k_merge<true>, dim3(M), dim3(256), 0, s, (const float *)nullptr, (const int64_t *)nullptr,
                       reinterpret_cast<const unsigned long long *>(keys_in), W, M, k, val, ids0);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

int irs_launch_pack_topk(irs_ctx *ctx, const float *val, const int64_t *ids0, int64_t n, uint64_t *keys, hipStream_t s) {
    hipLaunchKernelGGL(k_pack_topk, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, val, ids0, n,
                       reinterpret_cast<unsigned long long *>(keys));
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

int irs_launch_path_step(irs_ctx *ctx, const irs_path_args &pa, int B, const float *val, const int64_t *ids0, int k, hipStream_t s) {
    if (ctx->opt.guide.on) return irs_launch_path_step_guided(ctx, pa, B, val, ids0, k, s); // (irs_bind_guide: guide.hip)
    constexpr int S4 = IRS_WIN_SLOTS_SHORT, S16 = IRS_WIN_SLOTS_LONG;
    const auto kern = irs_window_slots(ctx) == S4 ? (pa.ex.on ? k_path_step<true, S4> : k_path_step<false, S4>)
                                                  : (pa.ex.on ? k_path_step<true, S16> : k_path_step<false, S16>);
    hipLaunchKernelGGL(kern, dim3((B + 3) / 4), dim3(256), 0, s, pa, B, val, ids0, k);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

int irs_launch_inc(irs_ctx *ctx, int32_t *ctr, hipStream_t s) {
    hipLaunchKernelGGL(k_inc, dim3(1), dim3(64), 0, s, ctr);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

// ------------------------------------------------------------------ path trace (irs_bind_path_trace)
// After a path step, before the step counter moves (and, in the until loop, before k_until_record sets fin): the item the step
// chose is read back from the window it was put into -- seq[r][hep[r]] after a grow, seq[r][L - 2] after a shift; the path entry
// is a float32 and only says whether anything was chosen -- and looked up in the lists the step chose from, whose score is the
// chain's.  A chosen item is always in its list (NaN would say otherwise).  One wave per row.
__global__ void __launch_bounds__(256) k_trace_record(const irs_trace_rec t, const int64_t *__restrict__ seq,
                                                      const int32_t *__restrict__ hep, int L, const float *__restrict__ paths,
                                                      int path_ld, const int32_t *__restrict__ step_ptr, const int32_t *__restrict__ map,
                                                      const int32_t *__restrict__ fin, const float *__restrict__ val,
                                                      const int64_t *__restrict__ ids0, int k, int B) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= B) return;
    if (fin && fin[r]) return;
    const int step = step_ptr[0];
    const double lse = (double)t.mx[r] + log((double)t.sm[r]);
    float lpi = 0.f;
    if (paths[(size_t)r * path_ld + step] != 0.f) {
        const int he = hep[r];
        const int64_t id0 = seq[(size_t)r * L + (he < L - 2 ? (he > 0 ? he : 0) : L - 2)] - 1;
        lpi = __uint_as_float(0x7FC00000u);
        for (int c0 = 0; c0 < k; c0 += 64) {
            const unsigned long long hit = __ballot(c0 + lane < k && ids0[(size_t)r * k + c0 + lane] == id0);
            if (hit) {
                lpi = (float)((double)val[(size_t)r * k + c0 + (__ffsll((long long)hit) - 1)] - lse);
                break;
            }
        }
    }
    if (lane == 0) {
        const size_t at = (size_t)(map ? map[r] : r) * t.ld + step;
        const int rk = t.rank[r];
        t.lp_item[at] = lpi;
        t.lp_target[at] = rk ? (float)((double)t.ts[r] - lse) : 0.f;
        t.rank_target[at] = rk;
    }
}

int irs_launch_trace_record(irs_ctx *ctx, const irs_trace_rec &t, const int64_t *seq, const int32_t *hep, const float *paths,
                            int path_ld, const int32_t *step_ptr, const int32_t *map, const int32_t *fin, const float *val,
                            const int64_t *ids0, int k, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_trace_record, dim3((B + 3) / 4), dim3(256), 0, s, t, seq, hep, ctx->dims.max_len, paths, path_ld, step_ptr, map,
                       fin, val, ids0, k, B);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

// ------------------------------------------------------------------ arrival rule (irs_set_arrival_rule, irs_arrival_offer)
// Behind the trace sweep, before the step chooses: a live row whose target stands at rank <= rank_max among what the window
// leaves, or at log-probability >= lp_min (the expression k_trace_record stores, so the decision can be replayed from the
// recorded arrays), and is admissible under the step's own test -- a catalog item outside the window seq[row][0 .. hep], the
// user's bound list and (no_repeat) the row's path so far -- gets its list rewritten to the target alone: (ts, t - 1), then the
// end mark.  The unchanged step kernels then choose it as the only survivor.  Rows that do not fire are not written.
// One wave per row; no LDS, no atomics (the status word is this row's, and the step kernels behind write it the same way).
// OFFER: an offer set is bound (irs_bind_offer_set): a target that is not one of oset[0 .. on) is not offered -- one binary search
// of the ascending ids, irs_excl_listed's.
template <bool EXCL, int SLOTS, bool OFFER>
__global__ void __launch_bounds__(256) k_arrival_offer(const int64_t *__restrict__ seq, const int32_t *__restrict__ hep, int L, int B,
                                                       int64_t n_item, const float *__restrict__ mx, const float *__restrict__ sm,
                                                       const float *__restrict__ ts, const int32_t *__restrict__ rank,
                                                       const int32_t *__restrict__ fin, float *__restrict__ val,
                                                       int64_t *__restrict__ ids0, int k, int rank_max, float lp_min,
                                                       int32_t *__restrict__ status, const irs_excl ex,
                                                       const int64_t *__restrict__ oset, int on) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    if (fin && fin[row]) return;
    const int rk = rank[row];
    if (rk == 0) return; // no target
    const float tsv = ts[row];
    bool fire = rank_max >= 1 && rk <= rank_max;
    if (!fire && lp_min <= 0.f) { // (the probability clause is on: irs_arrival_lp_on)
        const float lp = (float)((double)tsv - ((double)mx[row] + log((double)sm[row])));
        fire = lp >= lp_min; // (a NaN lp never fires)
    }
    if (!fire) return;
    const int64_t *w = seq + (size_t)row * L;
    const int64_t t = w[L - 1];
    if (t < 1 || t > n_item) return;
    if constexpr (OFFER) {
        if (!irs_excl_listed(oset, on, t - 1)) return; // (the same search in every lane)
    }
    irs_window<SLOTS> win;
    win.load(w, hep[row], L, lane);
    bool hit = false, listed = false;
    if constexpr (EXCL) {
        const irs_excl_view ev = irs_excl_open(ex, row, lane, ex.step_ptr ? ex.step_ptr[0] : ex.step_arg);
        hit = (ev.pth == t);
        listed = irs_excl_listed(ev.list, ev.n, t - 1); // (the same search in every lane)
    }
    hit = win.holds(t, hit);
    if (__any(hit) || listed) return;
    if (lane == 0) {
        val[(size_t)row * k] = tsv;
        ids0[(size_t)row * k] = t - 1;
        status[row] |= IRS_ROW_OFFERED;
    } else if (lane == 1 && k > 1) {
        val[(size_t)row * k + 1] = -INFINITY;
        ids0[(size_t)row * k + 1] = -1;
    }
}

int irs_launch_arrival_offer(irs_ctx *ctx, const int64_t *seq, const int32_t *hep, int B, const float *mx, const float *sm,
                             const float *ts, const int32_t *rank, const int32_t *fin, float *val, int64_t *ids0, int k, int rank_max,
                             float lp_min, int32_t *status, const irs_excl &ex, hipStream_t s) {
    constexpr int S4 = IRS_WIN_SLOTS_SHORT, S16 = IRS_WIN_SLOTS_LONG;
    const auto &of = ctx->opt.offer; // a bound offer set: the target must be in it
    const bool s4 = irs_window_slots(ctx) == S4;
    const auto kern = of.on ? (s4 ? (ex.on ? k_arrival_offer<true, S4, true> : k_arrival_offer<false, S4, true>)
                                  : (ex.on ? k_arrival_offer<true, S16, true> : k_arrival_offer<false, S16, true>))
                            : (s4 ? (ex.on ? k_arrival_offer<true, S4, false> : k_arrival_offer<false, S4, false>)
                                  : (ex.on ? k_arrival_offer<true, S16, false> : k_arrival_offer<false, S16, false>));
    hipLaunchKernelGGL(kern, dim3((B + 3) / 4), dim3(256), 0, s, seq, hep, ctx->dims.max_len, B, ctx->dims.n_item, mx, sm, ts, rank, fin,
                       val, ids0, k, rank_max, lp_min, status, ex, of.on ? of.ids : nullptr, of.on ? (int)of.n : 0);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

// ------------------------------------------------------------------ stop-at-target search (irs_generate_paths_until)
// The reference never stops at the target: it runs every step for every user and zeroes the tail on the host afterwards
// (model/influentialRS.py:459-467).  Here a user is finished after the step that chose seq[b][L - 1]; the three kernels below
// record a step of the live (compacted) rows into the caller's rows, and compact the rows that are still live.

// After a step on B compacted rows: the chosen item (stage[r][step]) and the step's status bits go to the caller's row map[r].
// The comparison is the host's (float32 path entry == int64 target, both as doubles).  A row that finishes here gets its tail
// zeroed once; a row that finished at an earlier step (still stepped until the next compaction) writes nothing.  One wave per row.
// `stage` is never cleared: this kernel relies on the path step writing stage[r][step] for EVERY row of EVERY step -- the chosen item,
// or 0 for a row without a candidate (irs_path_step_row writes paths[row][step] before it looks at `found`) -- so that no entry of
// an earlier step or call is ever read.  All lanes of the row's wave read fin[r] and step_status[r] before lane 0 rewrites them.
__global__ void __launch_bounds__(256) k_until_record(const float *__restrict__ stage, int P, int step,
                                                      const int32_t *__restrict__ map, const int64_t *__restrict__ seq, int L, int B,
                                                      int32_t *__restrict__ fin, int32_t *__restrict__ step_status,
                                                      float *__restrict__ paths, int32_t *__restrict__ status) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= B) return;
    const int was = fin[r];
    const int bits = step_status[r];
    if (bits && lane == 0) step_status[r] = 0;
    if (was) return;
    const int orig = map ? map[r] : r;
    const float item = stage[(size_t)r * P + step];
    const bool done = (double)item == (double)seq[(size_t)r * L + L - 1];
    float *row = paths + (size_t)orig * P;
    if (lane == 0) {
        row[step] = item;
        if (bits) status[orig] |= bits;
        if (done) fin[r] = 1;
    }
    if (done)
        for (int p = step + 1 + lane; p < P; p += 64) row[p] = 0.f;
}

// dst[r] = number of live rows before r (the row's place after compaction), -1 for a finished row; count[0] = live rows.
// ONE workgroup walks the rows 1024 at a time: ballot + popcount inside a wave, the 16 wave totals through LDS.
__global__ void __launch_bounds__(1024) k_until_scan(const int32_t *__restrict__ fin, int B, int32_t *__restrict__ dst,
                                                     int32_t *__restrict__ count) {
    __shared__ int s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int r0 = 0; r0 < B; r0 += 1024) {
        const int r = r0 + tid;
        const bool live = r < B && fin[r] == 0;
        const unsigned long long m = __ballot(live);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            const int c = s_wave[w];
            off += w < wave ? c : 0;
            total += c;
        }
        if (r < B) dst[r] = live ? base + off + before : -1;
        base += total;
        __syncthreads();
    }
    if (tid == 0) count[0] = base;
}

// Row r of the current state moves to row dst[r] of the other buffer set (never in place); one wave per row.
__global__ void __launch_bounds__(256) k_until_gather(const int32_t *__restrict__ dst, int B, int L,
                                                      const int64_t *__restrict__ seq, const int64_t *__restrict__ user,
                                                      const int32_t *__restrict__ hep, const int32_t *__restrict__ map,
                                                      int64_t *__restrict__ seq_out, int64_t *__restrict__ user_out,
                                                      int32_t *__restrict__ hep_out, int32_t *__restrict__ map_out) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= B) return;
    const int t = dst[r];
    if (t < 0) return;
    for (int p = lane; p < L; p += 64) seq_out[(size_t)t * L + p] = seq[(size_t)r * L + p];
    if (lane == 0) {
        if (user) user_out[t] = user[r];
        hep_out[t] = hep[r];
        map_out[t] = map ? map[r] : r;
    }
}

__global__ void k_set_step(int32_t *step_pair, int step) {
    if (threadIdx.x == 0 && blockIdx.x == 0) step_pair[0] = step, step_pair[1] = step;
}

int irs_launch_until_record(irs_ctx *ctx, const float *stage, int P, int step, const int32_t *map, const int64_t *seq, int B,
                            int32_t *fin, int32_t *step_status, float *paths, int32_t *status, hipStream_t s) {
    hipLaunchKernelGGL(k_until_record, dim3((B + 3) / 4), dim3(256), 0, s, stage, P, step, map, seq, ctx->dims.max_len, B, fin,
                       step_status, paths, status);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

int irs_launch_until_scan(irs_ctx *ctx, const int32_t *fin, int B, int32_t *dst, int32_t *count, hipStream_t s) {
    hipLaunchKernelGGL(k_until_scan, dim3(1), dim3(1024), 0, s, fin, B, dst, count);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

int irs_launch_until_gather(irs_ctx *ctx, const int32_t *dst, int B, const int64_t *seq, const int64_t *user, const int32_t *hep,
                            const int32_t *map, int64_t *seq_out, int64_t *user_out, int32_t *hep_out, int32_t *map_out,
                            hipStream_t s) {
    hipLaunchKernelGGL(k_until_gather, dim3((B + 3) / 4), dim3(256), 0, s, dst, B, ctx->dims.max_len, seq, user, hep, map, seq_out,
                       user_out, hep_out, map_out);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

int irs_launch_set_step(irs_ctx *ctx, int32_t *step_pair, int step, hipStream_t s) {
    hipLaunchKernelGGL(k_set_step, dim3(1), dim3(64), 0, s, step_pair, step);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

// ------------------------------------------------------------------ evaluation batch on the device
// Replaces the per-user Python of DataProvider.get_random_evaluate_data (data_provider.py:398-449: history =
// all but the last event, label = the last event, target = a random item absent from the last raw_len
// history items) and DataLoaderEvalIRS._collate_fn (:591-617: pre-padded window, gap zeros, target last).
// One wave per user.  The target is drawn by rejection from a counter RNG (splitmix64 of (seed, user,
// attempt)) over [1, n_item] or over an explicit candidate pool (the reference's `popular_item` set):
// distributional parity with random.sample, exact parity of everything else.
__global__ void __launch_bounds__(64) k_build_eval_batch(const irs_eval_batch_args a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t lo = a.offsets[b], hi = a.offsets[b + 1];
    const int64_t n_hist = hi - lo - 1;                       // history = all but the last event
    const int rn = (int)(n_hist < a.raw_len ? (n_hist < 0 ? 0 : n_hist) : a.raw_len);
    const int64_t *rw = a.items + lo + (n_hist - rn);         // the raw window, oldest first
    int64_t tgt = 0;
    if (a.targets_in) {
        tgt = a.targets_in[b];
    } else {
        const int64_t space = a.pool ? a.n_pool : a.n_item;
        bool found = false;
        for (int attempt = 0; attempt < 256 && !found; ++attempt) {
            unsigned long long z = a.seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)b * 2654435761ull + (unsigned long long)attempt + 1ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z = z ^ (z >> 31);
            const unsigned long long pick = __umul64hi(z, (unsigned long long)space); // uniform in [0, space)
            const int64_t cand = a.pool ? a.pool[pick] : (int64_t)pick + 1;
            bool hit = false;
            for (int i = lane; i < rn; i += 64) hit |= (rw[i] == cand);
            if (!__any(hit)) {
                tgt = cand;
                found = true;
            }
        }
        if (!found && lane == 0 && a.status) a.status[b] |= IRS_ROW_NO_CANDIDATE;
    }
    const int l_history = a.L - a.gap_len - 1;
    const int nh = rn < l_history ? rn : l_history;           // seq[-l_history:] of the raw window
    const int start = a.L - nh - a.gap_len - 1;
    int64_t *row = a.seq + (int64_t)b * a.L;
    for (int t = lane; t < a.L; t += 64) {
        int64_t v = 0;
        if (t >= start && t < start + nh) v = rw[rn - nh + (t - start)];
        if (t == a.L - 1) v = tgt;
        row[t] = v;
    }
    if (a.raw)
        for (int i = lane; i < a.raw_len; i += 64) a.raw[(int64_t)b * a.raw_len + i] = (i >= a.raw_len - rn) ? rw[i - (a.raw_len - rn)] : 0;
    if (lane == 0) {
        a.target[b] = tgt;
        a.label[b] = (hi > lo) ? a.items[hi - 1] : 0;
        if (a.raw_n) a.raw_n[b] = rn;
    }
}

int irs_launch_build_eval_batch(irs_ctx *ctx, const irs_eval_batch_args &a, hipStream_t s) {
    if (a.L - a.gap_len - 1 < 1) IRS_FAIL(ctx, IRS_E_UNSUPPORTED, "gap_len %d leaves no history slot in a window of %d", a.gap_len, a.L);
    hipLaunchKernelGGL(k_build_eval_batch, dim3(a.B), dim3(64), 0, s, a);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}
