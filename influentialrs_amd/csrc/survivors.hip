// Exact candidates for rows whose top-k list is hidden by their window (irs_topk_ensure_survivors, include/irs_hip.h).
// A search step chooses among the k best items of the catalog after dropping those in the row's window; when fewer than `want`
// of them survive, the row is STARVED: the step would see fewer continuations than the catalog holds.  Three launches repair it:
//   k_surv_flag    one wave per row: counts the list's survivors with the path step's own membership test and records the
//                  starved rows (count + list in the caller's scratch);
//   k_surv_strips  the recorded rows' exact scores over the whole float32 shard, cut into item strips like k_exh_strips
//                  (score.hip): a workgroup keeps the best `want` keys of its strip that are NOT in the row's window;
//   k_surv_merge   one workgroup per recorded row: the best `want` of the strips' keys become the row's list.
// The last two return at once when nothing was recorded.  No float atomics, and a row's result does not depend on its place
// in the recorded list: two identical calls give identical bits.
// With a bound exclusion set (irs_bind_exclusions; the EXCL forms, launched only while one is bound) "window" reads "window +
// the user's list + (no_repeat) the row's path so far" in all of the above; k_excl_prepare, at the end, is the binding's launch.
// With a bound offer set (irs_bind_offer_set; the OFFER forms) "the whole float32 shard" reads "the set": the strips cut the
// sanitised id array, a key carries the LOCAL index (local order is id order: the set ascends), and the window test and the
// output map local -> global through the array.  A hole scores nothing.  k_surv_flag is the same kernel either way.
#include "irs_internal.h"

#define SURV_STRIPS 256          // item strips of a large shard
#define SURV_STRIP_MIN_ITEMS 128 // a strip holds at least this many items (smaller shards: fewer strips, down to one)
#define SURV_KEYS_CAP (1 << 21)  // rows x strips x want <= this (16 MiB of keys) while strips > 1: the strip count shrinks
#define SURV_BUF 512             // keys of LDS per selection: compacted to `want` whenever more than SURV_BUF - 256 are held
// surv_select appends at most 256 keys between two looks at the held count and compacts to `want` keys as soon as more than
// SURV_BUF - 256 are held: a slot stays below SURV_BUF as long as want <= SURV_BUF - 256.  The public pass asks for at most 32
// (irs_topk_ensure_survivors), irs_recommend for at most IRS_MAX_RECOMMEND.
static_assert(IRS_MAX_RECOMMEND <= SURV_BUF - 256 && IRS_MAX_GUIDE_KC <= SURV_BUF - 256, "surv_select: want must fit between two compactions");
#define SURV_ROW_GROUPS 64       // workgroups that share the recorded rows, per strip and in the merge: each loops over its rows
#define SURV_HDR 256             // bytes in front of the list: word 0 is the count

static inline size_t surv_align16(size_t v) { return (v + 15) & ~(size_t)15; }

static int surv_strips(int64_t n_local, int rows, int want) {
    int ns = 1;
    while (ns < SURV_STRIPS && (int64_t)ns * 2 * SURV_STRIP_MIN_ITEMS <= n_local) ns <<= 1;
    while (ns > 1 && (int64_t)rows * ns * want > SURV_KEYS_CAP) ns >>= 1;
    return ns;
}

size_t irs_surv_scratch(const irs_ctx *ctx, int rows, int want) {
    const int ns = surv_strips(ctx->n_local, rows, want);
    return SURV_HDR + surv_align16((size_t)rows * sizeof(int32_t)) + (size_t)rows * ns * want * sizeof(unsigned long long);
}

// ---- flag pass: one wave per row.  The list is walked in order, 64 ids at a time (one per lane, broadcast by shuffle): it ends
// at the first negative id (a list that ended early is the whole catalog: not starved), and the walk stops as soon as `want`
// survivors are seen.  Only a row that shows all k valid entries and fewer than `want` survivors is recorded.
template <bool EXCL, int SLOTS>
__global__ void __launch_bounds__(256) k_surv_flag(const irs_excl ex, const int64_t *__restrict__ seq, int L, const int32_t *__restrict__ hep, int M,
                                                   int rps, int k, int want, const double *__restrict__ cum,
                                                   const int32_t *__restrict__ fin, const int32_t *__restrict__ done,
                                                   const int64_t *__restrict__ ids0, unsigned int *__restrict__ count,
                                                   int32_t *__restrict__ list) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    if (cum && cum[row] == -INFINITY) return;
    if (fin && fin[row] != 0) return;
    if (done && done[row / rps] != 0) return;
    const int64_t *w = seq + (size_t)row * L;
    irs_window<SLOTS> win; // window = seq[row, 0 .. hep]
    win.load(w, hep[row], L, lane);
    int found = 0;
    bool ended = false;
    irs_excl_view ev = {};
    if constexpr (EXCL) ev = irs_excl_open(ex, row, lane, ex.step_ptr ? ex.step_ptr[0] : ex.step_arg);
    for (int c0 = 0; c0 < k && !ended && found < want; c0 += 64) {
        const int c = c0 + lane;
        const long long mine = c < k ? (long long)ids0[(size_t)row * k + c] : -1ll;
        const int n_here = k - c0 < 64 ? k - c0 : 64;
        unsigned long long listed = 0ull;
        if constexpr (EXCL) listed = __ballot(irs_excl_listed(ev.list, ev.n, (int64_t)mine));
        for (int i = 0; i < n_here; ++i) {
            const long long id0 = __shfl(mine, i, 64);
            if (id0 < 0) {
                ended = true;
                break;
            }
            const int64_t item = id0 + 1;
            bool hit = false;
            if constexpr (EXCL) hit = (ev.pth == item) || ((listed >> i) & 1ull);
            hit = win.holds(item, hit);
            if (!__any(hit) && ++found >= want) break;
        }
    }
    if (!ended && found < want && lane == 0) list[atomicAdd(count, 1u)] = row;
}

// bitonic sort of n (a power of two) values in LDS by the whole workgroup; DESC: largest first
template <typename T, bool DESC>
__device__ __forceinline__ void surv_bitonic(T *a, int n) {
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < n / 2; i += blockDim.x) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const bool first = ((lo & size) == 0) == DESC; // this pair keeps its larger value first
                const T u = a[lo], v = a[hi];
                if ((u < v) == first) {
                    a[lo] = v;
                    a[hi] = u;
                }
            }
        }
    }
    __syncthreads();
}

// Streaming top-`want` of the keys keyfn(j), j in [j0, j1) (0 = no key): leaves the best min(n, want) admitted keys sorted
// descending in buf[0 ..) and returns their number.  admit(key) is asked only for a key that has beaten the running threshold
// (the want-th best admitted key so far), so its cost is paid for the few keys that could still enter the result.
// The held count is read into a register between two barriers: no thread can append to the next chunk while another still
// decides whether to compact.
template <typename KeyFn, typename AdmitFn>
__device__ __forceinline__ unsigned int surv_select(KeyFn &&keyfn, AdmitFn &&admit, int64_t j0, int64_t j1, int want,
                                                    unsigned long long *buf) {
    __shared__ unsigned int s_n;
    __shared__ unsigned long long s_thr;
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid == 0) {
        s_n = 0;
        s_thr = 0ull;
    }
    __syncthreads();
    for (int64_t base = j0; base < j1; base += 256) {
        const int64_t j = base + tid;
        if (j < j1) {
            const unsigned long long key = keyfn(j);
            if (key > s_thr && admit(key)) buf[atomicAdd(&s_n, 1u)] = key; // (at most 256 held at the loop's top: the slot is < SURV_BUF)
        }
        __syncthreads();
        const unsigned int n = s_n;
        __syncthreads();
        if (n > SURV_BUF - 256) {
            for (int i = n + tid; i < SURV_BUF; i += 256) buf[i] = 0ull;
            surv_bitonic<unsigned long long, true>(buf, SURV_BUF);
            if (tid == 0) {
                s_n = (n < (unsigned int)want) ? n : want;
                if (n >= (unsigned int)want) s_thr = buf[want - 1];
            }
            __syncthreads();
        }
    }
    const unsigned int n = s_n;
    for (int i = n + tid; i < SURV_BUF; i += 256) buf[i] = 0ull;
    surv_bitonic<unsigned long long, true>(buf, SURV_BUF);
    return n < (unsigned int)want ? n : (unsigned int)want;
}

// ---- exhaustive pass over the strips.  grid (strips, y): workgroup (s, y) serves recorded rows y, y + gridDim.y, ... on strip s,
// so one pass over the float32 shard serves all recorded rows together (a strip stays in cache from row to row).  The row's
// window ids are sorted into LDS once per (workgroup, row); an item is searched there only after its key has beaten the
// running threshold.  EXCL: the row's path entries are sorted in with the window (INT64_MAX fills both), and an item that is in
// neither is searched in the user's bound row.
// WSLOTS: window slots of the sort buffer, 256 (max_len <= 256) or IRS_MAX_LEN_LONG.
// OFFER: the items are oids[0 .. n_local) (n_local = the set's size), not [0, n_local) of the shard.
template <bool EXCL, int WSLOTS, bool OFFER>
__global__ void __launch_bounds__(256) k_surv_strips(const irs_excl ex, const float *__restrict__ x, int d, const float *__restrict__ W,
                                                     const float *__restrict__ bias, int64_t n_local, int64_t item_lo,
                                                     const int64_t *__restrict__ seq, int L, const int32_t *__restrict__ hep,
                                                     int want, int n_strips, const unsigned int *__restrict__ count,
                                                     const int32_t *__restrict__ list, unsigned long long *__restrict__ keys,
                                                     const int64_t *__restrict__ oids) {
    __shared__ unsigned long long buf[SURV_BUF];
    __shared__ float xs[256];
    constexpr int WIN = EXCL ? 2 * WSLOTS : WSLOTS; // EXCL: the window slots + IRS_MAX_PATH path slots, up to a power of two for the sort
    static_assert(IRS_MAX_PATH <= 256 && WSLOTS >= 256 && (WSLOTS & (WSLOTS - 1)) == 0, "path entries share the sorted window");
    __shared__ long long win[WIN];
    const unsigned int n_rows = *count;
    if (n_rows == 0u) return;
    const int tid = threadIdx.x;
    const int strip = blockIdx.x;
    const int64_t per = (n_local + n_strips - 1) / n_strips;
    const int64_t j0 = (int64_t)strip * per, j1 = (j0 + per < n_local) ? j0 + per : n_local;
    for (unsigned int fi = blockIdx.y; fi < n_rows; fi += gridDim.y) {
        const int row = list[fi];
        int wl = hep[row] + 1;
        wl = wl < 0 ? 0 : (wl > L ? L : wl);
        __syncthreads();
        for (int i = tid; i < d; i += 256) xs[i] = x[(size_t)row * d + i];
        if constexpr (WSLOTS == 256) // (L <= 256 = the workgroup)
            win[tid] = tid < wl ? (long long)seq[(size_t)row * L + tid] : 0x7FFFFFFFFFFFFFFFll;
        else
            for (int p = tid; p < WSLOTS; p += 256) win[p] = p < wl ? (long long)seq[(size_t)row * L + p] : 0x7FFFFFFFFFFFFFFFll;
        const int64_t *xl = nullptr; // EXCL: the user's bound row
        int xn = 0;
        if constexpr (EXCL) { // (thread tid < IRS_MAX_PATH opens path entry tid)
            const irs_excl_view ev = irs_excl_open(ex, row, tid, ex.step_ptr ? ex.step_ptr[0] : ex.step_arg);
            if constexpr (WSLOTS == 256)
                win[256 + tid] = (tid < IRS_MAX_PATH && ev.pth > 0) ? (long long)ev.pth : 0x7FFFFFFFFFFFFFFFll;
            else
                for (int p = tid; p < WSLOTS; p += 256)
                    win[WSLOTS + p] = (p < IRS_MAX_PATH && ev.pth > 0) ? (long long)ev.pth : 0x7FFFFFFFFFFFFFFFll;
            xl = ev.list, xn = ev.n;
        }
        surv_bitonic<long long, false>(win, WIN);
        const unsigned int n = surv_select(
            [&](int64_t j) -> unsigned long long {
                int64_t id = j;
                if constexpr (OFFER) {
                    id = oids[j];
                    if (id < 0) return 0ull; // (a hole: no key)
                }
                const float e = irs_chain(xs, W + (size_t)id * d, bias[id], d);
                return ((unsigned long long)irs_fkey(e) << 32) | (0xFFFFFFFFu - (unsigned int)j);
            },
            [&](unsigned long long key) -> bool { // the item is not in win[0 .. wl)
                const int64_t loc = (int64_t)(0xFFFFFFFFu - (unsigned int)key);
                const long long item = (long long)((OFFER ? oids[loc] : item_lo + loc) + 1);
                const int wn = EXCL ? WIN : wl; // (EXCL: window and path entries lie mixed in front of the fill)
                int lo = 0, hi = wn;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (win[mid] < item) lo = mid + 1;
                    else hi = mid;
                }
                if constexpr (EXCL) return !(lo < wn && win[lo] == item) && !irs_excl_listed(xl, xn, (int64_t)item - 1);
                return !(lo < wn && win[lo] == item);
            },
            j0, j1, want, buf);
        unsigned long long *o = keys + ((size_t)fi * n_strips + strip) * want;
        for (int i = tid; i < want; i += 256) o[i] = i < (int)n ? buf[i] : 0ull;
    }
}

// ---- list rewrite: the best `want` of a recorded row's strip keys, in the library's order; the list ends behind them
// (oids: the offer form's id array, through which a key's local index leaves; null: the index is the shard's)
__global__ void __launch_bounds__(256) k_surv_merge(int64_t item_lo, int k, int want, int n_strips, int rps,
                                                    const unsigned int *__restrict__ count, const int32_t *__restrict__ list,
                                                    const unsigned long long *__restrict__ keys, const int32_t *__restrict__ status_map,
                                                    float *__restrict__ val, int64_t *__restrict__ ids, int32_t *__restrict__ status,
                                                    const int64_t *__restrict__ oids) {
    __shared__ unsigned long long buf[SURV_BUF];
    const unsigned int n_rows = *count;
    if (n_rows == 0u) return;
    for (unsigned int fi = blockIdx.x; fi < n_rows; fi += gridDim.x) {
        const int row = list[fi];
        const unsigned long long *src = keys + (size_t)fi * n_strips * want;
        const unsigned int n = surv_select([&](int64_t j) -> unsigned long long { return src[j]; },
                                           [](unsigned long long) -> bool { return true; }, 0, (int64_t)n_strips * want, want, buf);
        for (int i = threadIdx.x; i <= (int)n && i < k; i += 256) {
            const unsigned long long kk = buf[i];
            const bool live = i < (int)n;
            val[(size_t)row * k + i] = live ? irs_unkey((unsigned int)(kk >> 32)) : -INFINITY;
            const int64_t loc = (int64_t)(0xFFFFFFFFu - (unsigned int)kk);
            ids[(size_t)row * k + i] = live ? (oids ? oids[loc] : item_lo + loc) : (int64_t)-1;
        }
        if (threadIdx.x == 0) {
            const int u = row / rps;
            atomicOr(&status[status_map ? status_map[u] : u], IRS_ROW_RESCUED);
        }
        __syncthreads();
    }
}

int irs_launch_survivors(irs_ctx *ctx, const irs_surv_args &a, void *scratch, hipStream_t s) {
    // the layout is the one the scratch was sized for (rows_cap >= M rows): the strip count is not monotone in the row count
    const int ns = surv_strips(ctx->n_local, a.rows_cap, a.want);
    unsigned int *count = (unsigned int *)scratch;
    int32_t *list = (int32_t *)((char *)scratch + SURV_HDR);
    unsigned long long *keys = (unsigned long long *)((char *)list + surv_align16((size_t)a.rows_cap * sizeof(int32_t)));
    const int L = ctx->dims.max_len;
    IRS_CHECK_HIP(ctx, hipMemsetAsync(count, 0, sizeof(unsigned int), s));
    constexpr int S4 = IRS_WIN_SLOTS_SHORT, S16 = IRS_WIN_SLOTS_LONG;
    const bool long_win = irs_window_slots(ctx) != S4;
    const auto k_flag = long_win ? (a.ex.on ? k_surv_flag<true, S16> : k_surv_flag<false, S16>)
                                 : (a.ex.on ? k_surv_flag<true, S4> : k_surv_flag<false, S4>);
    // a bound offer set: the repair comes from the set (the strip count stays the one the scratch was sized for)
    const auto &of = ctx->opt.offer;
    const int64_t *oids = of.on ? of.ids : nullptr;
    const int64_t n_span = of.on ? of.n : ctx->n_local;
    constexpr int LW = IRS_MAX_LEN_LONG;
    const auto k_strips = of.on ? (long_win ? (a.ex.on ? k_surv_strips<true, LW, true> : k_surv_strips<false, LW, true>)
                                            : (a.ex.on ? k_surv_strips<true, 256, true> : k_surv_strips<false, 256, true>))
                                : (long_win ? (a.ex.on ? k_surv_strips<true, LW, false> : k_surv_strips<false, LW, false>)
                                            : (a.ex.on ? k_surv_strips<true, 256, false> : k_surv_strips<false, 256, false>));
    hipLaunchKernelGGL(k_flag, dim3((a.M + 3) / 4), dim3(256), 0, s, a.ex, a.seq, L, a.hep, a.M, a.rps, a.k, a.want, a.cum, a.fin, a.done,
                       a.ids0, count, list);
    int ny = 4096 / ns < 4 ? 4 : (4096 / ns > SURV_ROW_GROUPS ? SURV_ROW_GROUPS : 4096 / ns);
    if (ny > a.M) ny = a.M;
    hipLaunchKernelGGL(k_strips, dim3(ns, ny), dim3(256), 0, s, a.ex, a.xrows, ctx->dims.d, ctx->proj_w, ctx->proj_b, n_span,
                       ctx->shard.item_lo, a.seq, L, a.hep, a.want, ns, count, list, keys, oids);
    hipLaunchKernelGGL(k_surv_merge, dim3(a.M < SURV_ROW_GROUPS ? a.M : SURV_ROW_GROUPS), dim3(256), 0, s, ctx->shard.item_lo, a.k, a.want, ns, a.rps, count, list,
                       keys, a.status_map, a.val, a.ids0, a.status, oids);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    return IRS_OK;
}

// ------------------------------------------------------------------ bound exclusions: the binding's one launch
// One workgroup per user: the valid ids of the caller's row (0 <= id < n_item; -1 holes anywhere, duplicates kept) sorted
// ascending in LDS, INT64_MAX behind them up to `stride` (the power of two the scratch rows have), and their number.
static int excl_stride(int n_excl) {
    int n2 = 1;
    while (n2 < n_excl) n2 <<= 1;
    return n_excl > 0 ? n2 : 0;
}

size_t irs_excl_scratch(int users, int n_excl) {
    return surv_align16((size_t)users * sizeof(int32_t)) + (size_t)users * excl_stride(n_excl) * sizeof(int64_t);
}

__global__ void __launch_bounds__(256) k_excl_prepare(const int64_t *__restrict__ ids0, int n_excl, int stride, int64_t n_item,
                                                      int32_t *__restrict__ cnt, int64_t *__restrict__ rows) {
    __shared__ long long a[IRS_MAX_EXCL];
    __shared__ int s_n;
    const int u = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < stride; i += 256) {
        const long long id = i < n_excl ? (long long)ids0[(size_t)u * n_excl + i] : -1ll;
        const bool ok = id >= 0 && id < (long long)n_item;
        a[i] = ok ? id : 0x7FFFFFFFFFFFFFFFll;
        mine += ok ? 1 : 0;
    }
    if (mine) atomicAdd(&s_n, mine);
    if (stride > 1) surv_bitonic<long long, false>(a, stride);
    else __syncthreads();
    for (int i = tid; i < stride; i += 256) rows[(size_t)u * stride + i] = (int64_t)a[i];
    if (tid == 0) cnt[u] = s_n;
}

int irs_launch_excl_prepare(irs_ctx *ctx, const int64_t *ids0, int users, int n_excl, void *scratch, hipStream_t s) {
    int32_t *cnt = (int32_t *)scratch;
    int64_t *rows = (int64_t *)((char *)scratch + surv_align16((size_t)users * sizeof(int32_t)));
    const int stride = excl_stride(n_excl);
    hipLaunchKernelGGL(k_excl_prepare, dim3(users), dim3(256), 0, s, ids0, n_excl, stride, ctx->dims.n_item, cnt, rows);
    IRS_CHECK_HIP(ctx, hipGetLastError());
    ctx->opt.excl.cnt = cnt;
    ctx->opt.excl.rows = stride ? rows : nullptr;
    ctx->opt.excl.stride = stride;
    return IRS_OK;
}
