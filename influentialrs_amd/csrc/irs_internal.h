// Internal declarations shared by the HIP translation units of libirs_hip.so.
// gfx950 (CDNA4) only: wave = 64 lanes, MFMA 32x32 tiles, 160 KiB LDS per CU.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/irs_hip.h"

// Lab switches.  The kernels carry measurement hooks (phase stamps, fragment dumps, "run without the MFMAs / DMA / barrier"
// variants) that tools/*_lab.hip turn on by including a kernel source with the switch defined.  Several of them change what
// a kernel COMPUTES, so a stray -D must never produce a library: every switch is legal only together with IRS_LAB, which
// influentialrs_amd/build.py never defines (and tests/test_cabi.py checks that it does not).
// The condition names exactly the switches the sources under csrc/ test (tests/test_cabi.py compares the two sets).
#if !defined(IRS_LAB) && (defined(X6_DUMP) || defined(X6_STAMP) || defined(X6_NO_SPLIT) || defined(X6_NO_MFMA) ||            \
                          defined(X6_NO_READS) || defined(X6_NO_DMA) || defined(X6_NO_BARRIER) || defined(X6_NO_QKV_STORE) ||  \
                          defined(X6_NW) || defined(SEQ_EXP) || defined(PLAN_STAMP) || defined(ATTN_STAMP) ||                  \
                          defined(IRS_SMALL_TIMING) || defined(IRS_DIRECT_TIMING))
#error "a lab switch (X6_* / SEQ_EXP / *_STAMP / IRS_*_TIMING) is defined without IRS_LAB: the product library must be built without them"
#endif

#include <atomic>
#include <functional>
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) and occupancy are PER DEVICE: the "done once" flags of the launchers are a
// bit per device ordinal (setting the attribute twice from two host threads is harmless, so a plain atomic mask suffices)
#define IRS_MAX_DEVICES 32
static inline int irs_cur_dev() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= IRS_MAX_DEVICES) d = 0;
    return d;
}
#define IRS_ONCE_PER_DEVICE(body_)                                                                                        \
    do {                                                                                                                  \
        static std::atomic<unsigned> once_mask_{0};                                                                       \
        const unsigned once_bit_ = 1u << irs_cur_dev();                                                                   \
        if (!(once_mask_.load(std::memory_order_acquire) & once_bit_)) {                                                  \
            body_;                                                                                                        \
            once_mask_.fetch_or(once_bit_, std::memory_order_release);                                                    \
        }                                                                                                                 \
    } while (0)

#define IRS_MAX_LAYERS 16
#define IRS_CAND_BUCKETS 64 // candidate lists per row (bucket = item tile mod 64)
#define IRS_CAND_SLOTS 64   // entries per bucket
#define IRS_CAND_CAP (IRS_CAND_BUCKETS * IRS_CAND_SLOTS) // emitted candidates kept per row by the sweep
#define IRS_REFINE_CAP 1024 // candidates exactly re-scored per row
#define IRS_MAX_GROUPS 2048 // pre-pass group maxima per row (upper bound: the pre-pass is decomposed to stay below it)
#define IRS_MAX_PATH 64     // beam-search path length bound
#define IRS_MAX_EXCL 4096   // ids of a user's bound exclusion list (irs_bind_exclusions): one LDS sort, <= 13 probes per search
#define IRS_LSE_SLOTS_RING 4096 // (max, sum) partial slots of the <= 32-row ring log-sum-exp sweep: 2048 waves x 2 lane halves
#define IRS_COOP_FALLBACK_MIN_ITEMS 262144 // shards from this size up redo flagged rows cooperatively (score.hip: k_exh_strips)
#define IRS_EXH_SCRATCH_KEYS (64 * 32768)  // EXH_FB_MAX x EXH_KEYS_PER_ROW keys of scratch for it

struct irs_layer_w {
    const float *sa_in_w, *sa_in_b, *sa_out_w, *sa_out_b;
    const float *ca_in_w, *ca_in_b, *ca_out_w, *ca_out_b;
    const float *l1_w, *l1_b, *l2_w, *l2_b;
    const float *n1_w, *n1_b, *n2_w, *n2_b, *n3_w, *n3_b;
};

struct irs_prof_ev {
    hipEvent_t a, b;
};

// ---- captured steps.  A search loop captures its step body once as a hipGraph and replays it.  The body bakes in kernel
// choices, workspace addresses, the call's arguments and the search options bound at the time.  The cache key holds the call:
// its arguments and the caller's pointers -- a loop fills ONE key (fields it does not bake in stay zero) and irs_replay_steps
// compares it as a whole.  Everything else is covered by the drop: whatever changes a kernel choice, the workspace, the derived
// weights or a search option (capi.hip: opts_changed) destroys the captured steps (irs_drop_graphs), so a key never meets a step
// captured under other bindings.
enum { IRS_STEP_GREEDY = 1, IRS_STEP_BEAM, IRS_STEP_SHARDED_BEAM, IRS_STEP_SHARDED_BEAM_SPLIT };
struct irs_step_key {
    int32_t kind, B, W, P, k, sweep, sample, sample_k;
    uint64_t seed;
    const void *comm, *seq, *user, *hep, *paths, *status;
};
static_assert(sizeof(irs_step_key) == 8 * sizeof(int32_t) + 7 * 8, "irs_step_key is compared with memcmp: no padding");
struct irs_step_graph {
    hipGraphExec_t exec; // null: nothing captured
    irs_step_key key;
};

// ---- bound exclusions as the kernels take them (irs_bind_exclusions; capi.hip: excl_args).  All zero: nothing is bound, and
// every launcher then takes the kernel form without the test (what the library launched before exclusions existed).
struct irs_excl {
    const int64_t *rows;     // [users][stride] a user's valid ids0, ascending, INT64_MAX behind them
    const int32_t *cnt;      // [users] valid ids of the row
    const int32_t *map;      // user slot of this call -> bound user (the until loops' compaction map); null: the identity
    const float *paths;      // no_repeat: the path rows whose non-zero entries [0, step) are dropped too; null: off
    const int32_t *step_ptr; // the survivor pass's step index (the step kernels pass their own): device counter, or step_arg
    int stride, div;         // div: rows per user slot (1, W, or rows_per_status): row r belongs to slot r / div
    int path_ld, path_by_user; // the path row is the bound user's (the greedy loops: the caller's rows) or row r itself (beam state)
    int step_arg, on;
};

// ---- beam-search state.  A step reads one side of the ping-pong state and writes the other; the kernels take these by value.
struct irs_beam_state {
    int64_t *seq; // [max_seqs][L]
    int32_t *hep; // [max_seqs]
    double *cum;  // [max_seqs]
    float *paths; // [max_seqs][P <= IRS_MAX_PATH]
    int32_t *fin; // [max_seqs] the beam has chosen its target (the until forms only)
};
// what moves at the compactions of irs_beam_search_until only; the plain and the sharded search use side 0's `user`
struct irs_beam_side {
    int64_t *user;      // [max_seqs]
    int32_t *done;      // [max_seqs] (by user) nothing is left to decide
    int32_t *map;  // compacted user -> the caller's row; null = identity (the loop sets it: un_map[side] after a compaction)
};
struct irs_beam_cand { // the candidate lists of a step's rows; lse_* null: W == 1
    const float *val;
    const int64_t *ids0;
    const float *lse_max, *lse_sum;
    int k;
    irs_excl ex; // bound exclusions (zero: none); the path rows are the step's input state
};
struct irs_beam_until { // what a step of the until forms takes besides (map as in irs_beam_side)
    int32_t *done;
    const int32_t *map;
    int stop_rule;
};
struct irs_beam_out { // the caller's outputs of irs_beam_search_until; fin and seq may be null
    float *paths;
    double *scores;
    int32_t *fin;
    int64_t *seq;
};
// ---- path trace (irs_bind_path_trace).  The caller's scratch holds, per row of a step: the sweep's before-count and the local
// id of the target, then what the record kernel reads after the step -- (max, sum exp), the target's score, its rank.
struct irs_trace_rows {
    unsigned long long *count; // [rows] items of the whole catalog ranked before the target
    int64_t *refid;            // [rows] local 0-based id of the target, -1: no target (t == 0, or outside the catalog)
    float *mx, *sm, *ts;       // [rows] max, sum exp(e - max), target score
    int32_t *rank;             // [rows] 1 + count - window correction; 0: no target
};
static inline size_t irs_trace_layout(void *base, int rows, irs_trace_rows *o) {
    const size_t r8 = ((size_t)rows * 8 + 255) / 256 * 256, r4 = ((size_t)rows * 4 + 255) / 256 * 256;
    if (o) {
        char *p = (char *)base;
        o->count = (unsigned long long *)p, o->refid = (int64_t *)(p + r8);
        o->mx = (float *)(p + 2 * r8), o->sm = (float *)(p + 2 * r8 + r4), o->ts = (float *)(p + 2 * r8 + 2 * r4);
        o->rank = (int32_t *)(p + 2 * r8 + 3 * r4);
    }
    return 2 * r8 + 4 * r4;
}
struct irs_trace_rec { // what the record kernel takes: a step's rows (the scratch) and the caller's three [users][ld] arrays
    const float *mx, *sm, *ts;
    const int32_t *rank;
    float *lp_item, *lp_target;
    int32_t *rank_target;
    int ld;
};
// ---- admissible rank (irs_bind_trace_admissible, irs_score_target_rank_admissible; admissible.hip).  What k_trace_rank_adm takes
// behind the trace sweep: the sweep's rows, the step's bound exclusions (list, map, path, step index), a bound offer set with the
// scores of the row pass, and where the value goes -- out[row] by launch row, and (rec != null) the caller's [users][ld] cell of
// the step, exactly where k_trace_record writes rank_target: row rec_map[row] (null: row), column rec_step[0], unless rec_fin[row].
struct irs_adm_args {
    const float *xrows;  // [M][d]
    const int64_t *seq;  // [M][L]
    const int32_t *hep;  // [M]
    int M;
    const float *ts;                 // [M] the target's score
    const int64_t *refid;            // [M] its local 0-based id, -1: no target
    const unsigned long long *count; // [M] items of the whole catalog ranked before it
    irs_excl ex;                     // zero: neither a list nor a path
    const int64_t *oids;             // a bound offer set's sanitised ids [on] (null: none)
    int64_t on, oc_pad;
    const float *osc;                // [M][oc_pad] the set's scores of these rows
    const int32_t *oholes;           // [1] holes of the set: != 0 and the ids need not ascend
    int32_t *out;                    // [M]
    int32_t *rec;                    // [users][rec_ld] or null
    int rec_ld;
    const int32_t *rec_map, *rec_fin, *rec_step;
};
static inline size_t irs_adm_layout(int rows) { return ((size_t)rows * 4 + 255) / 256 * 256; } // the step's values by launch row
// ---- beam trace (irs_bind_beam_trace; beam_trace.hip).  A linked beam step says, per output beam row, where it came from (the
// link word of irs_hip.h: IRS_BEAM_LINK_DEAD, parent p, or IRS_BEAM_LINK_COPY | p) and the list value of the candidate it chose
// (0 where it chose none); the carry kernel moves the recorded columns along.  Both null: the step as it was.
struct irs_beam_link {
    int32_t *link; // [B * W]
    float *val;    // [B * W]
};
// the bound scratch: the trace sweep's rows for `rows` = users * W beam rows, then the link words and the link values
static inline size_t irs_beam_trace_layout(void *base, int rows, irs_trace_rows *tr, irs_beam_link *lk) {
    const size_t head = irs_trace_layout(base, rows, tr), r4 = ((size_t)rows * 4 + 255) / 256 * 256;
    if (lk) lk->link = (int32_t *)((char *)base + head), lk->val = (float *)((char *)base + head + r4);
    return head + 2 * r4;
}
// ---- beam rule (irs_set_beam_rule; path.hip: the ruled form of k_beam_step).  What the ruled step takes behind the link: the
// trace sweep's four values on the step's INPUT rows, the rule, and what the arrival test needs besides the step's own arguments.
struct irs_beam_rule {
    const float *mx, *sm, *ts; // [B * W]
    const int32_t *rank;       // [B * W]
    int rank_max;              // 0: the rank clause is off
    float lp_min;              // NaN: the probability clause is off
    float weight;              // lambda >= 0; 0: the key is the score
    int64_t n_item;
    const int64_t *oset;       // a bound offer set's ascending ids0 (null: none): a target outside it is not offered
    int on;                    // ids in oset
};
struct irs_beam_carry_args { // irs_beam_trace_carry's arguments as the kernel takes them
    irs_beam_link lk;                  // by launch row b * W + j
    const float *mx, *sm, *ts;         // [B * W] the sweep's results on the step's INPUT rows
    const int32_t *rank;               // [B * W]
    int W, ld, step_arg;
    const int32_t *step_ptr;           // device step counter, or step_arg
    float *lp_item, *lp_target;        // [users][W][ld], by the caller's user row
    int32_t *rank_target;
    const int32_t *map;                // launch user -> the caller's user row; null: the identity
};
// ---- a bound guide as the guided path step takes it (irs_bind_guide; guide.hip).  table: the packed words [rows][words] of a
// binary guide (in the caller's scratch) or the caller's float32 [rows][F] table, rows = n_item + 1, row i = 1-based item i.
struct irs_guide {
    const void *table;
    int64_t rows;
    int F, words, k_c, kind;
};
// ---- a bound lookahead (irs_bind_lookahead; lookahead.hip).  The caller's scratch holds, for `rows` parent rows and N = rows * k_c
// children (child row * k_c + j): what the expand step writes, what the inner decode / LSE / gather write, and what the choose
// step writes.  Every array is rounded up to 256 bytes; a call on fewer rows uses the heads of the same arrays.
struct irs_look_rows {
    int64_t *seq;    // [N][L] child windows
    int64_t *user;   // [N] the parent's user (0 without one)
    int64_t *tgt0;   // [N] the parent's target as a 0-based id (t - 1): the inner gather's id list
    int64_t *ids0;   // [N] candidate ids, 0-based, -1: no candidate
    int32_t *hep;    // [N]
    float *x;        // [N][d] the children's decoded rows
    float *mx, *sm, *ts; // [N] max, sum exp(e - max), the target's score on the child row
    float *val;      // [N] the candidates' scores in the parent's list
    float *lp;       // [N] what the choose step compared
    int32_t *choice; // [rows] the chosen slot, -1: none
};
static inline size_t irs_look_layout(void *base, int rows, int k_c, int L, int d, irs_look_rows *o) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t N = (size_t)rows * k_c;
    const size_t n_seq = up(N * L * 8), r8 = up(N * 8), r4 = up(N * 4), n_x = up(N * d * 4), c4 = up((size_t)rows * 4);
    if (o) {
        char *p = (char *)base;
        o->seq = (int64_t *)p, p += n_seq;
        o->user = (int64_t *)p, p += r8;
        o->tgt0 = (int64_t *)p, p += r8;
        o->ids0 = (int64_t *)p, p += r8;
        o->hep = (int32_t *)p, p += r4;
        o->x = (float *)p, p += n_x;
        o->mx = (float *)p, p += r4;
        o->sm = (float *)p, p += r4;
        o->ts = (float *)p, p += r4;
        o->val = (float *)p, p += r4;
        o->lp = (float *)p, p += r4;
        o->choice = (int32_t *)p;
    }
    return n_seq + 3 * r8 + 7 * r4 + n_x + c4;
}
struct irs_look_expand_args { // irs_lookahead_expand's arguments as the kernel takes them
    const int64_t *seq;  // [M][L] parent windows
    const int32_t *hep;  // [M]
    const int64_t *user; // [M] or null
    int M, L, k, k_c;
    const float *val;    // [M][k] the parents' ranked lists
    const int64_t *ids0; // [M][k]
    const int32_t *fin;  // [M] or null: != 0 expands to no candidate
    const int32_t *step_ptr; // device step counter, or step_arg
    int step_arg;
    irs_excl ex;         // bound exclusions (zero: none)
    int64_t *c_seq, *c_user, *c_tgt0, *c_ids0;
    int32_t *c_hep;
    float *c_val;
};
struct irs_look_choose_args { // irs_lookahead_choose's arguments as the kernel takes them
    const int64_t *seq;  // [M][L] parent windows (the target in slot L - 1)
    int M, L, k, k_c;
    const int64_t *c_ids0; // [M][k_c]
    const float *c_val, *mx, *sm, *ts; // [M][k_c]
    const int32_t *fin;  // [M] or null: != 0 leaves the list alone
    float *val;          // [M][k] in / out
    int64_t *ids0;       // [M][k] in / out
    float *lp;           // [M][k_c]
    int32_t *choice;     // [M]
    int32_t *rec_item;   // [users][ld][k_c] or null
    float *rec_lp;       // [users][ld][k_c] or null
    int rec_ld;
    const int32_t *rec_map, *rec_step; // row -> the caller's row (null: the identity); the device step counter
};
struct irs_eval_batch_args { // irs_build_eval_batch's arguments as the kernel takes them
    const int64_t *items, *offsets;
    int B, L, raw_len, gap_len;
    int64_t n_item;
    const int64_t *targets_in, *pool;
    int64_t n_pool;
    unsigned long long seed;
    int64_t *seq, *target, *label, *raw;
    int32_t *raw_n, *status;
};

// ---- a bound offer set (irs_bind_offer_set; offer_set.hip).  The caller's scratch holds a header whose int32 word 0 is the number
// of holes the prepare launch found, the sanitised ids padded with -1 to whole tiles of the score kernel, and the float32 scores
// of one pass: `rows` rows x c_pad.
#define IRS_OFFER_TILE 64
#define IRS_OFFER_HDR 256
struct irs_offer_rows {
    int32_t *holes; // [1] entries of the caller's array that became -1
    int64_t *ids;   // [c_pad] 0-based ids, ascending where the caller's were; -1: a hole, and everything behind C
    float *sc;      // [rows][c_pad]
    int64_t c_pad;
};
static inline size_t irs_offer_layout(void *base, int64_t n_ids, int rows, irs_offer_rows *o) {
    const size_t c_pad = ((size_t)n_ids + IRS_OFFER_TILE - 1) / IRS_OFFER_TILE * IRS_OFFER_TILE;
    const size_t n_id = (c_pad * 8 + 255) / 256 * 256;
    if (o) {
        char *p = (char *)base;
        o->holes = (int32_t *)p, o->ids = (int64_t *)(p + IRS_OFFER_HDR), o->sc = (float *)(p + IRS_OFFER_HDR + n_id);
        o->c_pad = (int64_t)c_pad;
    }
    return IRS_OFFER_HDR + n_id + (size_t)rows * c_pad * 4;
}

// ---- search options: what a caller binds to a context for its search calls.  Every change goes through opts_changed
// (capi.hip), which drops the captured steps; which entry point admits which option is capi.hip's search_rules.
struct irs_search_opts {
    // exact candidates (irs_bind_survivor_scratch): the caller's scratch while bound; the single-device loops then run the
    // survivor pass between their top-k and their step, the sharded loops refuse
    struct {
        void *scratch;
        size_t bytes;
    } surv;

    // bound exclusions (irs_bind_exclusions): the prepared rows in the caller's scratch while bound; every step and loop entry
    // point then drops window + list (+ path under no_repeat), the sharded loops refuse
    struct {
        int on;              // a binding exists (a list, no_repeat, or both)
        const int32_t *cnt;  // [users] valid ids of a user's row
        const int64_t *rows; // [users][stride] ascending, INT64_MAX behind the valid ids
        int users, stride, no_repeat;
    } excl;

    // path trace (irs_bind_path_trace): the caller's three [users][ld] arrays and scratch while bound; the greedy loops then
    // run the target sweep before their step and the record kernel after it, the beam and the sharded loops refuse
    struct {
        int on;
        float *item, *target;
        int32_t *rank;
        int users, ld;
        void *scratch;
    } trace;

    // admissible rank (irs_bind_trace_admissible): the caller's fourth [users][ld] array of the bound path trace (its users and ld)
    // and scratch while bound; the greedy loops then run k_trace_rank_adm behind the target sweep.  Only ever on while trace.on
    struct {
        int on;
        int32_t *rank;
        void *scratch;
    } adm;

    // bound guide (irs_bind_guide): the Rec2Inf choice rule of the greedy path step -- among the first k_c admissible candidates,
    // the one nearest to the target in the bound feature table; the beam and the sharded entry points then refuse
    struct {
        int on;
        irs_guide g;
    } guide;

    // bound lookahead (irs_bind_lookahead): the model-based choice of the greedy loops -- among the first k_c admissible candidates,
    // the one under which the target's next-step log-probability is highest; the beam and the sharded entry points then refuse
    struct {
        int on, kc, users, ld;
        void *scratch;
        int32_t *rec_item; // [users][ld][kc] or null
        float *rec_lp;
    } look;

    // arrival rule (irs_set_arrival_rule): between the trace sweep and the path step, a live row whose target stands at rank
    // <= rank (0: clause off) or at log-probability >= lp (lp_on) is offered the target alone; needs a bound trace.  kind: which
    // rank the clause reads -- IRS_RANK_WINDOW the trace's, IRS_RANK_ADMISSIBLE the admissible one (needs adm.on)
    struct {
        int on, rank, lp_on;
        float lp;
        int kind;
    } arrive;

    // beam trace (irs_bind_beam_trace): the caller's three [users][W][ld] arrays and scratch while bound; the two beam loops then
    // run the target sweep before a linked beam step and the carry kernel after it, every other search entry point refuses
    struct {
        int on;
        float *item, *target;
        int32_t *rank;
        int users, W, ld;
        void *scratch;
    } btrace;

    // beam rule (irs_set_beam_rule): behind the trace sweep of the two beam loops, the ruled beam step offers the target to a beam
    // whose target stands at rank <= rank (0: clause off) or at log-probability >= lp (lp_on), and orders the candidates by
    // score + weight * lp_target(parent); needs a bound beam trace, every other search entry point refuses
    struct {
        int on, rank, lp_on;
        float lp, weight;
    } brule;

    // offer set (irs_bind_offer_set): the sanitised ids and the score pass in the caller's scratch (irs_offer_layout) while bound;
    // irs_score_topk_offer ranks inside it, and the single-device loops, irs_recommend, the survivor pass and the arrival rule read
    // "the set" where they read "the catalog"; the sharded loops refuse
    struct {
        int on;
        const int64_t *ids; // [n] (in the scratch)
        int64_t n;
        void *scratch;
        int rows;           // rows of a pass: what the scratch was sized for
    } offer;

    // sampler (irs_bind_sampler): between the arrival offer and the path step of the greedy loops, k_sampler_choose draws one of
    // the first top_k admissible candidates of a live row -- temperature, nucleus, a draw keyed by the caller's row and the step --
    // and rewrites the row's list to it alone; the loops are then called with sample = 0.  The records ([users][ld], each may be
    // null) take the draw, the chosen candidate's log-probability under the proposal and the support.  The beam and the sharded
    // entry points refuse, and so do a guide and a lookahead: one choice rule at a time
    struct {
        int on, top_k;
        float temperature, inv_t, top_p;
        float *rec_u, *rec_lq;
        int32_t *rec_support;
        int users, ld;
    } sampler;
};
// the candidates a step chooses among: a guided and a lookahead step among their k_c, a bound sampler among its top_k, a sampled
// step among sample_k, a beam step of width W among W
static inline int irs_opt_choices(const irs_search_opts &o, int W, int sample, int sample_k) {
    return W ? W : (o.guide.on ? o.guide.g.k_c : (o.look.on ? o.look.kc : (o.sampler.on ? o.sampler.top_k : (sample ? sample_k : 1))));
}
// some option puts a launch of its own between the ranking and the greedy step, or needs a step kernel of its own: the merged
// top-k + step kernel cannot run (the arrival rule needs a trace, which is in the list; an offer set's lists come from its own launcher)
static inline bool irs_opt_splits_step(const irs_search_opts &o) {
    return o.surv.scratch || o.excl.on || o.trace.on || o.guide.on || o.look.on || o.offer.on || o.sampler.on;
}

struct irs_ctx {
    irs_dims dims;
    irs_shard shard;
    int64_t n_local; // items in this shard
    int d_pad;       // d rounded up to 16/32/64/128/256
    int KS;          // d_pad / 16 (bf16 MFMA k-steps)
    int n_tiles;     // ceil(n_local / 32)
    int max_seqs;    // sequences per decode call
    int max_rows;    // scored rows per call
    int m_pad_max;   // max_rows rounded up to 32

    // bound weights (device)
    const float *item_emb, *user_emb, *pe, *um_w, *um_b, *proj_w, *proj_b;
    irs_layer_w layer[IRS_MAX_LAYERS];

    // derived weights (device, in the caller's arena)
    uint4 *wp;        // bf16 fragments [n_tiles][KS][64] x 16 B
    float *bias_pad;  // [n_tiles*32], -inf beyond n_local
    float *c_l;       // [n_layers][d] cross-attention constants
    float *wnorm_max; // [3] max_j max(||W_j||, ||bf16(W_j)||), max_j ||W_j - bf16(W_j)||, max_j |b_j| (k_prep_x)
    float *w_frag16;  // fragment-packed layer weights of the 16-token latency kernel (d = 128, F = 256), or null
    uint4 *w_x6;      // split-bf16 step streams of the fused layer kernel k_block_x6 ([n_layers - 1] x 768 KB), or null
    int use_x6;       // decoder GEMMs of the throughput path on split-bf16 MFMAs (IRS_DECODER_GEMM=x6|f32)
    bool h3_ok;       // finalisation's float16 range bound holds (else IRS_GEMM_H3 runs as IRS_GEMM_X6 and V stays float32)
    float h3_bound;   // the largest operand magnitude the bound weights allow (irs_h3_operand_bound)
    int use_seq;      // sequence-resident decoder for the d = 128 throughput shape: 0 off, 1 on, 2 auto (default: from 384 sequences up)
    bool seq_last;    // the last irs_decode took it
    int32_t route_last[IRS_ROUTE_FIELDS]; // the last irs_launch_decode's DecodeRoute, packed (irs_decoder_route_last)
    int route_n;      // fields in route_last: 0 before the first decode
    int use_attn_h3;  // throughput attention on split-float16 MFMAs over K / V planes written by the layer kernel (default on; IRS_ATTN_GEMM=f32 off)
    int lse_no_ring;  // IRS_LSE_RING=0: the register-fragment log-sum-exp kernel at <= 32 rows too (A/B measurements, tests)
    bool finalized;
    bool proj_stale;  // a training entry point ran since irs_finalize_weights: wp / wnorm_max may lag project.*

    // workspace (device, caller-owned)
    char *ws;
    size_t ws_bytes;
    // decoder activations
    float *act_x, *act_y, *act_qkv, *act_ao, *act_h, *act_ru;
    float *act_qkv_b1; // second q | k | v buffer of the single-sequence fused-attention path (<= 256 rows)
    float *act_xf, *act_yf; // fragment-major copies of x / y (residual inputs of the LN-fused GEMMs)
    // packed (pad-free) decode plan
    int32_t *tok_row;  // [max_seqs * L] packed index -> b*L + t
    int32_t *seq_cnt, *seq_off, *seq_qrow; // [max_seqs]
    int32_t *seq_padq; // [max_seqs] index within the packed sequence of the one pad token it may hold (pos), or -1
    int32_t *m_dev;    // [1] number of packed rows
    // plan of the sequence-resident layer kernel (decoder.hip: k_plan_seq; null unless the shape supports it)
    int32_t *tile_seq, *tile_idx;   // [16 max_seqs] grid half tile -> sequence (-1: none), its block index
    int32_t *seq_row0, *qrow_tile;  // [max_seqs] first K / V image row in its workgroup; tile-order row of the consumed token
    int32_t *n_wg_dev;              // [2] workgroups in use; the first half-live one (= [0] when there is none)
    // scoring
    uint4 *xb;          // packed bf16 rows [m_pad/32][KS][64] x 16 B
    float *eps;         // [m_pad]
    float *thr;         // [m_pad]
    float *gm;          // [m_pad / 4][n_groups <= IRS_MAX_GROUPS][4]
    unsigned int *cand_cnt; // [m_pad][IRS_CAND_BUCKETS]
    unsigned long long *cand; // [m_pad][IRS_CAND_CAP]
    float *lse_part;    // [lse_slots][m_pad][2]
    int lse_slots;
    float *ref_tmp;     // [m_pad]
    int thr_valid, thr_M, thr_k, thr_age, carry_period; // carried emission thresholds (irs_launch_topk)
    int use_dense;    // dense form of the swept top-k on small catalogs (irs_set_topk_dense): 0 never, 1 wherever eligible, 2 auto (default)
    bool dense_last;  // the last irs_launch_topk took it
    unsigned int *fb_count;        // [1] rows recorded for the cooperative exhaustive fallback
    int32_t *fb_list;              // [max_rows]
    unsigned long long *exh_keys;  // [EXH_FB_MAX][strips][k] per-strip lists (null on small shards)
    // path generation scratch
    float *xrows;       // [max_rows][d]
    float *top_val;     // [max_rows][max_k]
    int64_t *top_ids;   // [max_rows][max_k]
    int32_t *row_status;// [max_rows]
    int32_t *step_ctr;  // [2] current step, next step (hipGraph loops)
    int32_t *step_pair; // set around a decode launched by the merged small-batch path loop: the plan kernel copies
                        // step_pair[1] over step_pair[0]
    int32_t *pos_tmp;   // [max_seqs]
    // beam-search state: the two sides of the ping-pong, and of what irs_beam_search_until moves at a compaction (its map is
    // un_map[2], the scan's places and count un_dst / un_count / un_count_host below)
    irs_beam_state bm[2];
    irs_beam_side bm_side[2];
    float *lse_max, *lse_sum; // [max_rows]
    // stop-at-target search (irs_generate_paths_until): the live users' compacted state, ping-pong [2]
    int64_t *un_seq[2];  // [max_seqs][L]
    int64_t *un_user[2]; // [max_seqs]
    int32_t *un_hep[2];  // [max_seqs]
    int32_t *un_map[2];  // [max_seqs] compacted row -> the caller's row
    int32_t *un_fin;     // [max_seqs] the compacted row has chosen its target
    int32_t *un_dst;     // [max_seqs] row of a live user after the next compaction (-1: finished)
    int32_t *un_status;  // [max_seqs] status bits of the step just run, by compacted row
    float *un_stage;     // [max_seqs][IRS_MAX_PATH] chosen items by compacted row (column `step` is read, then scattered)
    int32_t *un_count;   // [1] live users
    int32_t un_count_host; // where the 4-byte copy of un_count lands
    // item-sharded loops (comm.hip)
    float *x_local;           // [max_seqs][d] this rank's decoded rows (the all-gather's send buffer)
    uint64_t *keys_send, *keys_recv; // [max_rows][max_k] packed per-shard lists
    float *lse_gmax;          // [max_rows] all-reduced row maxima
    float *ce_pairs;          // [world][2][max_rows] gathered per-shard (lse, label score) of irs_ce_forward_sharded
    int sh_nograph;           // a capture with the collectives inside failed: the sharded loops stay on stream launches
    int sh_overlap;           // irs_set_sharded_overlap: the greedy sharded loop runs two user micro-batches per step, collectives on sh_side
    hipStream_t sh_side;      // (created on first use)
    hipEvent_t sh_ev[8];

    // captured steps of the search loops (irs_replay_steps): three independent caches, dropped together by irs_drop_graphs
    irs_step_graph g_greedy, g_beam, g_sharded;

    // what the caller has bound for the search entry points (irs_search_opts above), and the rows of the running search call
    // (its first step's): the layout of opt.surv.scratch that its later, smaller steps keep
    irs_search_opts opt;
    int surv_rows;

    // profiling
    int prof_family;
    irs_prof_ev *prof_ev;
    int prof_n, prof_cap;
    double prof_flops, prof_bytes;

    char err[512];
};

#define IRS_CHECK_HIP(ctx, expr)                                                                         \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess) {                                                                          \
            snprintf((ctx)->err, sizeof((ctx)->err), "%s:%d %s -> %s", __FILE__, __LINE__, #expr,        \
                     hipGetErrorString(_e));                                                             \
            return IRS_E_HIP;                                                                            \
        }                                                                                                \
    } while (0)

#define IRS_FAIL(ctx, code, ...)                                  \
    do {                                                          \
        snprintf((ctx)->err, sizeof((ctx)->err), __VA_ARGS__);    \
        return (code);                                            \
    } while (0)

// a user's trace and lookahead record end with its arrival: the until loop zeroes rows [0, B) of them, all ld columns, first
static inline int irs_opt_zero_records(irs_ctx *ctx, int B, hipStream_t s) {
    const irs_search_opts &o = ctx->opt;
    if (o.trace.on) {
        const size_t n = (size_t)B * o.trace.ld * 4;
        IRS_CHECK_HIP(ctx, hipMemsetAsync(o.trace.item, 0, n, s));
        IRS_CHECK_HIP(ctx, hipMemsetAsync(o.trace.target, 0, n, s));
        IRS_CHECK_HIP(ctx, hipMemsetAsync(o.trace.rank, 0, n, s));
        if (o.adm.on) IRS_CHECK_HIP(ctx, hipMemsetAsync(o.adm.rank, 0, n, s));
    }
    if (o.look.on && o.look.rec_item) {
        const size_t n = (size_t)B * o.look.ld * o.look.kc * 4;
        IRS_CHECK_HIP(ctx, hipMemsetAsync(o.look.rec_item, 0, n, s));
        IRS_CHECK_HIP(ctx, hipMemsetAsync(o.look.rec_lp, 0, n, s));
    }
    if (o.sampler.on) {
        const size_t n = (size_t)B * o.sampler.ld * 4;
        if (o.sampler.rec_u) IRS_CHECK_HIP(ctx, hipMemsetAsync(o.sampler.rec_u, 0, n, s));
        if (o.sampler.rec_lq) IRS_CHECK_HIP(ctx, hipMemsetAsync(o.sampler.rec_lq, 0, n, s));
        if (o.sampler.rec_support) IRS_CHECK_HIP(ctx, hipMemsetAsync(o.sampler.rec_support, 0, n, s));
    }
    return IRS_OK;
}

// profiling bracket helpers (no-ops unless the family is enabled)
void irs_prof_begin(irs_ctx *ctx, int family, hipStream_t s);
void irs_prof_end(irs_ctx *ctx, int family, hipStream_t s, double flops, double bytes);

// ---- captured steps, and what the four search entry points share (capi.hip)
// Replays the captured `body` `times` times on `s`; captures it first, on a private stream, unless `g` holds an equal key.  A
// failed capture leaves `g` empty and nothing has run: the return value is the body's own code (*capture_failed =
// IRS_CAPTURE_BODY) or IRS_E_HIP with HIP's message in ctx->err (IRS_CAPTURE_HIP).  A failed replay leaves *capture_failed 0.
enum { IRS_CAPTURE_BODY = 1, IRS_CAPTURE_HIP = 2 };
int irs_replay_steps(irs_ctx *ctx, irs_step_graph *g, const irs_step_key &key, const std::function<int(hipStream_t)> &body,
                     int times, hipStream_t s, int *capture_failed = nullptr);
void irs_drop_graphs(irs_ctx *ctx);
// which search entry point admits which bound option, in the order that entry point checks (capi.hip: search_rules); the
// sharded loops of comm.hip come here for theirs
int irs_sharded_option_rules(irs_ctx *ctx, const char *fn);
// the probability clause of an arrival rule is on for lp_min <= 0 (-inf included); lp_min > 0 and NaN turn it off
static inline bool irs_arrival_lp_on(float lp_min) { return lp_min <= 0.f; }
// event records are not captured: with a profiling family enabled every loop runs on the stream and records its brackets
static inline bool irs_may_capture(const irs_ctx *ctx, int use_graph) { return use_graph && ctx->prof_family == IRS_PROF_NONE; }
int irs_check_k(irs_ctx *ctx, const char *fn, int k, int world, int sweep, int sample, int sample_k);
int irs_check_beam_args(irs_ctx *ctx, const char *fn, bool ptrs_ok, int B, int W, int P); // ptrs_ok: no required pointer is null
int irs_ready_filter(irs_ctx *ctx, int sweep); // finalized, workspace bound, and no stale bf16 catalog under a filtering sweep
// beam step from ctx->bm[in] to ctx->bm[in ^ 1] on the lists in top_val / top_ids, then the step counter (until == nullptr: plain)
int irs_enqueue_beam_tail(irs_ctx *ctx, int in, const float *lse_max, const float *lse_sum, int B, int W, int k, int P, int32_t *status,
                          const irs_beam_until *until, hipStream_t s, const irs_excl *ex = nullptr);
int irs_search_begin(irs_ctx *ctx, int32_t *status, int B, hipStream_t s); // step counter and status to zero
int irs_beam_finish(irs_ctx *ctx, size_t rows, int P, float *paths, double *scores, int64_t *seq_final, hipStream_t s);

// ---- decode shapes: the workspace (capi.hip) and the decoder's route choice (decoder.hip: decode_route) must agree on them
// the sequence-resident layer kernel's shape (k_block_x6<.., SEQ>): its plan tables exist in the workspace only for it
static inline bool irs_seq_shape(const irs_dims &D) {
    return D.d == 128 && D.ffn_dim == 256 && D.n_heads == 4 && D.max_len <= 256 && D.n_layers > 1;
}
// a rows-only decode of B sequences is planned by ONE workgroup (k_plan_small), which also computes r_u and, around a decode of
// the merged path loop (ctx->step_pair), hands the step counter over
static inline bool irs_small_plan(const irs_dims &D, int B) { return B <= 64 && D.max_len >= 4; }

// ---- decoder.hip ----
int irs_launch_pif(irs_ctx *ctx, const int64_t *user, int B, float *r_u, hipStream_t s);
int irs_launch_decode(irs_ctx *ctx, const int64_t *seq, const int64_t *user, int B, float *x_out, const int32_t *pos,
                      float *xrows, float *r_u_out, hipStream_t s);
int irs_launch_cross_const(irs_ctx *ctx, hipStream_t s);
size_t irs_small_frag_floats(const irs_ctx *ctx);
int irs_launch_pack_small(irs_ctx *ctx, hipStream_t s);
size_t irs_x6_bytes(const irs_ctx *ctx);
int irs_launch_pack_x6(irs_ctx *ctx, hipStream_t s);
int irs_launch_h3_range(irs_ctx *ctx, float *stats, hipStream_t s);
float irs_h3_operand_bound(const irs_ctx *ctx, const float *stats);

// ---- score.hip ----
int irs_launch_pack_w(irs_ctx *ctx, hipStream_t s);
struct irs_path_args;
bool irs_topk_is_direct(const irs_ctx *ctx, int M, int k);
int irs_launch_topk(irs_ctx *ctx, const float *xrows, int M, int k, int sweep, float *val, int64_t *ids0,
                    int32_t *status, hipStream_t s, const irs_path_args *path = nullptr, float *lse_max = nullptr,
                    float *lse_sum = nullptr, int carry = 0);
int irs_launch_gather(irs_ctx *ctx, const float *xrows, int M, const int64_t *ids0, int g, float *out, hipStream_t s);
int irs_launch_count_before(irs_ctx *ctx, const float *xrows, int M, const float *ref_score, const int64_t *ref_id0,
                            const int64_t *excl, int n_excl, int64_t *count, hipStream_t s);
int irs_launch_dense(irs_ctx *ctx, const float *xrows, int M, float *out, int64_t ld, hipStream_t s);
int irs_launch_lse(irs_ctx *ctx, const float *xrows, int M, float *out_max, float *out_sum, hipStream_t s);
// the target sweep of the path trace: sc.count / sc.refid are its scratch, the four outputs go where the caller says
int irs_launch_target_trace(irs_ctx *ctx, const float *xrows, const int64_t *seq, const int32_t *hep, int M, const irs_trace_rows &sc,
                            float *out_max, float *out_sum, float *out_tscore, int32_t *out_rank, hipStream_t s);
// what irs_launch_target_trace runs behind its first launch (k_trace_target): the MODE_TRACE sweep against (out_tscore, sc.refid)
// with sc.count cleared, the partials' reduction and the window correction.  The replay pass enters here with its own first launch.
int irs_launch_trace_sweep(irs_ctx *ctx, const float *xrows, const int64_t *seq, const int32_t *hep, int M, const irs_trace_rows &sc,
                           float *out_max, float *out_sum, float *out_tscore, int32_t *out_rank, hipStream_t s);
int irs_launch_refresh_bias(irs_ctx *ctx, hipStream_t s);
int irs_launch_lse_combine(irs_ctx *ctx, const float *mx, const float *sm, float *lse, int M, hipStream_t s);
int irs_launch_ce_reduce(irs_ctx *ctx, const float *lse, const float *lab_score, const int64_t *labels0, int M, double *out,
                         hipStream_t s);
int irs_launch_ce_grad(irs_ctx *ctx, const float *xrows, const int64_t *labels0, const float *lse, int M, float scale,
                       float *out, int64_t ld, hipStream_t s);

// ---- ce_backward.hip ---- (the fused backward over this context's shard; arguments already validated)
size_t irs_ce_bwd_scratch(const irs_ctx *ctx, int M);
int irs_launch_ce_backward(irs_ctx *ctx, const float *xrows, const int64_t *labels0, const float *lse, int M, float scale,
                           int accumulate, float *dx, float *dw, float *db, void *scratch, hipStream_t s);

// ---- survivors.hip ---- (exact candidates for rows whose window hides their top-k; arguments already validated)
struct irs_surv_args {
    const float *xrows;  // [M][d]
    const int64_t *seq;  // [M][L]
    const int32_t *hep;  // [M]
    int M, rps, k, want; // rps: rows per status word
    int rows_cap;        // rows the scratch was sized for (>= M): irs_surv_scratch(rows_cap, want) bytes
    const double *cum;   // [M] or null: -inf skips the row
    const int32_t *fin;  // [M] or null: != 0 skips the row
    const int32_t *done; // [M / rps] or null: != 0 skips the user's rows
    float *val;          // [M][k] in / out
    int64_t *ids0;       // [M][k] in / out
    int32_t *status;     // IRS_ROW_RESCUED goes to status[u], u = row / rps, or to status[status_map[u]]
    const int32_t *status_map;
    irs_excl ex;         // bound exclusions (zero: none)
};
size_t irs_excl_scratch(int users, int n_excl);
int irs_launch_excl_prepare(irs_ctx *ctx, const int64_t *ids0, int users, int n_excl, void *scratch, hipStream_t s);
size_t irs_surv_scratch(const irs_ctx *ctx, int rows, int want);
int irs_launch_survivors(irs_ctx *ctx, const irs_surv_args &a, void *scratch, hipStream_t s);

// ---- offer_set.hip ---- (arguments already validated; irs_launch_offer_topk reads ctx->opt.offer)
int irs_launch_offer_prepare(irs_ctx *ctx, const int64_t *ids0, int64_t n_ids, const irs_offer_rows &o, hipStream_t s);
int irs_launch_offer_topk(irs_ctx *ctx, const float *xrows, int M, int k, float *val, int64_t *ids0, int32_t *status, hipStream_t s);
// the score pass alone: o.sc[r][*] for `rows` rows (at most what the scratch holds) of x; irs_launch_offer_topk's first launch
int irs_launch_offer_scores(irs_ctx *ctx, const float *x, int rows, const irs_offer_rows &o, hipStream_t s);

// ---- admissible.hip ---- (arguments already validated)
int irs_launch_trace_rank_adm(irs_ctx *ctx, const irs_adm_args &a, hipStream_t s);

// ---- recommend.hip ---- (the first n admissible entries of every row's list; arguments already validated.  seq null: no window;
// out_lp null: mx / sm are not read; ex: the bound exclusion lists, never a path)
int irs_launch_recommend_take(irs_ctx *ctx, const int64_t *seq, const int32_t *hep, int M, const float *val, const int64_t *ids0, int k,
                              const float *mx, const float *sm, int n, float *out_val, int64_t *out_ids0, float *out_lp,
                              int32_t *out_count, const irs_excl &ex, hipStream_t s);

// ---- comm.hip ---- (collectives in bytes, stream-ordered; irs_comm_check: the communicator is the context's shard)
int irs_comm_check(irs_ctx *ctx, const irs_comm *c, const char *fn);
int irs_comm_allgather(irs_ctx *ctx, irs_comm *c, const void *send, void *recv, size_t bytes_per_rank, hipStream_t s);
int irs_comm_alltoall(irs_ctx *ctx, irs_comm *c, const void *send, void *recv, size_t bytes_per_rank, hipStream_t s);

// ---- path.hip ----
int irs_launch_merge(irs_ctx *ctx, const float *val_in, const int64_t *ids_in, int W, int M, int k, float *val,
                     int64_t *ids0, hipStream_t s);
int irs_launch_merge_keys(irs_ctx *ctx, const uint64_t *keys_in, int W, int M, int k, float *val, int64_t *ids0, hipStream_t s);
int irs_launch_pack_topk(irs_ctx *ctx, const float *val, const int64_t *ids0, int64_t n, uint64_t *keys, hipStream_t s);
int irs_launch_path_step(irs_ctx *ctx, const irs_path_args &pa, int B, const float *val, const int64_t *ids0, int k, hipStream_t s);
int irs_launch_inc(irs_ctx *ctx, int32_t *ctr, hipStream_t s);
// the arrival rule on B rows, behind the trace sweep (mx / sm / ts / rank by launch row) and before the path step: a row that
// fires gets (ts, t - 1), (-inf, -1) at the head of its list and IRS_ROW_OFFERED in status[row]; rows with fin[r] != 0 (null:
// none) are skipped.  `ex`: the step's bound exclusions (its map, its path rows and its step index: ex.step_ptr / ex.step_arg)
int irs_launch_arrival_offer(irs_ctx *ctx, const int64_t *seq, const int32_t *hep, int B, const float *mx, const float *sm,
                             const float *ts, const int32_t *rank, const int32_t *fin, float *val, int64_t *ids0, int k, int rank_max,
                             float lp_min, int32_t *status, const irs_excl &ex, hipStream_t s);
// after a path step on B rows, before the step counter moves: the three traced values of step step_ptr[0] go to row map[r] (null: r)
// of the caller's arrays; rows with fin[r] != 0 (null: none) are not written
int irs_launch_trace_record(irs_ctx *ctx, const irs_trace_rec &t, const int64_t *seq, const int32_t *hep, const float *paths,
                            int path_ld, const int32_t *step_ptr, const int32_t *map, const int32_t *fin, const float *val,
                            const int64_t *ids0, int k, int B, hipStream_t s);
// the stop-at-target loop's own kernels (irs_generate_paths_until, capi.hip); map == nullptr is the identity
int irs_launch_until_record(irs_ctx *ctx, const float *stage, int P, int step, const int32_t *map, const int64_t *seq, int B,
                            int32_t *fin, int32_t *step_status, float *paths, int32_t *status, hipStream_t s);
int irs_launch_until_scan(irs_ctx *ctx, const int32_t *fin, int B, int32_t *dst, int32_t *count, hipStream_t s);
int irs_launch_until_gather(irs_ctx *ctx, const int32_t *dst, int B, const int64_t *seq, const int64_t *user, const int32_t *hep,
                            const int32_t *map, int64_t *seq_out, int64_t *user_out, int32_t *hep_out, int32_t *map_out,
                            hipStream_t s);
int irs_launch_set_step(irs_ctx *ctx, int32_t *step_pair, int step, hipStream_t s);
int irs_launch_beam_init(irs_ctx *ctx, const int64_t *seq0, const int64_t *user0, const int32_t *hep0, int B, int W, int P,
                         const irs_beam_state &st, int64_t *user, hipStream_t s);
// until == nullptr: the plain step (fin is not touched); else the step of irs_beam_step_until / irs_beam_search_until
// link != nullptr: the linked form of either, which also writes link->link / link->val (irs_beam_link)
// rule != nullptr (with a link): the ruled form of the linked step (irs_beam_rule)
int irs_launch_beam_step(irs_ctx *ctx, const irs_beam_state &in, const irs_beam_state &out, const irs_beam_cand &cand, int B, int W,
                         int step, const int32_t *step_ptr, int P, int32_t *status, const irs_beam_until *until, hipStream_t s,
                         const irs_beam_link *link = nullptr, const irs_beam_rule *rule = nullptr);

// ---- beam_trace.hip ---- (arguments already validated: 1 <= W <= 32, 1 <= ld <= IRS_MAX_PATH)
int irs_launch_beam_trace_carry(irs_ctx *ctx, const irs_beam_carry_args &a, int B, hipStream_t s);
// dst == nullptr sends every user to the caller's outputs (out / side_out are then not touched)
int irs_launch_beam_retire(irs_ctx *ctx, const int32_t *dst, int B, int W, int P, const irs_beam_state &in,
                           const irs_beam_side &side_in, const irs_beam_state &out, const irs_beam_side &side_out,
                           const irs_beam_out &res, hipStream_t s);

int irs_launch_build_eval_batch(irs_ctx *ctx, const irs_eval_batch_args &a, hipStream_t s);

// ---- guide.hip ---- (the Rec2Inf choice rule; arguments already validated)
size_t irs_guide_scratch(int64_t n_item, int kind, int F);
int irs_launch_guide_pack(irs_ctx *ctx, const uint8_t *table, int64_t rows, int F, uint32_t *packed, hipStream_t s);
// the path step while a guide is bound (irs_launch_path_step chooses it)
int irs_launch_path_step_guided(irs_ctx *ctx, const irs_path_args &pa, int B, const float *val, const int64_t *ids0, int k,
                                hipStream_t s);

// ---- lookahead.hip ---- (the one-step lookahead choice; arguments already validated)
int irs_launch_lookahead_expand(irs_ctx *ctx, const irs_look_expand_args &a, hipStream_t s);
int irs_launch_lookahead_choose(irs_ctx *ctx, const irs_look_choose_args &a, hipStream_t s);

// ---- sampler.hip ---- (the bound sampler's choice; arguments already validated)
struct irs_sampler_args { // irs_sampler_choose's arguments as the kernel takes them
    const int64_t *seq;      // [M][L]
    const int32_t *hep;      // [M]
    int M, L, k, top_k;
    float inv_t, top_p;
    float *val;              // [M][k] in / out
    int64_t *ids0;           // [M][k] in / out
    const int32_t *fin;      // [M] or null: != 0 leaves the row alone
    const int32_t *status;   // [M] the step's status words: IRS_ROW_OFFERED marks a row the arrival rule has chosen for
    const int32_t *row_ids;  // [M] row -> the caller's row (null: the identity): keys the draw, and the records' row
    const int32_t *step_ptr; // device step counter, or step_arg
    int step_arg;
    unsigned long long seed;
    float *rec_u, *rec_lq;   // [rec_users][rec_ld] or null
    int32_t *rec_support;
    int rec_users, rec_ld;
    irs_excl ex;             // bound exclusions (zero: none)
};
int irs_launch_sampler_choose(irs_ctx *ctx, const irs_sampler_args &a, hipStream_t s);

// ---- replay.hip ---- (path replay: irs_replay_windows / irs_replay_paths; arguments already validated)
struct irs_replay_args { // the builder's arguments as the kernel takes them; the rows are [0, R) of row_user / row_step and of the outputs
    int layout, B, L, P, path_ld, R;
    int64_t n_item;
    const int64_t *seq0;  // [B][L]
    const int32_t *hep0;  // [B] (SLOT)
    const int64_t *user;  // [B] or null
    const int64_t *target;// [B] (FULL; only read for target_out)
    const int64_t *paths; // [B][path_ld]
    const int32_t *row_user, *row_step;
    int64_t *seq_out;     // [R][L]
    int32_t *hep_out;     // [R]
    int64_t *user_out;    // [R] or null
    int32_t *status;      // [R]
    int64_t *item_out, *target_out; // [R] or null: the forced item (0: none) and the target (0: invalid row) of the replay pass
};
// the scratch of one pass of `chunk` rows, every array rounded up to 256 bytes; the trace rows last (irs_trace_layout)
struct irs_replay_rows {
    int64_t *seq, *user, *item, *target;
    int32_t *hep;
    float *iscore, *x;
    irs_trace_rows tr;
};
static inline size_t irs_replay_layout(void *base, int chunk, int L, int d, irs_replay_rows *o) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t n_seq = up((size_t)chunk * L * 8), r8 = up((size_t)chunk * 8), r4 = up((size_t)chunk * 4), n_x = up((size_t)chunk * d * 4);
    const size_t head = n_seq + 3 * r8 + 2 * r4 + n_x;
    if (o) {
        char *p = (char *)base;
        o->seq = (int64_t *)p, o->user = (int64_t *)(p + n_seq), o->item = (int64_t *)(p + n_seq + r8);
        o->target = (int64_t *)(p + n_seq + 2 * r8);
        o->hep = (int32_t *)(p + n_seq + 3 * r8), o->iscore = (float *)(p + n_seq + 3 * r8 + r4);
        o->x = (float *)(p + n_seq + 3 * r8 + 2 * r4);
        irs_trace_layout(p + head, chunk, &o->tr);
    }
    return head + irs_trace_layout(nullptr, chunk, nullptr);
}
int irs_launch_replay_windows(irs_ctx *ctx, const irs_replay_args &a, hipStream_t s);
// one pass behind the decode: scores of target and forced item, the trace sweep, the record into rows [0, M) of the caller's arrays
int irs_launch_replay_score(irs_ctx *ctx, const irs_replay_rows &sc, int M, const int32_t *status, float *lp_item, float *lp_target,
                            int32_t *rank, hipStream_t s);

// ---- small device helpers ----
#ifdef __HIPCC__
// float -> unsigned key whose unsigned order equals float order; -0 folded onto +0
// (identical to fkey() in oracle/oracle_score.c).
__device__ __forceinline__ unsigned int irs_fkey(float f) {
    unsigned int u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float irs_unkey(unsigned int k) {
    unsigned int u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    return __uint_as_float(u);
}
// exact score: k-ascending float32 fma chain seeded with the bias.  The chain itself is serial; the LOADS of the item
// row are not: they are requested eight float4 at a time ahead of the fmas that consume them (with one load per
// loop trip a 128-float row cost 32 dependent memory round trips -- most of k_refine's time).
__device__ __forceinline__ float irs_chain(const float *__restrict__ x, const float *__restrict__ w, float b, int d) {
    float acc = b;
    if ((d & 3) == 0 && ((((uintptr_t)w) & 15) == 0)) {
        const float4 *w4 = reinterpret_cast<const float4 *>(w);
        const int n4 = d >> 2;
        int k = 0;
        for (; k + 8 <= n4; k += 8) {
            float4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = w4[k + j];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc = __fmaf_rn(x[4 * (k + j) + 0], v[j].x, acc);
                acc = __fmaf_rn(x[4 * (k + j) + 1], v[j].y, acc);
                acc = __fmaf_rn(x[4 * (k + j) + 2], v[j].z, acc);
                acc = __fmaf_rn(x[4 * (k + j) + 3], v[j].w, acc);
            }
        }
        for (; k < n4; ++k) {
            float4 v = w4[k];
            acc = __fmaf_rn(x[4 * k + 0], v.x, acc);
            acc = __fmaf_rn(x[4 * k + 1], v.y, acc);
            acc = __fmaf_rn(x[4 * k + 2], v.z, acc);
            acc = __fmaf_rn(x[4 * k + 3], v.w, acc);
        }
    } else {
        for (int k = 0; k < d; ++k) acc = __fmaf_rn(x[k], w[k], acc);
    }
    return acc;
}

// ---- one row of the persuasion-path step (reference model/influentialRS.py:419-450), executed by one wave:
// window filter of the ranked candidates, greedy / sampled choice, path record, window grow / shift.
struct irs_path_args {
    int64_t *seq;
    int32_t *hep;
    int L;
    float *paths;
    int path_ld, sample, sample_k;
    unsigned long long seed;
    int32_t *status;
    const int32_t *step_ptr;
    int step_arg;
    int32_t *step_next;
    int enabled;
    irs_excl ex; // bound exclusions (zero: none)
};

// ---- membership in a bound exclusion set: the ONE test of the path step, the beam steps and the survivor pass.
// A wave opens its row's view once: the user's sorted list, and (no_repeat) path entry `lane` of the row as an item, -1 for
// none.  irs_excl_listed is the per-lane half: a binary search of one 0-based id in the sorted list (<= 13 probes at 4096
// ids); the callers ballot it over the 64 candidates of a round.  The per-wave half is `view.pth == item`, OR-ed into the
// window compare that the callers already reduce with __any.
struct irs_excl_view {
    const int64_t *list;
    int n;
    int64_t pth;
};
__device__ __forceinline__ bool irs_excl_listed(const int64_t *__restrict__ list, int n, int64_t id0) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < id0) lo = mid + 1;
        else hi = mid;
    }
    return id0 >= 0 && lo < n && list[lo] == id0;
}
__device__ __forceinline__ int irs_excl_user(const irs_excl &ex, int row) {
    const int slot = row / ex.div;
    return ex.map ? ex.map[slot] : slot;
}
__device__ __forceinline__ irs_excl_view irs_excl_open(const irs_excl &ex, int row, int lane, int step) {
    const int user = irs_excl_user(ex, row);
    irs_excl_view v;
    v.list = ex.rows ? ex.rows + (size_t)user * ex.stride : nullptr;
    v.n = ex.rows ? ex.cnt[user] : 0;
    v.pth = -1;
    if (ex.paths && lane < step && lane < ex.path_ld) {
        const float f = ex.paths[(size_t)(ex.path_by_user ? user : row) * ex.path_ld + lane];
        if (f != 0.f) v.pth = (int64_t)f;
    }
    return v;
}

// ---- the register image of a window: the ONE membership test of the path step, the beam steps and the survivor flag pass.
// A wave holds window slot lane + 64 i in register i of every lane (-1 beyond the window's last live slot), so "is this item in the
// window" is SLOTS compares per lane and one __any.  SLOTS = 4 serves contexts with max_len <= 256, SLOTS = 16 the long windows
// of irs_create_ex (max_len <= IRS_MAX_LEN_LONG); the launchers choose by ctx->dims.max_len (irs_window_slots).
#define IRS_WIN_SLOTS_SHORT 4
#define IRS_WIN_SLOTS_LONG (IRS_MAX_LEN_LONG / 64)
static inline int irs_window_slots(const irs_ctx *ctx) { return ctx->dims.max_len > 256 ? IRS_WIN_SLOTS_LONG : IRS_WIN_SLOTS_SHORT; }
template <int SLOTS>
struct irs_window {
    int64_t v[SLOTS];
    // he: the window's last live slot (the window is w[0 .. he])
    __device__ __forceinline__ void load(const int64_t *w, int he, int L, int lane) {
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            int p = lane + 64 * i;
            v[i] = (p < he + 1 && p < L) ? w[p] : (int64_t)-1;
        }
    }
    // this lane's part of the test, OR-ed onto the caller's own terms (`hit`); the callers reduce with __any
    __device__ __forceinline__ bool holds(int64_t item, bool hit = false) const {
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) hit |= (v[i] == item);
        return hit;
    }
};

// EXCL: the form with a bound exclusion set (p_.ex.on); without it the body is the one the library always had.
// SLOTS: the window image's registers per lane (irs_window).
template <bool EXCL = false, int SLOTS = IRS_WIN_SLOTS_SHORT>
__device__ __forceinline__ void irs_path_step_row(const irs_path_args &p_, int row, int lane, const float *__restrict__ val,
                                                  const int64_t *__restrict__ ids0, int k) {
    const int L = p_.L, path_ld = p_.path_ld, sample = p_.sample;
    int sample_k = p_.sample_k;
    const unsigned long long seed = p_.seed;
    int64_t *seq = p_.seq;
    int32_t *hep = p_.hep, *status = p_.status, *step_next = p_.step_next;
    float *paths = p_.paths;
    const int step = p_.step_ptr ? p_.step_ptr[0] : p_.step_arg;
    // merged small-batch loop: publish the next step index in a second word (nobody reads it during this kernel;
    // the next step's first kernel copies it over step_ptr[0]) instead of a k_inc launch
    if (step_next && row == 0 && lane == 0) step_next[0] = step + 1;
    int64_t *w = seq + (size_t)row * L;
    const int he = hep[row];
    // window = seq[row, 0 .. he], into registers (L <= 64 SLOTS)
    irs_window<SLOTS> win;
    win.load(w, he, L, lane);
    int64_t chosen = 0;
    int found = 0;
    float surv_val[IRS_MAX_SAMPLE_K];
    int64_t surv_id[IRS_MAX_SAMPLE_K];
    if (sample_k > IRS_MAX_SAMPLE_K) sample_k = IRS_MAX_SAMPLE_K; // the entry points reject larger values
    const int want = sample ? sample_k : 1;
    if constexpr (EXCL) { // 64 candidates per round, one per lane: each lane searches its own in the user's list, one ballot
        const irs_excl_view ev = irs_excl_open(p_.ex, row, lane, step);
        bool more = true;
        for (int c0 = 0; c0 < k && found < want && more; c0 += 64) {
            const int cl = c0 + lane;
            const int64_t cid = cl < k ? ids0[(size_t)row * k + cl] : (int64_t)-1;
            const unsigned long long listed = __ballot(irs_excl_listed(ev.list, ev.n, cid));
            for (int c = 0; c < 64 && c0 + c < k && found < want; ++c) {
                const int64_t id0 = __shfl(cid, c, 64);
                if (id0 < 0) {
                    more = false;
                    break;
                }
                const int64_t item = id0 + 1;
                const bool hit = win.holds(item, ev.pth == item);
                if (!__any(hit) && !((listed >> c) & 1ull)) {
                    surv_val[found] = val[(size_t)row * k + c0 + c];
                    surv_id[found] = item;
                    ++found;
                }
            }
        }
    } else {
        for (int c = 0; c < k && found < want; ++c) {
            int64_t id0 = ids0[(size_t)row * k + c];
            if (id0 < 0) break;
            int64_t item = id0 + 1;
            if (!__any(win.holds(item))) {
                surv_val[found] = val[(size_t)row * k + c];
                surv_id[found] = item;
                ++found;
            }
        }
    }
    if (found == 0) {
        if (lane == 0) status[row] |= IRS_ROW_NO_CANDIDATE;
        chosen = 0;
    } else if (!sample) {
        chosen = surv_id[0];
    } else {
        // multinomial over the first `found` survivors with weights exp(val) (softmax's
        // normaliser cancels, influentialRS.py:431-434).  Counter RNG: splitmix64(seed, row, step).
        unsigned long long z = seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)row * 1315423911ull + (unsigned long long)step + 1ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        float u = (float)((z >> 40) & 0xFFFFFF) * (1.0f / 16777216.0f);
        float mx = surv_val[0], tot = 0.f, p[IRS_MAX_SAMPLE_K];
        for (int i = 0; i < found; ++i) {
            p[i] = __expf(surv_val[i] - mx);
            tot += p[i];
        }
        float acc = 0.f;
        chosen = surv_id[found - 1];
        for (int i = 0; i < found; ++i) {
            acc += p[i] / tot;
            if (u < acc) {
                chosen = surv_id[i];
                break;
            }
        }
    }
    if (lane == 0 && step < path_ld) paths[(size_t)row * path_ld + step] = (float)chosen;
    if (found == 0) return;
    if (he < L - 2) { // room before the target: grow (influentialRS.py:438-441)
        if (lane == 0) {
            w[he + 1] = chosen;
            hep[row] = he + 1;
        }
    } else { // shift left by one, keep the target last (influentialRS.py:442-450)
        int64_t nv[SLOTS];
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            int p = lane + 64 * i;
            nv[i] = (p + 1 <= L - 2) ? w[p + 1] : 0;
        }
        // all loads of this wave are complete before the stores (single wave, in-order memory ops per lane;
        // cross-lane overlap p <-> p+1 needs the explicit fence below)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            int p = lane + 64 * i;
            if (p < L - 2) w[p] = nv[i];
        }
        if (lane == 0) w[L - 2] = chosen;
    }
}

// ---- cross-lane all-reductions without the LDS crossbar.  hipcc lowers every __shfl_xor to ds_bpermute_b32 (an
// LDS-pipe round trip, awaited at once when the next step depends on it); the latency kernels run chains of them.
// Here: DPP for the steps inside a 16-lane row (quad_perm for xor 1 / 2, row_ror:8 for xor 8; row_half_mirror reaches
// the other quad, so level 4 needs the quads to agree already -- true after levels 1 and 2, or when the data is
// uniform per quad), gfx950's v_permlane16_swap / v_permlane32_swap for the steps across rows.  STEPS says which of
// the six butterfly levels run (bit i = level 2^i).  Every lane of a reduced group ends with the same bits.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __uint_as_float((unsigned int)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), CTRL, 0xF, 0xF, true));
}
struct OpSum {
    __device__ __forceinline__ float operator()(float a, float b) const { return a + b; }
};
struct OpMax {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
template <int STEPS, typename OP>
__device__ __forceinline__ float lanes_reduce(float v, OP op) {
    if (STEPS & 1) v = op(v, dpp_f32<0xB1>(v));  // quad_perm [1,0,3,2]
    if (STEPS & 2) v = op(v, dpp_f32<0x4E>(v));  // quad_perm [2,3,0,1]
    if (STEPS & 4) v = op(v, dpp_f32<0x141>(v)); // row_half_mirror
    if (STEPS & 8) v = op(v, dpp_f32<0x128>(v)); // row_ror:8 = lane ^ 8 inside the row, no agreement needed
    if (STEPS & 16) {
        const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = op(__uint_as_float(a[0]), __uint_as_float(a[1]));
    }
    if (STEPS & 32) {
        const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = op(__uint_as_float(b[0]), __uint_as_float(b[1]));
    }
    return v;
}
template <int STEPS>
__device__ __forceinline__ float lanes_sum(float v) { return lanes_reduce<STEPS>(v, OpSum()); }
template <int STEPS>
__device__ __forceinline__ float lanes_max(float v) { return lanes_reduce<STEPS>(v, OpMax()); }


#endif
