// hwbrj_engine.h -- host-side orchestration of the MI355X join pipeline (internal C++).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <deque>
#include <string>
#include <vector>

#include "../../include/hwbrj.h"
#include "hwbrj_common.h"
#include "hwbrj_kernels.h"

namespace hwbrj {

// Picks mode / partitioning / slice geometry for a filter configuration (DESIGN.md "Modes").
// Returns false (and sets *err) for configurations outside the reference's contract.
// mat: the materializing pipeline's geometry (join jobs sized for its hash
// table, k_join_mat).
bool plan_geometry(const bloom_filter_args_t* args, uint64_t nR, Geometry* g, std::string* err,
                   bool mat = false);

constexpr int kRcMatGlobal = 11;  // a payload join in the global-bitmap mode: use the side pass (Engine::side)

// The validity bitmaps of two key columns (layout SRC_KEYS; include/hwbrj.h "validity bitmaps"): row
// i of a column is bit i & 7 of byte i >> 3, set = valid; nullptr: that column has no NULL keys and
// runs the kernels it runs without a KeyMasks. A NULL key joins nothing. Partition-slice modes and no
// filter only (9 otherwise).
// sv: the group joins on key columns only (JoinReq::s_val), the bitmap of S's value column in the
// same layout: an S row takes part iff its key bit and its value bit are set, so count is COUNT(S.val)
// and sum / min / max are over the same rows. Under GROUP_ALL a NULL R row still gets its identity row.
struct KeyMasks {
    const uint8_t* r  = nullptr;
    const uint8_t* s  = nullptr;
    const uint8_t* sv = nullptr;
};

// One join of device-resident relations: what it produces (kind), where, and how its inputs are read.
//  COUNT: matches only. PAIRS: {R.payload, S.payload} of every match. SEMI: whole S tuples {key,
//  payload}, those with a partner in R or (anti) those without. OUTER: rows {R.payload | null_pay,
//  S.payload | null_pay}; keep_s: the S rows without a partner are rows too, keep_r: the R rows.
//  GROUP: rows {R.payload, count, sum} (hwbrj_group_row_t, 16 bytes) or, agg = GRP_COUNT_MINMAX,
//  {R.payload, count, min, max} (hwbrj_group_minmax_row_t); all: every R row, else those with count > 0.
// Rows go to out[0, cap) (uint2, GROUP: uint4); the counts also count the rows beyond cap.
// Every kind but COUNT runs the payload-carrying pipeline (the materializing geometry, S payloads
// beside the partition words); SEMI's R side is the counting join's (32-bit codes, no payloads), the
// others carry R's payloads too and differ from the join kernel on.
// jkind: the per-partition join of COUNT (JoinParams::jkind: 0 PRO, 1 PRH, 2 PRHO).
// layout: what dR and dS both point to: SRC_TUPLES (uint2 {key, payload}) or SRC_KEYS (one uint32 key
// per element, 16-byte aligned; every payload is the row index, |R|, |S| < 2^31). Only the kernels
// that read the relations differ; the partition words and payloads, and so everything from the pools
// on, do not depend on it. s_val: GROUP on key columns, S's value column (|S| uint32 beside its keys):
// the payloads that are aggregated, read by the S payload scatter as SRC_KEYS_VAL.
// masks: validity bitmaps (KeyMasks, SRC_KEYS only). A side with a bitmap runs the SRC_KEYS_MASK
// scatter (GROUP's S side SRC_KEYS_VAL_MASK, with one bitmap or two), the other side the kernel it
// runs without; nothing after the scatters knows: a NULL key is in no partition. The rows NULL keys
// contribute themselves (anti, outer, GROUP all) come from k_null_rows / k_null_group_rows after the
// kind's own emit kernels, through the same row counter.
// rmark: the marking probes of a prepared build (OUTER, keep_r off): every R row with a partner sets
// its bit there (k_join_outer_mark), and no R-only row is written.
// gacc: the accumulating group probe of a prepared build (GROUP, all off): the build's accumulators
// of form agg, one entry per R row; every R row with a partner folds its count and aggregate into
// its entry (k_join_group_acc), and no row is written (out and cap are not read).
enum JoinKind : int { JOIN_COUNT = 0, JOIN_PAIRS, JOIN_SEMI, JOIN_OUTER, JOIN_GROUP };
struct JoinReq {
    JoinKind    kind = JOIN_COUNT;
    void*       out  = nullptr;
    uint64_t    cap  = 0;
    bool        anti = false;                      // SEMI
    bool        keep_s = false, keep_r = false;    // OUTER
    uint32_t    null_pay = 0;
    bool        all   = false;                     // GROUP
    uint32_t    agg   = GRP_COUNT_SUM;
    const void* s_val = nullptr;
    int         jkind = 0, layout = SRC_TUPLES;
    KeyMasks    masks;
    uint32_t*   rmark = nullptr;  // OUTER on a prepared build: the build's marks (the marking probes)
    uint4*      gacc  = nullptr;  // GROUP on a prepared build: the build's accumulators (the accumulating probe)
    bool carries_s_payloads() const { return kind != JOIN_COUNT; }
    bool carries_r_payloads() const { return kind == JOIN_PAIRS || kind == JOIN_OUTER || kind == JOIN_GROUP; }
};
// The relations of a join, its filter (nullptr: none) and its stream (nullptr: the Engine's own)
struct JoinIn {
    const void*                dR;
    uint64_t                   nR;
    const void*                dS;
    uint64_t                   nS;
    const bloom_filter_args_t* args;
    hipStream_t                stream;
};
// What a kind counts beside its rows: OUTER cls = {inner, S-only, R-only} rows; GROUP pairs = the sum
// of the rows' counts
struct JoinExtras {
    uint64_t cls[3] = {0, 0, 0};
    uint64_t pairs  = 0;
};

// The derived sizes of one join, computed in one place (JoinShape::make) for both enqueue paths and
// kept for the table readback: F partitions of NSUB subs (NJ join jobs), nseg slice segments, CH
// chunks per probe item; G scatter workgroups whose regions hold capR / capS chunks (LR / LS in all);
// build sweeps of BSW chunks into slots of SLOT words.
struct JoinShape {
    uint32_t F = 0, NSUB = 0, NJ = 0, nseg = 1, CH = 0, G = 0;
    uint64_t capR = 0, capS = 0, LR = 0, LS = 0, items_max = 0;
    uint64_t BSW = 0, SLOT = 0, sweeps_max = 0;
    bool     slice_mode = false;
    uint64_t seg_stride() const { return LS * 32; }  // survivor words of one slice segment
    static JoinShape make(uint32_t F, uint32_t NSUB, uint32_t NJ, uint32_t nseg, uint32_t G, uint64_t capR,
                          uint64_t capS, bool slice_mode);
};

// The modes whose pass-1 scatters are the only readers of the raw relations (Engine::enqueue): a
// bitmap beside a key column reaches every reader there. Not the global-bitmap mode (k_build_global,
// k_probe_global and the side passes read the columns) nor basic k >= 2 (k_bitpos reads R).
inline bool masks_supported(const Geometry& g) {
    return g.mode == MODE_NOBLOOM || g.mode == MODE_SLICE_BLOCK || (g.mode == MODE_SLICE_BASIC && g.k == 1);
}
constexpr int kRcMaskFilter = 9;  // a validity bitmap with an unsupported filter (hwbrj_join_partitioned's code)

struct DevBuf {
    void*  p     = nullptr;
    size_t bytes = 0;
    bool   ensure(size_t need);  // grow-only
    void   release();
    template <class T> T* as() const { return (T*) p; }
};

// Pass-1 output of one relation: its chunk pool and metas, the scatter's per-workgroup queues, and
// the chunk lists / element / item starts indexed from them (k_plan, k_list_fill).
struct PartSide {
    DevBuf pool, meta, used, wgqc, wgqe, wgqo, lstart, estart, istart, list;
    DevBuf col;  // per-partition totals from k_plan: u64 elements [F], then u32 chunks [F]
    // chunks: G regions of the scatter's region capacity; F partitions
    bool   ensure(uint64_t chunks, uint32_t G, uint32_t F);
    void   release();
    // the scatter's outputs (pool, meta, wg_used, wgq_chunks, wgq_elems, cap)
    void   bind(ScatterParams* sp, uint64_t cap) const;
};
// k_plan + k_list_fill of one scattered side: lists and starts for items of per_item chunks, nseg
// items per piece
void index_side(const PartSide& s, uint64_t cap, uint32_t log2F, uint32_t per_item, uint32_t nseg,
                uint32_t G, hipStream_t st);
// chunks of one scatter workgroup's region for n tuples over G workgroups and F partitions
uint64_t region_cap(uint64_t n, uint32_t G, uint32_t F);
// Pass-1 limits: k_plan's row groups (G <= 512), the list entries' 27-bit chunk ids (hwbrj_kernels.hip,
// K4) and the metas' 22-bit region offsets
inline bool part_fits(uint32_t G, uint64_t capR, uint64_t capS) {
    return G <= 512 && G * capR <= (1ull << 27) && G * capS <= (1ull << 27) && capR < (1u << 22) &&
           capS < (1u << 22);
}
// workgroups per CU of a kernel with this much LDS (160 KB per CU), at most 2
inline uint32_t wg_per_cu(size_t lds_bytes) {
    return (uint32_t) std::max<size_t>(1, std::min<size_t>(2, 163840 / lds_bytes));
}
// JoinParams::bitmap: the job keys v = code >> hash_shift fit k_join's direct-address bitmap
inline bool join_uses_bitmap(const Geometry& g) {
    return g.sub_shift > 0 && 32 - g.hash_shift <= join_bitmap_log2();
}

// What the R side of a join (pass-1, lists, k_build, slices) leaves behind for the stages after it:
// everything the probe and the join stages read of R. The Engine keeps one for the one-shot entries,
// rewritten by every join; a prepared build (Build, include/hwbrj.h hwbrj_build_keys_device) owns
// another, written once. R.istart (the sweeps' starts) is the only table of R's PartSide the later
// stages read: a build frees the rest, and ppoolR, after its k_build (Engine::build).
// g, s, kbits, nR: the geometry, the R half of the shape (JoinShape::make with capS = 0), the packed
// join-key bits and |R| of the last R side run into it (a probe takes its shape from them).
// rvalid: a build's own copy of R's validity bitmap (the NULL R rows of the outer and group probes),
// or empty: R had none.
struct RSide {
    PartSide  R;
    DevBuf    slices, rjoin, rrun, rpay, ppoolR, rvalid;
    Geometry  g{};
    JoinShape s{};
    uint32_t  kbits = 0;
    uint64_t  nR    = 0;
    bool      r_masked = false;
    void      release();
    size_t    bytes() const;
};

// A prepared build (hwbrj_build_t): R's side, made once by Engine::build, probed by any number of
// S batches (Engine::run with the build). rows: HWBRJ_BUILD_ROWS, the payload pipeline's R side with
// R's row indices as payloads, and one mark bit per R row (marks; bit i & 31 of dword i >> 5) that
// the marking probes OR into and Engine::unmatched reads; cnt: its row counter. args: the filter the
// build was made with (has_args), kept for the probes' stats and export.
// gacc[agg]: the group accumulators of form agg (GroupAgg), one 16-byte entry per R row in the layout
// of the form's output row, empty until the first accumulating probe or reset of that form
// (Engine::group_acc_reset); gacc_ns[agg]: the sum of the nS of the accumulating probes since then or
// since the last reset, which stays below 2^32 so that 32-bit counts and 64-bit sums stay exact.
struct Build {
    RSide               r;
    bool                rows = false, has_args = false;
    int                 device = 0;
    bloom_filter_args_t args{};
    DevBuf              marks, cnt;
    DevBuf              gacc[2];
    uint64_t            gacc_ns[2] = {0, 0};
    size_t              bytes() const { return r.bytes() + marks.bytes + cnt.bytes + gacc[0].bytes + gacc[1].bytes; }
    void                release();  // every device buffer
};

class Engine {
  public:
    explicit Engine(int device);
    ~Engine();
    // One synchronous join (JoinReq): enqueue, wait, then the kind's extra counts (*x, or nullptr).
    // Returns 0 on success. st->matches = matches (COUNT) or rows (all of them, also beyond cap).
    // kRcMatGlobal: a payload join in the global-bitmap mode (run COUNT, then side()).
    // b: a probe of a prepared build: in.dR is not read, in.nR and in.args are the build's, and the
    // R side is skipped (enqueue).
    int  run(const JoinIn& in, const JoinReq& req, hwbrj_stats_t* st, JoinExtras* x = nullptr,
             const Build* b = nullptr);
    // A prepared build: the R side of the one-shot join of (dR, vR, nR, args), into buffers b owns
    // (rows: the payload pipeline's, else the counting join's with the packing the hint decides now).
    // Synchronous; what only k_build reads is freed before it returns. *ms: its device time.
    int  build(const void* dR, const uint8_t* vR, uint64_t nR, const bloom_filter_args_t* args, hipStream_t stream,
               Build* b, double* ms);
    // {R row, -1} of every R row whose mark is clear (k_null_rows over the marks); *n: all of them
    int  unmatched(Build* b, uint2* out, uint64_t cap, uint64_t* n, hipStream_t stream, double* ms);
    // The group accumulators of form agg: allocated if they are not yet, set to the identity rows, and
    // the form's running nS to 0. Synchronous.
    int  group_acc_reset(Build* b, uint32_t agg);
    // The rows of the accumulators of form agg (k_group_acc_rows): all nR of them, or those with a
    // count; *n: all of them, *pairs: the sum of their counts. A form without accumulators is one after
    // a reset, and is answered without allocating them.
    int  group_rows(Build* b, uint32_t agg, bool all, uint4* out, uint64_t cap, uint64_t* n, uint64_t* pairs,
                    hipStream_t stream, double* ms);
    int  export_build_filter(const Build& b, uint8_t* host_out, uint64_t nbytes);
    // The build's filter applied to a key column (k_filter_keys): the selection bitmap of dS[0, nS) under
    // vS (or nullptr) into out, *n_pass = its set bits, *ms = the pass's device time. Synchronous. Reads
    // b's slices and geometry only: no join state, no ring slot, no pending join is touched. The caller
    // (hwbrj_api.cpp) has checked the arguments; nS > 0 and b has a filter.
    int  filter_keys(const Build& b, const int32_t* dS, const uint8_t* vS, uint64_t nS, uint8_t* out, uint64_t* n_pass,
                     hipStream_t stream, double* ms);
    // Enqueue only, a counting join without masks: wait() then waits for the last enqueued join.
    int  run_async(const JoinIn& in, int jkind = 0, int layout = SRC_TUPLES);
    int  wait(hwbrj_stats_t* st);
    // Every join enqueued since the last wait / wait_all, oldest first, each with its own counts
    // (they stay on the device in a ring of kJoinRing result slots, one per join; an enqueue that
    // finds the ring full collects it on the host first). *n = the number of joins; 7 when it
    // exceeds cap (the oldest cap are written).
    static constexpr int kJoinRing = 64;
    int  wait_all(hwbrj_stats_t* st, int cap, int* n);
    // async joins time their S scatter (the dominant kernel) with events on the side stream they
    // run it on: stats ms_s_scatter of every collected join (include/hwbrj.h hwbrj_set_async_timing)
    void set_async_timing(bool on) { async_timing_ = on; }
    // Allocates every buffer a join of these inputs needs, without launching it (the host BPRO
    // stages this before its timed region, like the reference's allocations before its timer).
    int  reserve(const uint2* dR, uint64_t nR, const uint2* dS, uint64_t nS,
                 const bloom_filter_args_t* args, int jkind = 0);
    int  export_filter(uint8_t* host_out, uint64_t nbytes);
    // Test-only readback of the last collected synchronous join (include/hwbrj.h hwbrj_tables_info /
    // hwbrj_tables_read): its geometry and launch shape, and one of its tables copied to the host.
    // hipMemcpy only: no kernel, no device write.
    int  tables_info(uint64_t* out, int n);
    int  tables_read(int which, void* host_out, uint64_t cap_bytes, uint64_t* bytes);
    // The side pass of a payload join after a counting join (global-bitmap mode; one skeleton:
    // side_pass), selected by req.kind. *n = rows (all of them, also beyond the capacity); *x as in
    // run(); *ms = the side pass's device time.
    int  side(const JoinIn& in, const JoinReq& req, uint64_t* n, JoinExtras* x, double* ms);
    int  generate(uint2* d_out, uint64_t n, uint64_t offset, uint64_t count, uint32_t nthreads,
                  uint64_t maxid, uint64_t threshold, double selectivity, uint64_t seed,
                  hipStream_t stream);
    // The partitioned multi-GPU join of rank `rank` (include/hwbrj.h hwbrj_join_partitioned).
    // native: x is the library's own RCCL exchange, whose collectives are enqueued on this
    // engine's stream (no host synchronisation before them).
    int  join_partitioned(const hwbrj_exchange_t* x, int rank, int world, const uint2* dR,
                          uint64_t nR, uint64_t nR_total, const uint2* dS, uint64_t nS,
                          const bloom_filter_args_t* args, hwbrj_stats_t* st, bool native = false);
    void release();
    int  device() const { return device_; }

    // ---- native RCCL transport (hwbrj_comm.cpp) ----
    int  comm_init(const uint8_t* unique_id, int world, int rank);
    int  comm_destroy();
    bool has_comm() const { return comm_ != nullptr; }
    int  comm_world() const { return comm_world_; }
    int  comm_rank() const { return comm_rank_; }
    // the partitioned join over this engine's communicator
    int  join_partitioned_rccl(const uint2* dR, uint64_t nR, uint64_t nR_total, const uint2* dS,
                               uint64_t nS, const bloom_filter_args_t* args, hwbrj_stats_t* st);
    // replicated design: the filter slices built on rank 0 only and broadcast (ncclBroadcast on the
    // join stream) instead of rebuilt from R on every rank
    void set_filter_broadcast(bool on) { bcast_ = on; }
    hipStream_t stream() const { return own_stream_; }
    DevBuf*     xslot(int s) { return &xslot_[s]; }
    DevBuf*     xcnt() { return &xcnt_; }
    void*       comm() const { return comm_; }
    // the library's own RCCL exchange (hwbrj_comm.cpp): collectives on this engine's stream
    hwbrj_exchange_t native_exchange();

    // ---- the async partitioned join (hwbrj_pjoin_async.cpp; include/hwbrj.h) ----
    static constexpr int kPjDepth = 8;   // joins in flight (result ring slots)
    static constexpr int kPjKey   = 10;  // words of a plan's shape key
    // x == nullptr: over this engine's RCCL communicator (no host wait); else the caller's
    // exchange callbacks (host-synchronous exchanges, the same padded layout and plan)
    int  join_partitioned_async(const hwbrj_exchange_t* x, int rank, int world, const uint2* dR, uint64_t nR,
                                uint64_t nR_total, const uint2* dS, uint64_t nS, const bloom_filter_args_t* args);
    int  join_partitioned_wait(hwbrj_stats_t* st);
    void pj_async_info(uint64_t* out) const;
    // end of a synchronous native join asked for a plan (pj_make_plan()): a collective
    bool pj_make_plan() const { return pj_make_plan_; }
    int  pj_plan_from_sync(int world, int rank, uint64_t nR, uint64_t nR_total, uint64_t nS,
                           const bloom_filter_args_t* args, uint64_t mr, uint64_t mi, uint64_t mw);
    // drains the joins in flight (before a synchronous join grows buffers they use)
    int  pj_drain();

  private:
    struct PjGeom {
        Geometry g{};
        uint32_t F = 0, NSUB = 0, W = 0, QL = 0, q0 = 0, nseg = 1, CH = 0, G = 0, NC = 0, items_max = 0;
        uint64_t BSW = 0, SLOT = 0, capR = 0, capS = 0, LS = 0;
        bool     slice_mode = false;
    };
    struct PjPlan {
        bool     valid = false;
        uint64_t BR = 0, BI = 0, BW = 0;  // block bounds: R chunks, survivor items, survivor words
        uint64_t key[kPjKey] = {};
    };
    struct PjX {  // the transport of an async join
        hwbrj_exchange_t x{};
        bool             native = true;
        int              rank = 0, world = 1;
    };
    struct PjIn {
        PjX                 xc;
        const uint2*        dR = nullptr;
        const uint2*        dS = nullptr;
        uint64_t            nR = 0, nR_total = 0, nS = 0;
        bool                has_args = false;
        bloom_filter_args_t args{};
    };
    struct PjPending {
        PjIn          in;
        PjGeom        G;
        bool          sync = false;  // ran synchronously at enqueue (made the plan): rc, st
        bool          failed_mode = false;
        int           rc   = 0;
        int           slot = 0;
        hwbrj_stats_t st{};
    };
    bool pj_geom(int world, int rank, uint64_t nR, uint64_t nR_total, uint64_t nS,
                 const bloom_filter_args_t* args, PjGeom* G);
    int  pj_async_alloc(const PjGeom& G, const PjPlan& p, bool all, const PjX& c);
    int  pj_a2a_u64(const PjX& c, const uint64_t* d_send, uint64_t* d_recv, uint64_t n);
    int  pj_max_dev(const PjX& c, uint64_t* d, uint64_t n);
    int  pj_max_host(const PjX& c, uint64_t* h, uint64_t n);
    int  pj_establish_plan(const PjGeom& G, uint64_t mr, uint64_t mi, uint64_t mw, const uint64_t* key);
    int  pj_sync_join(const PjIn& in, hwbrj_stats_t* st);
    PjPlan                pj_plan_;
    PjX                   pj_cur_;  // the transport of the synchronous join making a plan
    bloom_filter_args_t   pj_plan_args_{};
    bool                  pj_make_plan_ = false;
    bool                  pj_lost_      = false;  // the plan's buffers were released (this rank)
    std::deque<PjPending> pj_q_;
    uint64_t              pj_seq_ = 0, pj_async_ = 0, pj_sync_ = 0, pj_fallbacks_ = 0, pj_plans_ = 0;
    uint64_t              pj_last_flag_ = 0, pj_last_sizes_[3] = {0, 0, 0};
    DevBuf                pjX, pjRitems, pjRing;  // flag + sizes + counts messages; ritems; result ring
    hipEvent_t            pjEv_[2 * kPjDepth] = {};

  private:
    struct SideBuf {  // a buffer of one kind's side pass: `bytes` of 32-bit words `fill` on entry
        DevBuf*  buf;
        size_t   bytes;
        uint32_t fill;
    };
    template <class Launch>
    int side_pass(const void* dR, uint64_t nR, int layout, hipStream_t stream, const char* what,
                  const std::vector<SideBuf>& own, uint64_t* c, uint32_t nc, double* ms, Launch&& launch);
    int pairs_side(const JoinIn& in, const JoinReq& q, uint64_t* n, double* ms);
    int semi_side(const JoinIn& in, const JoinReq& q, uint64_t* n, double* ms);
    int outer_side(const JoinIn& in, const JoinReq& q, uint64_t* n, uint64_t cls[3], double* ms);
    int group_side(const JoinIn& in, const JoinReq& q, uint64_t* n, uint64_t* pairs, double* ms);
    void*        comm_       = nullptr;  // ncclComm_t of this device's rank (hwbrj_comm_init)
    int          comm_world_ = 1, comm_rank_ = 0;
    bool         bcast_      = false;
    DevBuf       xslot_[HWBRJ_PJ_NSLOTS], xcnt_;  // the native exchange's buffers
    DevBuf       agree_;                           // status words of the broadcast join's agreement
    DevBuf       fkcnt_;                           // filter_keys' row counter
    int          device_;
    int          cus_ = 256;
    hipStream_t  own_stream_ = nullptr;
    hipStream_t  ovl_stream_ = nullptr;             // async joins: the S pass's stream
    hipEvent_t   ovl_ev_[2]  = {nullptr, nullptr};  // (fork, join of ovl_stream_)
    hipEvent_t   ev_[10];
    bool         have_filter_ = false;
    Geometry     last_g_{};
    // the last enqueued join (collected by wait)
    bool         pending_      = false;
    uint32_t     last_nj_      = 0;  // join jobs of the last enqueue (job_surv layout)
    // phase events: recorded by synchronous joins only (run_async clears phase_ev_); surv_fused_:
    // the pending join's survivor phase is fused into its probe (no ev_[7] of its own)
    bool         phase_ev_     = true;
    bool         pending_ev_   = true;
    // the stream the pending join was enqueued on. Joins on the same stream are ordered by it; a
    // join on another stream waits for ev_[8]. Compared by handle: a stream must outlive the
    // joins enqueued on it (a destroyed stream's handle can be reused by a new one).
    hipStream_t  pending_stream_ = nullptr;
    bool         pending_sfirst_ = false;  // the pending join ran its S pass first (phase boundaries)
    bool         pending_prepared_ = false;  // the pending join probed a prepared build: no R phases
    bool         pack3_hint_     = true;   // the last waited join had none: packed join keys pay
    int          pending_rc_     = 0;   // nonzero: the pending join failed after enqueuing kernels
    std::string  pending_err_;
    bool         surv_fused_   = false;
    // per-join results: join i writes its counts and k_join's partial sums into ring slot
    // i mod kJoinRing (jring_), so every join of a back-to-back run can be checked, not only the
    // last (the reference sums every thread's count per run, parallel_radix_join_bloom.c:1696-1707)
    struct JoinRec {
        uint32_t slot = 0;
        bool     args = false, fmt = false, slots = false, timed = false;
        bool     s_masked = false;  // S had a validity bitmap (KeyMasks)
        uint32_t kbits = 0;  // packed join-key bits (0: 32-bit codes)
        uint64_t nS   = 0;
        Geometry g{};
    };
    DevBuf                     jring_;
    std::vector<JoinRec>       jr_;     // enqueued since the last wait, oldest first
    std::vector<hwbrj_stats_t> jdone_;  // collected early (the ring was full), oldest first
    uint32_t                   jr_next_ = 0;
    hwbrj_stats_t              last_st_{};  // the last collected join (with its phase times)
    bool                       async_timing_ = false;      // hwbrj_set_async_timing
    hipEvent_t                 tev_[kJoinRing][2] = {};    // per slot: the async S scatter's start, end
    void*        ring_take(uint32_t* slot);            // the next slot's bytes (jring_ grown first)
    // the last taken slot. Its u64 words 6 and 7 belong to the join's kind (zeroed with the counts
    // by the R scatter, not read by ring_collect): OUTER's {R-only, S-only} rows, GROUP's pairs in
    // word 6; run() reads them after the join (the slot is taken again by the next enqueue only)
    const uint64_t* last_slot_ = nullptr;
    int          ring_collect();                       // jr_ (completed) -> jdone_
    int          wait_pending();
    void         ring_drop() { jr_.clear(); jdone_.clear(); }
    hipError_t   mark(int i, hipStream_t stream);  // ev_[i] when phase_ev_
    bool         alloc_only_   = false;  // reserve(): enqueue returns after its allocations
    // One enqueue's state, stage to stage (hwbrj_engine.cpp "Engine::enqueue")
    struct JoinCtx {
        JoinIn         in;  // (stream: never nullptr after validate)
        const JoinReq& q;
        Geometry       g{};
        JoinShape      s{};
        // the bitmap of each non-empty side, or nullptr (an empty column has no NULL rows); vV: S's
        // value column (the group joins)
        const uint8_t *vR = nullptr, *vS = nullptr, *vV = nullptr;
        bool      basic_kk = false;       // basic k >= 2 on the payload pipeline: slices from bit positions
        uint64_t  nRk      = 0;           // its k * |R| bit positions
        bool      bcast    = false;       // the slices arrive by RCCL broadcast: a collective
        bool      jnew     = false;       // the job table is cleared first
        char*     sm       = nullptr;     // the ring slot, number rslot
        uint32_t  rslot = 0, kbits = 0;   // kbits: packed join-key bits of build / probe / join
        bool      rtimed = false, s_first = false;
        const Build* b  = nullptr;        // a probe of this prepared build: no R side
        const RSide* rs = nullptr;        // what the stages after the R side read: b->r, or the Engine's own
        uint64_t* result() const { return (uint64_t*) sm; }  // [0] matches / rows, [1] dense count, [2] filtered
    };
    // what tables_info / tables_read need of the last enqueued join: which pipeline left its tables
    // in the buffers below, and the shape they are indexed with
    enum { kTabNone = 0, kTabJoin = 1, kTabOther = 2 };  // kTabOther: a pipeline with other tables
    struct TabRec {
        int       state = kTabNone;
        bool      sync = false, mat = false;
        Geometry  g{};
        JoinShape s{};
        uint32_t  stage_cap = 0, jkind = 0, kbits = 0, bitmap = 0, split = 0;
    };
    // the stages of enqueue, in order (hwbrj_engine.cpp)
    int          validate(JoinCtx* c);
    void         plan(JoinCtx* c);
    bool         ensure_common(const JoinShape& s, uint32_t surv_segs, bool* jnew, bool r_side = true);
    bool         ensure_buffers(JoinCtx* c);
    int          s_pass(const JoinCtx& c, hipStream_t st, bool marks, hipEvent_t* tev);
    int          r_side(const JoinCtx& c, RSide* r, uint32_t* zero_small, uint32_t* zero_word);
    int          passes(JoinCtx* c);
    int          probe(const JoinCtx& c, ProbeParams* pp);
    int          join_count(const JoinCtx& c, const JoinParams& jp);
    int          join_pairs(const JoinCtx& c, const JobInputs& ji);
    int          join_semi(const JoinCtx& c, const JobInputs& ji);
    int          join_outer(const JoinCtx& c, const JobInputs& ji);
    int          join_group(const JoinCtx& c, const JobInputs& ji);
    int          clear_job_surv(const JoinCtx& c);
    MatJoinParams mat_params(const JoinCtx& c, const JobInputs& ji) const;
    int          finish(const JoinIn& in, const Geometry& g, bool s_first, const TabRec& tab, JoinRec rec,
                        bool prepared = false);
    // the parameter blocks both enqueue paths share; each path overrides what differs
    ScatterParams scatter_params(const Geometry& g, const PartSide& side, uint64_t cap) const;
    BuildParams  build_params(const RSide& r, const Geometry& g, const JoinShape& s) const;
    ProbeParams  probe_params(const Geometry& g, const JoinShape& s) const;
    JoinParams   join_params(const RSide& r, const Geometry& g, const JoinShape& s, char* slot, int jkind) const;
    int          enqueue(const JoinIn& in, const JoinReq& req, const Build* b = nullptr);
    int          export_slices(const DevBuf& sl, const Geometry& g, uint8_t* host_out, uint64_t nbytes);
    // basic k >= 2 without payloads: the repartitioning pipeline (hwbrj_engine.cpp)
    int          enqueue_basic_kk(const JoinIn& in, const Geometry& g, const JoinReq& req);
    TabRec       tab_;
    int          tables_ready();  // 0, or why the tables cannot be read (the codes of hwbrj.h)
    CrcTables*   d_tabs_ = nullptr;
    GenPlan*     d_plan_ = nullptr;
    // the one-shot entries' R side (RSide) under the names its buffers always had
    RSide     rs_;
    PartSide& R_ = rs_.R;
    PartSide  S_;
    DevBuf &  slices = rs_.slices, &rjoin = rs_.rjoin, &rrun = rs_.rrun, &rpay = rs_.rpay, &ppoolR = rs_.ppoolR;
    DevBuf bitmap, surv, survcnt, survoff, dense, small;
    DevBuf bpos;        // basic k >= 2: R bit positions (k_bitpos)
    DevBuf mtab, mcount;  // the side passes: R table, counters
    // materializing pipeline: payload pools (chunk layout of R_.pool / S_.pool), R payloads of the
    // build sweeps, survivors' chunk positions
    DevBuf ppoolS, survpos;
    DevBuf smark;  // existence / outer join: one bit per S chunk position (matched survivors); the
                   // outer side pass: one bit per slot of its table of R (outer_side)
    DevBuf gcnt, gsum;  // the group join's side pass: count and sum per R row (group_side)
    DevBuf gmin, gmax;  // its min/max form: min and max per R row
    DevBuf dense2, kkcnt;  // basic k >= 2: the second dense candidate buffer, per-pass counts
    DevBuf jtask, jparts;  // join task table; parts per job (+ the task count)
    // partitioned join: owned partitions' lists, tables and received survivor descriptors
    DevBuf pjList, pjLstart, pjSweep, pjTab, pjRegion, pjTot, pjSoff, pjIbase, pjCnt, pjOff, pjIstart, pjJobs;
    DevBuf pjBsum, pjBound, pjWtot, pjWscan, pjTab2;  // device-side item tables (scans, bounds)
};

Engine* engine_for_current_device();
void    set_last_error(const std::string& s);

// RCCL entry points used by the engine (hwbrj_comm.cpp; librccl is bound at first use). Return 0 or
// an error code with the message in set_last_error.
int rccl_broadcast(void* comm, void* buf, size_t bytes, int root, hipStream_t stream);
// The counts a join leaves in the small buffer (`small`: result words, then k_join's partial-sum
// slots), read in one copy: h[0] matches, h[1] dense count, h[2] filtered, h[3] probe ticks,
// h[4] join ticks, h[5] unstaged probe items; with slots, their sums are added to h[0], h[3], h[4].
int read_join_counts(const void* small, bool slots, hipStream_t stream, uint64_t h[6]);
int rccl_agree_status(void* comm, int world, int rank, int rc, hipStream_t stream, DevBuf* tmp);
class Engine;
int rccl_alltoall_u64_dev(Engine* e, const uint64_t* d_send, uint64_t* d_recv, uint64_t n);
int rccl_allreduce_max_u64(Engine* e, uint64_t* d, uint64_t n);
// HWBRJ_RCCL_SELF (tests): a rank's own exchange blocks go through ncclSend / ncclRecv too
bool rccl_self_blocks();

// glibc's rand() (stdlib/random_r.c TYPE_3) with private state (hwbrj_gen.cpp).
struct GlibcRand {
    int32_t st[31];
    int     f = 3, r = 0;
    void    seed(uint32_t s);
    int32_t next() {
        st[f]           = (int32_t) ((uint32_t) st[f] + (uint32_t) st[r]);
        const int32_t v = (int32_t) ((uint32_t) st[f] >> 1);
        f               = f == 30 ? 0 : f + 1;
        r               = r == 30 ? 0 : r + 1;
        return v;
    }
};

}  // namespace hwbrj
