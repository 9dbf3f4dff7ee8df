// hwbrj_engine.cpp -- host orchestration of the MI355X bloom radix join (DESIGN.md "Pipeline").
//
// The reference runs R pass-1 (+ bloom add), S pass-1 (+ bloom contains), pass-2 and the
// bucket-chaining join inside pthreads with barriers (src/parallel_radix_join_bloom.c:1059-1506).
// Here every barrier is a kernel boundary on one HIP stream, and the task queues are replaced by
// device-built chunk lists and item tables (no host round trips inside the join).
#include "hwbrj_engine.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

namespace hwbrj {

#define HWBRJ_CHECK(expr)                                                                 \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) {                                                           \
            set_last_error(std::string(#expr) + ": " + hipGetErrorString(e_));            \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

// ---------------------------------------------------------------------------- tables
bool build_crc_tables(CrcTables* t) {
    uint32_t col[32];  // f(e_i)
    for (int i = 0; i < 32; i++) col[i] = crc_f_bitwise(1u << i);
    for (int j = 0; j < 8; j++)
        for (int v = 0; v < 16; v++) t->fwd[j][v] = crc_f_bitwise((uint32_t) v << (4 * j));
    // Invert the 32x32 GF(2) matrix whose column i is col[i]: solve f(x) = e_r for every r.
    // Gauss-Jordan on rows of [M | I] packed as 64-bit rows (row r: bit c of M, bit 32+c of I).
    uint64_t rows[32];
    for (int r = 0; r < 32; r++) {
        uint64_t row = 0;
        for (int c = 0; c < 32; c++)
            if ((col[c] >> r) & 1u) row |= 1ull << c;
        rows[r] = row | (1ull << (32 + r));
    }
    for (int c = 0; c < 32; c++) {
        int piv = -1;
        for (int r = c; r < 32; r++)
            if ((rows[r] >> c) & 1ull) {
                piv = r;
                break;
            }
        if (piv < 0) return false;
        std::swap(rows[c], rows[piv]);
        for (int r = 0; r < 32; r++)
            if (r != c && ((rows[r] >> c) & 1ull)) rows[r] ^= rows[c];
    }
    // rows now = [I | M^-1]; column j of M^-1 = finv(e_j)
    uint32_t icol[32];
    for (int j = 0; j < 32; j++) {
        uint32_t v = 0;
        for (int r = 0; r < 32; r++)
            if ((rows[r] >> (32 + j)) & 1ull) v |= 1u << r;
        icol[j] = v;
    }
    for (int j = 0; j < 8; j++)
        for (int v = 0; v < 16; v++) {
            uint32_t x = (uint32_t) v << (4 * j), r = 0;
            for (int b = 0; b < 32; b++)
                if ((x >> b) & 1u) r ^= icol[b];
            t->inv[j][v] = r;
        }
    // self-check on a few values
    for (uint32_t x : {0u, 1u, 42u, 0xDEADBEEFu, 0x7FFFFFFFu}) {
        if (nibble_map(&t->inv[0][0], nibble_map(&t->fwd[0][0], x)) != x) return false;
        if (nibble_map(&t->fwd[0][0], x) != crc_f_bitwise(x)) return false;
    }
    return true;
}

// ------------------------------------------------------------------------- generator plan
int make_gen_plan(GenPlan* plan, uint64_t num_tuples, uint32_t nthreads, uint64_t maxid,
                  uint64_t threshold, double selectivity) {
    // src/generator.c:331-395, integer widths as in the reference
    if (nthreads == 0 || nthreads > (uint32_t) kMaxGenChunks || threshold == 0) return 1;
    const unsigned int pagesize      = 4096;
    unsigned int       npages        = (unsigned int) ((num_tuples * 8u) / pagesize + 1u);
    unsigned int       npages_perthr = npages / nthreads;
    uint64_t ntuples_perthr = (uint64_t) npages_perthr * (uint64_t) (pagesize / 8u);
    uint64_t ntuples_above  = (uint64_t) ((double) num_tuples * (1 - selectivity));
    if (npages_perthr == 0) ntuples_perthr = num_tuples / nthreads;
    uint64_t ntuples_above_perthr  = (uint64_t) ((double) ntuples_perthr * (1 - selectivity));
    uint64_t ntuples_lastthr       = num_tuples - ntuples_perthr * (nthreads - 1);
    uint64_t ntuples_above_lastthr = ntuples_above - (uint64_t) (nthreads - 1) * ntuples_above_perthr;
    uint64_t offset = 0, offset_above = 0;
    plan->nchunks    = nthreads;
    plan->num_tuples = num_tuples;
    plan->threshold  = threshold;
    const uint64_t span = maxid > threshold ? maxid - threshold : 0;
    for (uint32_t t = 0; t < nthreads; t++) {
        GenChunk& c  = plan->chunk[t];
        c.firstkey   = (int64_t) ((offset + 1) % threshold);
        c.firstabove = (int64_t) (threshold + (offset_above + 1) % (span > 1 ? span : 1));
        uint64_t na  = (t == nthreads - 1) ? ntuples_above_lastthr : ntuples_above_perthr;
        c.n          = (t == nthreads - 1) ? ntuples_lastthr : ntuples_perthr;
        c.start      = offset + offset_above;
        if (na > c.n || c.start + c.n > num_tuples) return 2;  // the reference would overrun
        c.n_below = c.n - na;
        offset += ntuples_perthr - ntuples_above_perthr;
        offset_above += ntuples_above_perthr;
    }
    return 0;
}

// ------------------------------------------------------------------------------ geometry
bool plan_geometry(const bloom_filter_args_t* a, uint64_t nR, Geometry* g, std::string* err, bool mat) {
    memset(g, 0, sizeof(*g));
    g->variant = -1;
    if (!a) {
        g->mode  = MODE_NOBLOOM;
        g->log2F = kMaxLog2F;
    } else {
        const uint64_t m = a->m, B = a->B, k = a->k;
        if (m == 0 || (m & (m - 1)) != 0) {
            *err = "m must be a power of 2";  // src/bloom_filter.c:27
            return false;
        }
        if (m > (1ull << 32)) {
            *err = "m > 2^32 bits is outside the 32-bit hash contract of src/bloom_filter.c";
            return false;
        }
        if (k > 4096) {
            *err = "k > 4096 is not supported";
            return false;
        }
        if (a->variant != BASIC && a->variant != BLOCKED && a->variant != SECTORIZED) {
            *err = "unknown filter variant";
            return false;
        }
        g->variant = (int) a->variant;
        g->k       = (uint32_t) k;
        g->m       = m;
        if (a->variant != BASIC) {
            if (B == 0 || (B & (B - 1)) != 0) {
                *err = "B must be a power 2";  // src/bloom_filter.c:30
                return false;
            }
            if (m % B != 0) {
                *err = "m must be a multiple of B";  // :31
                return false;
            }
            if (B > (1ull << 31)) {
                *err = "B too large";
                return false;
            }
            g->B          = (uint32_t) B;
            g->nblocks    = (uint32_t) std::min<uint64_t>(m / B, 0xFFFFFFFFull);
            g->block_span = (uint32_t) ((B / 8) * 8);
        }
        uint64_t F = 0;
        if (a->variant == BASIC) {
            // k >= 2: KIND_BASIC_KK, whose slice build partitions k * |R| bit positions (bounded by
            // the scatter's chunk ids; beyond that the global fallback)
            if (k >= 1 && m >= 32 && k * nR <= (1ull << 31)) {
                g->mode = MODE_SLICE_BASIC;
                F       = std::min<uint64_t>(1024, m / 32);
            } else {
                g->mode = MODE_GLOBAL;
            }
        } else {
            if (B >= 8 && m >= 32 && (m / B) <= 0xFFFFFFFFull) {
                g->mode = MODE_SLICE_BLOCK;
                F       = std::min<uint64_t>(std::min<uint64_t>(1024, m / B), m / 32);
            } else {
                g->mode = MODE_GLOBAL;
            }
        }
        g->log2F = (g->mode == MODE_GLOBAL) ? kMaxLog2F : ilog2u(F);
        if (g->mode == MODE_SLICE_BLOCK || g->mode == MODE_SLICE_BASIC) {
            g->slice_bits = (uint32_t) (m >> g->log2F);
            g->seg_bits   = std::min(g->slice_bits, kSliceMaxBits);
            g->nseg       = g->slice_bits / g->seg_bits;
            g->seg_words  = std::max<uint32_t>(4, g->seg_bits / 32);
        }
        if (g->mode == MODE_SLICE_BLOCK && ilog2u(B) <= g->log2F) g->format = FMT_PACKED;
        // S partitions use R's word format (the 22-bit S words of round 2, FMT_C22, cut 2.6 GB of
        // S traffic but cost more in the probe's key recovery: removed in round 6)
        g->s_format = g->format;
        if (g->mode == MODE_SLICE_BLOCK || g->mode == MODE_SLICE_BASIC) g->log2seg = ilog2u(g->seg_bits);
        if (a->variant != BASIC) {
            g->log2B    = ilog2u(B);
            g->log2secw = std::min<uint32_t>(g->log2B, 6);
            g->nsecmask = (uint32_t) (B >> g->log2secw) - 1u;
            if (g->mode == MODE_SLICE_BLOCK) g->lbmask = (g->nblocks >> g->log2F) - 1u;
        }
    }
    // Join sub-partitions (k_join): codes of a job share their low hash_shift bits. Where the
    // partition digit is a code digit (sub_shift = log2F), 2^(14 - log2F) subs make the job keys
    // v = code >> hash_shift fit the 2^18-bit LDS bitmap; otherwise (or when that needs > 64 subs)
    // the hash table path needs <= ~4096 R keys per job.
    const uint64_t F    = 1ull << g->log2F;
    const uint64_t rper = (nR + F - 1) / F;
    uint32_t       l2s  = 0;
    g->sub_shift  = (g->mode == MODE_SLICE_BASIC) ? 0 : g->log2F;
    if (mat && g->sub_shift > 0) {  // k_join_mat's bitmap path: keys v < 2^17, <= 4096 R tuples per job
        l2s = g->log2F >= 15 ? 0 : std::min<uint32_t>(6, 15 - g->log2F);
        while (l2s < 6 && (rper >> l2s) > 4000) l2s++;
    } else if (mat) {  // its hash table: <= 2048 R tuples per piece, so ~1536 per job on average
        while (l2s < 6 && (rper >> l2s) > 1536) l2s++;
    } else if (g->sub_shift > 0 && g->log2F + 6 >= 14) {
        l2s = g->log2F >= 14 ? 0 : 14 - g->log2F;
    } else {
        while (l2s < 6 && (rper >> l2s) > 4096) l2s++;
    }
    if (g->sub_shift + l2s == 0) l2s = 1;  // k_join stores code >> hash_shift with an empty sentinel
    g->log2NSUB   = l2s;
    g->hash_shift = g->sub_shift + g->log2NSUB;
    return true;
}

// ---------------------------------------------------------------------------- buffers
bool DevBuf::ensure(size_t need) {
    if (need == 0) need = 16;
    if (need <= bytes) return true;
    release();
    if (hipMalloc(&p, need) != hipSuccess) {
        p     = nullptr;
        bytes = 0;
        return false;
    }
    bytes = need;
    return true;
}

void DevBuf::release() {
    if (p) (void) hipFree(p);
    p     = nullptr;
    bytes = 0;
}

bool PartSide::ensure(uint64_t chunks, uint32_t G, uint32_t F) {
    const uint64_t GF = (uint64_t) G * F;
    return pool.ensure(chunks * 128) && meta.ensure(chunks * 2) && list.ensure(chunks * 4) &&
           used.ensure(G * 4) && wgqc.ensure(GF * 4) && wgqe.ensure(GF * 4) && wgqo.ensure(GF * 4) &&
           lstart.ensure((F + 1) * 4) && estart.ensure((F + 1) * 8) && istart.ensure((F + 1) * 4) &&
           col.ensure(F * 12);
}

void PartSide::release() {
    for (DevBuf* b : {&pool, &meta, &used, &wgqc, &wgqe, &wgqo, &lstart, &estart, &istart, &list, &col}) b->release();
}

void RSide::release() {
    R.release();
    for (DevBuf* b : {&slices, &rjoin, &rrun, &rpay, &ppoolR, &rvalid}) b->release();
}

size_t RSide::bytes() const {
    size_t n = 0;
    for (const DevBuf* b : {&R.pool, &R.meta, &R.used, &R.wgqc, &R.wgqe, &R.wgqo, &R.lstart, &R.estart, &R.istart,
                            &R.list, &R.col, &slices, &rjoin, &rrun, &rpay, &ppoolR, &rvalid})
        n += b->bytes;
    return n;
}

void PartSide::bind(ScatterParams* sp, uint64_t cap) const {
    sp->pool       = pool.as<uint32_t>();
    sp->meta       = meta.as<uint32_t>();
    sp->wg_used    = used.as<uint32_t>();
    sp->wgq_chunks = wgqc.as<uint32_t>();
    sp->wgq_elems  = wgqe.as<uint32_t>();
    sp->cap        = cap;
}

void index_side(const PartSide& s, uint64_t cap, uint32_t log2F, uint32_t per_item, uint32_t nseg,
                uint32_t G, hipStream_t st) {
    uint32_t* colc = s.col.as<uint32_t>() + 2 * (1u << log2F);  // (behind the u64 element totals)
    launch_plan(s.wgqc.as<uint32_t>(), s.wgqe.as<uint32_t>(), G, log2F, s.wgqo.as<uint32_t>(), colc,
                s.col.as<uint64_t>(), st);
    launch_list_fill(s.meta.as<uint32_t>(), s.used.as<uint32_t>(), cap, log2F, s.wgqo.as<uint32_t>(), colc,
                     s.col.as<uint64_t>(), per_item, nseg, s.lstart.as<uint32_t>(), s.estart.as<uint64_t>(),
                     s.istart.as<uint32_t>(), s.list.as<uint32_t>(), G, st);
}

// ---------------------------------------------------------------------------- test hooks
TestHooks& test_hooks() {
    static TestHooks h;
    return h;
}

Engine::Engine(int device) : device_(device) {
    (void) hipSetDevice(device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) cus_ = prop.multiProcessorCount;
    (void) hipStreamCreateWithFlags(&own_stream_, hipStreamNonBlocking);
    // ev_[0..7] only time phases (elapsed-time reads after ev_[8] has completed): no system-scope
    // fence on record, whose cache writeback idled the GPU ~6 us per marker. ev_[8] (waited on,
    // and ordering later joins) and ev_[9] keep the default release.
    for (int i = 0; i < 10; i++)
        (void) (i < 8 ? hipEventCreateWithFlags(&ev_[i], hipEventDisableSystemFence) : hipEventCreate(&ev_[i]));
    CrcTables t;
    if (!build_crc_tables(&t)) set_last_error("CRC table inversion failed");
    (void) hipMalloc((void**) &d_tabs_, sizeof(CrcTables));
    (void) hipMemcpy(d_tabs_, &t, sizeof(CrcTables), hipMemcpyHostToDevice);
    (void) hipMalloc((void**) &d_plan_, sizeof(GenPlan));
}

Engine::~Engine() { release(); }

void Engine::release() {
    (void) pj_drain();
    pj_q_.clear();                       // (joins in flight are dropped)
    if (pj_plan_.valid) pj_lost_ = true;  // (the next async join runs in the failed mode: a new plan)
    for (DevBuf* b : {&pjX, &pjRitems, &pjRing}) b->release();
    R_.release();
    S_.release();
    for (DevBuf* b : {&slices, &bitmap, &rjoin, &rrun, &surv, &survcnt, &survoff,
                      &dense, &small, &bpos, &mtab, &mcount, &jtask, &jparts, &pjList,
                      &pjLstart, &pjSweep, &pjTab, &pjRegion, &pjTot, &pjSoff, &pjIbase, &pjCnt, &pjOff,
                      &pjIstart, &pjJobs, &ppoolR, &ppoolS, &rpay, &survpos, &smark, &gcnt, &gsum, &gmin, &gmax, &dense2, &kkcnt, &xcnt_, &pjBsum, &pjBound, &pjWtot, &pjWscan, &pjTab2})
        b->release();
    for (DevBuf& b : xslot_) b.release();
    fkcnt_.release();
    if (pending_) (void) hipEventSynchronize(ev_[8]);  // (the ring's joins end before it is freed)
    ring_drop();
    jring_.release();
    have_filter_ = false;
    tab_.state   = kTabNone;
}

// One join's result slot: 128 bytes of result words (read_join_counts), then k_join's partial sums
static size_t ring_slot_bytes() { return 128 + join_sum_slots() * join_sum_stride() * 8; }

uint64_t region_cap(uint64_t n, uint32_t G, uint32_t F) {
    const uint64_t units = (n + 3) / 4;
    const uint64_t per   = ((units + G - 1) / G) * 4;
    return (per + 31) / 32 + F + 1;
}

int Engine::run(const JoinIn& in, const JoinReq& req, hwbrj_stats_t* st, JoinExtras* x, const Build* b) {
    int rc = enqueue(in, req, b);
    if (rc == 0) rc = wait(st);
    if (rc || !x) return rc;
    // (the join has completed; its ring slot is taken again by the next enqueue only)
    if (req.kind == JOIN_OUTER) {
        uint64_t c[2];  // {R-only, S-only}; inner = rows - both
        HWBRJ_CHECK(hipMemcpy(c, last_slot_ + 6, sizeof(c), hipMemcpyDeviceToHost));
        x->cls[0] = (uint64_t) st->matches - c[0] - c[1];
        x->cls[1] = c[1];
        x->cls[2] = c[0];
    } else if (req.kind == JOIN_GROUP) {
        HWBRJ_CHECK(hipMemcpy(&x->pairs, last_slot_ + 6, sizeof(x->pairs), hipMemcpyDeviceToHost));
    }
    return 0;
}

int Engine::run_async(const JoinIn& in, int jkind, int layout) {
    // back-to-back joins: no phase events (each marker idles the GPU ~6 us between the kernels
    // around it, profiles/r03/gaps_*), so hwbrj_join_wait reports counts only
    JoinReq req;
    req.jkind    = jkind;
    req.layout   = layout;
    phase_ev_    = false;
    const int rc = enqueue(in, req);
    phase_ev_    = true;
    return rc;
}

// Phase boundary i (synchronous joins only). A marker idles the GPU ~6 us between the kernels
// around it; attaching the boundary to the next kernel's dispatch instead (hipExtLaunchKernel's
// start event) measured slower still (~10 us gaps, profiles/r03/async_no_events_ab.log).
hipError_t Engine::mark(int i, hipStream_t stream) {
    return phase_ev_ ? hipEventRecord(ev_[i], stream) : hipSuccess;
}

int Engine::reserve(const uint2* dR, uint64_t nR, const uint2* dS, uint64_t nS,
                    const bloom_filter_args_t* args, int jkind) {
    JoinReq req;
    req.jkind    = jkind;
    alloc_only_  = true;
    const int rc = enqueue(JoinIn{dR, nR, dS, nS, args, nullptr}, req);
    alloc_only_  = false;
    last_nj_     = 0;  // buffers may be new: the next join clears its job table
    return rc;
}

// ------------------------------------------------------------------- shape and limits
JoinShape JoinShape::make(uint32_t F, uint32_t NSUB, uint32_t NJ, uint32_t nseg, uint32_t G, uint64_t capR,
                          uint64_t capS, bool slice_mode) {
    JoinShape s;
    s.F = F, s.NSUB = NSUB, s.NJ = NJ, s.nseg = nseg, s.G = G;
    s.CH         = probe_chunks_per_item();  // chunks per probe item
    s.capR = capR, s.capS = capS;
    s.LR = (uint64_t) G * capR, s.LS = (uint64_t) G * capS;  // max chunks
    s.items_max  = (s.LS / s.CH + F + 1) * nseg;
    s.BSW        = build_chunks_per_sweep();
    s.SLOT       = build_sweep_slot();
    s.sweeps_max = s.LR / s.BSW + F + 1;  // build sweeps over all R partitions
    s.slice_mode = slice_mode;
    return s;
}

// the existence and payload joins' bitmap path: job keys v = code >> hash_shift < 2^17 (k_join_mat's condition)
static bool pay_bitmap(const Geometry& g) { return g.sub_shift > 0 && 32 - g.hash_shift <= 17; }
// the marks over S (one bit per chunk position): the anti join and the hash-set path's jobs of several
// R pieces; the outer join that keeps S
static bool semi_marks(const Geometry& g, const JoinReq& q) {
    return q.kind == JOIN_SEMI && (q.anti || !pay_bitmap(g));
}
static bool uses_smark(const Geometry& g, const JoinReq& q) {
    return semi_marks(g, q) || (q.kind == JOIN_OUTER && q.keep_s);
}

// Pass-1 limits of a shape under a request: nullptr, or why it is refused (code 3)
static const char* shape_limits(const JoinShape& s, const JoinReq& q) {
    if (s.G > 512) return "more than 512 scatter workgroups (k_plan row groups)";
    if (!part_fits(s.G, s.capR, s.capS))
        return "relation too large for 27-bit chunk ids (|S| or |R| > ~4.2e9 tuples per GPU)";
    if (q.carries_s_payloads() && (s.capS >= (1u << 21) || s.capR >= (1u << 21)))  // half indices (scatter_body_pay) < 2^22
        return "relation too large for the materializing scatter's 22-bit half indices";
    return nullptr;
}

// What both pipelines keep: the sides, the build sweeps' runs, the survivor runs of surv_segs segments,
// the result ring and the job table.
// jparts: nparts [NJ] | job_surv [NJ] | nextra; jtask: extra parts {job, part}
// (job_surv is left zero by k_join_split for the NJ jobs it saw: a join with another NJ clears the
// whole buffer, *jnew, so no stale count of an earlier job layout is read; last_nj_ moves whether or
// not an allocation fails)
// r_side off (a probe of a prepared build): no buffer of R's is grown, the build has its own.
bool Engine::ensure_common(const JoinShape& s, uint32_t surv_segs, bool* jnew, bool r_side) {
    *jnew    = jparts.bytes < (size_t) (2 * s.NJ + 1) * 4 || s.NJ != last_nj_;
    last_nj_ = s.NJ;
    if (r_side && !(R_.ensure(s.LR, s.G, s.F) && rjoin.ensure(s.sweeps_max * s.SLOT * 4) &&
                    rrun.ensure(2 * s.sweeps_max * s.NSUB * 4)))
        return false;
    return S_.ensure(s.LS, s.G, s.F) && surv.ensure(surv_segs * s.LS * 128) &&
           survcnt.ensure(s.items_max * s.NSUB * 4) && survoff.ensure(s.items_max * s.NSUB * 4) &&
           jring_.ensure(kJoinRing * ring_slot_bytes()) && jtask.ensure((size_t) join_extra_tasks() * 8) &&
           jparts.ensure((size_t) (2 * s.NJ + 1) * 4);
}

bool Engine::ensure_buffers(JoinCtx* c) {
    const JoinShape& s = c->s;
    const Geometry&  g = c->g;
    bool ok = ensure_common(s, s.nseg, &c->jnew, !c->b);
    if (s.slice_mode && !c->b) ok = ok && slices.ensure((uint64_t) s.F * s.nseg * g.seg_words * 4);
    if (g.mode == MODE_GLOBAL) ok = ok && bitmap.ensure(((g.m + 31) / 32) * 4) && dense.ensure(c->in.nS * 4);
    if (c->basic_kk) ok = ok && bpos.ensure(c->nRk * 4);
    if (c->q.carries_s_payloads()) ok = ok && ppoolS.ensure(s.LS * 128) && survpos.ensure(s.nseg * s.LS * 128);
    if (c->q.carries_r_payloads() && !c->b) ok = ok && ppoolR.ensure(s.LR * 128) && rpay.ensure(s.sweeps_max * s.SLOT * 4);
    if (uses_smark(g, c->q)) ok = ok && smark.ensure(s.LS * 4);
    return ok;
}

// ------------------------------------------------------------------- parameter blocks
ScatterParams Engine::scatter_params(const Geometry& g, const PartSide& side, uint64_t cap) const {
    ScatterParams sp{};
    sp.tabs = d_tabs_;
    sp.g    = g;
    side.bind(&sp, cap);
    return sp;
}

// k_build over R's lists (R items = build sweeps); no slices, no payloads, 32-bit codes
BuildParams Engine::build_params(const RSide& r, const Geometry& g, const JoinShape& s) const {
    BuildParams bp{};
    bp.g           = g;
    bp.tabs        = d_tabs_;
    bp.pool        = r.R.pool.as<uint32_t>();
    bp.list        = r.R.list.as<uint32_t>();
    bp.list_start  = r.R.lstart.as<uint32_t>();
    bp.elem_start  = r.R.estart.as<uint64_t>();
    bp.sweep_start = r.R.istart.as<uint32_t>();
    bp.out_codes   = r.rjoin.as<uint32_t>();
    bp.run_cnt     = r.rrun.as<uint32_t>();
    bp.run_off     = r.rrun.as<uint32_t>() + s.sweeps_max * s.NSUB;
    return bp;
}

// k_probe / k_probe_bitj over S's lists; no slices, no counter, no chunk positions, 32-bit codes
ProbeParams Engine::probe_params(const Geometry& g, const JoinShape& s) const {
    ProbeParams pp{};
    pp.g               = g;
    pp.tabs            = d_tabs_;
    pp.pool            = S_.pool.as<uint32_t>();
    pp.list            = S_.list.as<uint32_t>();
    pp.list_start      = S_.lstart.as<uint32_t>();
    pp.item_start      = S_.istart.as<uint32_t>();
    pp.surv            = surv.as<uint32_t>();
    pp.surv_seg_stride = s.seg_stride();
    pp.surv_cnt        = survcnt.as<uint32_t>();
    pp.surv_off        = survoff.as<uint32_t>();
    pp.job_surv        = jparts.as<uint32_t>() + s.NJ;
    return pp;
}

// k_join over the build's and the probe's runs, its partial sums in the ring slot; 32-bit codes
JoinParams Engine::join_params(const RSide& r, const Geometry& g, const JoinShape& s, char* slot, int jkind) const {
    JoinParams jp{};
    jp.r_codes         = r.rjoin.as<uint32_t>();
    jp.r_sweep_start   = r.R.istart.as<uint32_t>();
    jp.r_cnt           = r.rrun.as<uint32_t>();
    jp.r_off           = r.rrun.as<uint32_t>() + s.sweeps_max * s.NSUB;
    jp.slot            = (uint32_t) s.SLOT;
    jp.surv            = surv.as<uint32_t>();
    jp.surv_cnt        = survcnt.as<uint32_t>();
    jp.surv_off        = survoff.as<uint32_t>();
    jp.item_start      = S_.istart.as<uint32_t>();
    jp.list_start      = S_.lstart.as<uint32_t>();
    jp.surv_seg_stride = s.seg_stride();
    jp.nseg            = s.nseg;
    jp.CH              = s.CH;
    jp.log2NSUB        = g.log2NSUB;
    jp.hash_shift      = g.hash_shift;
    jp.bitmap          = join_uses_bitmap(g) ? 1u : 0u;
    jp.jsum            = (uint64_t*) (slot + 128);  // 64 partial sums, one per 128-B line
    jp.nparts          = jparts.as<uint32_t>();
    jp.extra           = jtask.as<uint2>();
    jp.nextra          = jparts.as<uint32_t>() + 2 * s.NJ;
    jp.jkind           = (uint32_t) jkind;
    jp.split_surv      = test_hooks().join_split;  // (tests: force the skew split)
    jp.timing          = phase_ev_ ? 1u : 0u;      // (back-to-back joins: counts only)
    return jp;
}

// what the jobs of the payload joins share with k_join's (xcd8: the launch wrappers)
static JobInputs job_inputs(const JoinParams& jp, const uint32_t* surv_pos) {
    JobInputs ji{};
    ji.r_codes = jp.r_codes, ji.r_sweep_start = jp.r_sweep_start, ji.r_cnt = jp.r_cnt, ji.r_off = jp.r_off;
    ji.slot = jp.slot, ji.surv = jp.surv, ji.surv_pos = surv_pos, ji.surv_cnt = jp.surv_cnt, ji.surv_off = jp.surv_off;
    ji.item_start = jp.item_start, ji.list_start = jp.list_start, ji.surv_seg_stride = jp.surv_seg_stride;
    ji.nseg = jp.nseg, ji.CH = jp.CH, ji.log2NSUB = jp.log2NSUB, ji.hash_shift = jp.hash_shift;
    return ji;
}

// ------------------------------------------------------------------- Engine::enqueue
// The host sequence behind every single-GPU join (JoinReq), stage by stage: validate, plan, ensure
// buffers, take the ring slot, the S pass / R pass / build in their order rules (passes), probe, the
// kind's join stage, finish.

// 1. The refusals, in this order (the C ABI tests pin codes and messages), and the geometry.
int Engine::validate(JoinCtx* c) {
    const JoinReq& q  = c->q;
    const JoinIn&  in = c->in;
    if (q.jkind < 0 || q.jkind > 2) {
        set_last_error("unknown per-partition join algorithm");
        return 2;
    }
    HWBRJ_CHECK(hipSetDevice(device_));
    tab_.state = kTabNone;  // (buffers may grow or be rewritten from here on: tables_read)
    const bool group = q.kind == JOIN_GROUP;
    if (q.layout != SRC_TUPLES && q.layout != SRC_KEYS) {
        set_last_error("relations are tuples or key columns");
        return 2;
    }
    if (q.layout == SRC_KEYS && group && in.nS && !q.s_val) {
        set_last_error("key columns: a group join needs S's value column");
        return 2;
    }
    // (hwbrj_api.cpp refuses first; a group join produces no S row index, so S is not held to 2^31)
    if (q.layout == SRC_KEYS && q.carries_s_payloads() &&
        (in.nR >= (1ull << 31) || (!group && in.nS >= (1ull << 31)))) {
        set_last_error("key columns: row indices are int32 (|R|, |S| < 2^31)");
        return 3;
    }
    c->vR = in.nR ? q.masks.r : nullptr;
    c->vS = in.nS ? q.masks.s : nullptr;
    c->vV = in.nS ? q.masks.sv : nullptr;
    const bool masked = c->vR || c->vS || c->vV;
    if (masked && q.layout != SRC_KEYS) {
        set_last_error("validity bitmaps: key columns");
        return 2;
    }
    if (c->vV && !group) {
        set_last_error("validity bitmaps: a value column's belongs to the group joins");
        return 2;
    }
    std::string err;
    if (c->b) {  // (a probe: the build's geometry, planned and found supported when it was made)
        c->g = c->b->r.g;
    } else if (!plan_geometry(in.args, in.nR, &c->g, &err, q.carries_s_payloads())) {
        set_last_error(err);
        return 2;
    }
    if (masked && !masks_supported(c->g)) {  // (hwbrj_api.cpp refuses first, before any device call)
        set_last_error("validity bitmaps need partition slices (blocked/sectorized, basic k = 1, or no filter)");
        return kRcMaskFilter;
    }
    if (q.carries_s_payloads() && c->g.mode == MODE_GLOBAL) {
        set_last_error("global-bitmap mode: materialized by the side pass");
        return kRcMatGlobal;
    }
    return 0;
}

// 2. The shape, and whether this join is a collective.
void Engine::plan(JoinCtx* c) {
    const Geometry& g  = c->g;
    const bool      pl = c->q.carries_s_payloads();
    const uint32_t  F = 1u << g.log2F, NSUB = 1u << g.log2NSUB;
    const bool      slice_mode = g.mode == MODE_SLICE_BLOCK || g.mode == MODE_SLICE_BASIC;
    const size_t    sc_lds     = pl ? scatter_pay_lds_bytes(g.log2F) : scatter_lds_bytes(g.log2F);
    const uint32_t  G          = (uint32_t) cus_ * wg_per_cu(sc_lds);
    // basic k >= 2: the S-side buffers first partition the R keys' k * |R| bit positions
    c->basic_kk = g.mode == MODE_SLICE_BASIC && g.k > 1;
    c->nRk      = c->basic_kk ? (uint64_t) g.k * c->in.nR : 0;
    c->s = JoinShape::make(F, NSUB, F * NSUB, slice_mode ? g.nseg : 1, G, region_cap(c->in.nR, G, F),
                           region_cap(std::max(c->in.nS, c->nRk), G, F), slice_mode);
    // a probe: capR, and with it the sweeps' layout of rrun, are the build's; capS from this batch
    if (c->b) {
        const JoinShape& r = c->b->r.s;
        c->s = JoinShape::make(r.F, r.NSUB, r.NJ, r.nseg, r.G, r.capR, region_cap(c->in.nS, r.G, r.F), r.slice_mode);
    }
    // the north_star's bitmap broadcast (opt-in, hwbrj_set_filter_broadcast) makes this join a
    // collective: from here on a failure of this rank alone must not leave its peers waiting in
    // ncclBroadcast, so every return before the first kernel goes through one status agreement
    // (enqueue's pre(); argument errors before it fail alike on every rank)
    c->bcast = bcast_ && comm_ && slice_mode && !c->basic_kk && !c->b;  // (a build's slices are always local)
}

// b: a probe of a prepared build (Build). The same stages over the build's RSide instead of the
// Engine's own, without the R side: the shape takes capR from the build, only the S side and the job
// table are ensured, the S scatter carries the ring slot's zeroing, and the tables are not read back.
int Engine::enqueue(const JoinIn& in, const JoinReq& req, const Build* b) {
    JoinCtx c{in, req};
    c.b  = b;
    c.rs = b ? &b->r : &rs_;
    if (const int rc = validate(&c)) return rc;
    // Every join on this device shares this Engine's scratch (pools, lists, slices, counters):
    // a join enqueued on another stream than a still-pending one must run after it (on the same
    // stream, stream order does it: no wait packet between back-to-back joins).
    if (!c.in.stream) c.in.stream = own_stream_;
    if (pending_ && c.in.stream != pending_stream_) HWBRJ_CHECK(hipStreamWaitEvent(c.in.stream, ev_[8], 0));
    if (!b && !req.carries_s_payloads() && c.g.mode == MODE_SLICE_BASIC && c.g.k > 1 &&
        (uint64_t) c.g.k * in.nR <= (1ull << 31))
        return enqueue_basic_kk(c.in, c.g, req);
    plan(&c);
    auto pre = [&](int rc) -> int {
        if (!c.bcast || alloc_only_) return rc;
        return rccl_agree_status(comm_, comm_world_, comm_rank_, rc, c.in.stream, &agree_);
    };
    if (const char* why = shape_limits(c.s, req)) {
        set_last_error(why);
        return pre(3);
    }
    if (!ensure_buffers(&c)) {
        set_last_error("hipMalloc failed (device memory)");
        return pre(4);
    }
    if (alloc_only_) return 0;
    if (const int rc = pre(0)) return rc;
    // this join's result slot (ring_take collects a full ring first)
    if (!(c.sm = (char*) ring_take(&c.rslot))) return 1;
    if (const int rc = passes(&c)) return rc;
    ProbeParams pp;
    if (const int rc = probe(c, &pp)) return rc;
    JoinParams jp = join_params(*c.rs, c.g, c.s, c.sm, req.jkind);
    jp.r_kbits    = c.kbits;
    jp.fmt_cnt    = pp.fmt_cnt;
    const JobInputs ji = job_inputs(jp, survpos.as<uint32_t>());
    int rc = 0;
    switch (req.kind) {
        case JOIN_COUNT: rc = join_count(c, jp); break;
        case JOIN_PAIRS: rc = join_pairs(c, ji); break;
        case JOIN_SEMI: rc = join_semi(c, ji); break;
        case JOIN_OUTER: rc = join_outer(c, ji); break;
        case JOIN_GROUP: rc = join_group(c, ji); break;
    }
    if (rc) return rc;
    TabRec t;  // the shape of this join's tables (tables_info / tables_read)
    // (the existence / outer / group join's tables: not read back)
    // nor a probe's: R's tables are the build's
    t.state = !b && (req.kind == JOIN_COUNT || req.kind == JOIN_PAIRS) ? kTabJoin : kTabOther;
    t.mat   = req.carries_r_payloads();
    t.s     = c.s;
    (void) probe_lds_bytes(c.g, &t.stage_cap, req.carries_s_payloads());
    t.jkind  = (uint32_t) req.jkind;
    t.kbits  = c.kbits;
    t.bitmap = t.mat ? (pay_bitmap(c.g) ? 1u : 0u) : jp.bitmap;
    t.split  = jp.split_surv;
    JoinRec r;
    r.slot     = c.rslot;
    r.fmt      = pp.fmt_cnt != nullptr;
    r.kbits    = c.kbits;
    r.slots    = !req.carries_s_payloads();  // (the matches are in k_join's partial sums)
    r.timed    = c.rtimed;
    r.s_masked = c.vS != nullptr || c.vV != nullptr;
    return finish(c.in, c.g, c.s_first, t, r, b != nullptr);
}

// 8. The epilogue of both enqueue paths: the join's completion event, what wait() and the next
// enqueue need of it, its tables' shape and its record in the ring.
// prepared: a probe's filter belongs to its build, so export_filter finds none.
int Engine::finish(const JoinIn& in, const Geometry& g, bool s_first, const TabRec& tab, JoinRec rec, bool prepared) {
    HWBRJ_CHECK(hipEventRecord(ev_[8], in.stream));
    HWBRJ_CHECK(hipGetLastError());
    pending_        = true;
    pending_rc_     = 0;
    pending_ev_     = phase_ev_;
    pending_sfirst_ = s_first;
    pending_prepared_ = prepared;
    pending_stream_ = in.stream;
    have_filter_    = in.args != nullptr && !prepared;
    last_g_         = g;
    tab_            = tab;
    tab_.sync       = phase_ev_;
    tab_.g          = g;
    rec.args = in.args != nullptr;
    rec.nS   = in.nS;
    rec.g    = g;
    jr_.push_back(rec);
    return 0;
}

// S pass-1 and its lists (async joins: on a second stream, concurrent with the R side). It starts
// from a clear block: no zeroing (the R scatter's alone), and the shared slot of seg_cnt / src_val /
// valid holds only what this source reads.
// (a group join on key columns with a bitmap on S: the value-column scatter's masked form, one
// bitmap or both, whichever column they belong to: vmask = {vS ? vS : vV, vS ? vV : nullptr})
int Engine::s_pass(const JoinCtx& c, hipStream_t st, bool marks, hipEvent_t* tev) {
    const Geometry&  g  = c.g;
    // what the S payload scatter reads: the layout, or S's key column with its value column
    const int        layout_s   = c.q.layout == SRC_KEYS && c.q.kind == JOIN_GROUP ? SRC_KEYS_VAL : c.q.layout;
    const bool       val_masked = layout_s == SRC_KEYS_VAL && (c.vS || c.vV);
    ScatterValParams ss{};
    (ScatterParams&) ss = scatter_params(g, S_, c.s.capS);
    ss.vmask[0] = !val_masked ? nullptr : c.vS ? c.vS : c.vV;
    ss.vmask[1] = val_masked && c.vS ? c.vV : nullptr;
    ss.n        = c.in.nS;
    if (g.mode == MODE_GLOBAL) {
        launch_probe_global(c.in.dS, c.q.layout, c.in.nS, g, d_tabs_, bitmap.as<uint32_t>(), dense.as<uint32_t>(),
                            c.result() + 1, st);
        ss.src   = dense.p;
        ss.n_dev = c.result() + 1;
    } else {
        ss.src = c.in.dS;
        if (layout_s == SRC_KEYS_VAL) ss.src_val = c.q.s_val;  // (shares seg_cnt's slot: not SRC_CODES)
        else if (c.vS) ss.valid = c.vS;                          // (the same slot: never both)
    }
    ss.ppool = c.q.carries_s_payloads() ? ppoolS.as<uint32_t>() : nullptr;
    if (c.b) {  // a probe has no R scatter: this one's workgroup 0 zeroes the slot's counts and the extra-task count
        ss.zero_small = (uint32_t*) c.sm;
        ss.zero_word  = jparts.as<uint32_t>() + 2 * c.s.NJ;
    }
    if (tev) HWBRJ_CHECK(hipEventRecord(tev[0], st));
    launch_scatter(ss, g.mode == MODE_GLOBAL ? SRC_CODES : val_masked ? SRC_KEYS_VAL_MASK : c.vS ? SRC_KEYS_MASK : layout_s,
                   SIDE_S, c.s.G, st);
    if (tev) HWBRJ_CHECK(hipEventRecord(tev[1], st));
    if (marks) HWBRJ_CHECK(mark(4, st));
    index_side(S_, c.s.capS, g.log2F, c.s.CH, c.s.nseg, c.s.G, st);
    if (marks) HWBRJ_CHECK(mark(5, st));
    return 0;
}

// R: pass-1 (+ filter), its lists, the build sweeps; then the slices' broadcast, or their build from
// bit positions (basic k >= 2).
// r: where it is left (the Engine's own RSide, or a build's); zero_small / zero_word: the join's
// zeroing the R scatter carries (a build: none, it is part of no join).
int Engine::r_side(const JoinCtx& c, RSide* r, uint32_t* zero_small, uint32_t* zero_word) {
    const Geometry&  g = c.g;
    const JoinShape& s = c.s;
    const JoinIn&    in = c.in;
    hipStream_t      stream = in.stream;
    const bool       rpay_on = c.q.carries_r_payloads();
    if (g.mode == MODE_GLOBAL)
        launch_build_global(in.dR, c.q.layout, in.nR, g, d_tabs_, bitmap.as<uint32_t>(), stream);
    // zeroing (the reference callocs before its timer, :1583, :1601): the counts and the join's
    // extra-task count are zeroed by this scatter's workgroup 0 (two memset dispatches less per join)
    ScatterParams sp = scatter_params(g, r->R, s.capR);
    sp.src        = in.dR;
    sp.n          = in.nR;
    sp.ppool      = rpay_on ? r->ppoolR.as<uint32_t>() : nullptr;
    sp.zero_small = zero_small;
    sp.zero_word  = zero_word;
    if (c.vR) sp.valid = c.vR;
    launch_scatter(sp, c.vR ? SRC_KEYS_MASK : c.q.layout, SIDE_R, s.G, stream);
    HWBRJ_CHECK(mark(1, stream));
    index_side(r->R, s.capR, g.log2F, (uint32_t) s.BSW, 1, s.G, stream);
    HWBRJ_CHECK(mark(2, stream));
    BuildParams bp = build_params(*r, g, s);
    bp.slices  = s.slice_mode ? r->slices.as<uint32_t>() : nullptr;
    bp.ppool   = rpay_on ? r->ppoolR.as<uint32_t>() : nullptr;
    bp.out_pay = rpay_on ? r->rpay.as<uint32_t>() : nullptr;
    bp.kbits   = c.kbits;
    // the broadcast: rank 0 builds the slices, the other ranks only sub-partition R for the join
    // and receive them over RCCL (HWBRJ_HOOK_BCAST_NONROOT: this rank takes the non-root side, for
    // tests at world 1; value 2 zeroes the slices first, so the counts show whether k_build wrote any)
    const int nonroot_hook = c.bcast && comm_world_ == 1 ? test_hooks().bcast_nonroot : 0;  // (tests only: world 1)
    bp.no_slices = c.bcast && (comm_rank_ != 0 || nonroot_hook) ? 1u : 0u;
    if (nonroot_hook == 2) HWBRJ_CHECK(hipMemsetAsync(slices.p, 0, slices.bytes, stream));
    launch_build(bp, s.F, stream);
    if (c.bcast) {
        const int rc = rccl_broadcast(comm_, slices.p, (size_t) s.F * s.nseg * g.seg_words * 4, 0, stream);
        if (rc) {  // kernels of this join are enqueued: later joins must still order after them
            (void) hipEventRecord(ev_[8], stream);
            pending_        = true;
            pending_stream_ = stream;
            pending_rc_     = rc;
            pending_err_    = hwbrj_last_error();
            return rc;
        }
    }
    if (c.basic_kk) {
        // basic k >= 2: the k bit positions of every R key, partitioned by slice with the S-side
        // scatter buffers (free until the S pass), then one LDS slice build per partition
        launch_bitpos(in.dR, c.q.layout, in.nR, g, bpos.as<uint32_t>(), stream);
        ScatterParams sb = scatter_params(g, S_, s.capS);  // (a clear block: seg_cnt's slot is read)
        sb.src = bpos.p;
        sb.n   = c.nRk;
        launch_scatter(sb, SRC_CODES, SIDE_R, s.G, stream);
        index_side(S_, s.capS, g.log2F, (uint32_t) s.BSW, 1, s.G, stream);
        launch_slice_fill(S_.pool.as<uint32_t>(), S_.list.as<uint32_t>(), S_.lstart.as<uint32_t>(), g,
                          slices.as<uint32_t>(), stream);
    }
    HWBRJ_CHECK(mark(3, stream));
    return 0;
}

// 5. The S pass, the R side and the build, in their order rules.
int Engine::passes(JoinCtx* c) {
    const Geometry& g      = c->g;
    hipStream_t     stream = c->in.stream;
    const bool      pl     = c->q.carries_s_payloads();
    // job_surv is left zero by every counting join's k_join_split, so the job table is cleared only when new
    if (c->jnew) HWBRJ_CHECK(hipMemsetAsync(jparts.p, 0, jparts.bytes, stream));
    if (g.mode == MODE_GLOBAL) HWBRJ_CHECK(hipMemsetAsync(bitmap.p, 0, bitmap.bytes, stream));
    // 3-byte join keys from build / probe to k_join, unless the last join this Engine waited for had
    // probe items too large for the stage (their 32-bit survivor runs make the join read two formats,
    // k_join_mixed): a performance hint only, both paths give the same counts
    c->kbits = !pl && join_pack3(g) && pack3_hint_ ? join_key_bits(g) : 0u;  // 18 at the north star
    if (c->b) c->kbits = c->b->r.kbits;  // (a build's packing was decided when it was made)
    HWBRJ_CHECK(mark(0, stream));
    if (c->b) {  // a probe: the S pass alone (wait_common gives the R phases 0)
        c->s_first = true;
        return s_pass(*c, stream, true, nullptr);
    }
    const bool ovl = HWBRJ_OVL_ASYNC && !phase_ev_ && g.mode != MODE_GLOBAL && !c->basic_kk && !pl && !c->bcast;
    if (ovl) {  // S pass on the side stream (with phase events, its phases would show inside the R side's)
        if (!ovl_stream_) {
            HWBRJ_CHECK(hipStreamCreateWithFlags(&ovl_stream_, hipStreamNonBlocking));
            HWBRJ_CHECK(hipEventCreateWithFlags(&ovl_ev_[0], hipEventDisableTiming));
            HWBRJ_CHECK(hipEventCreateWithFlags(&ovl_ev_[1], hipEventDisableTiming));
        }
        HWBRJ_CHECK(hipEventRecord(ovl_ev_[0], stream));
        HWBRJ_CHECK(hipStreamWaitEvent(ovl_stream_, ovl_ev_[0], 0));
        // (opt-in, hwbrj_set_async_timing: the S scatter bracketed by timing events on the side
        // stream, so the dominant kernel is timed in the schedule the back-to-back joins run)
        hipEvent_t* tev = nullptr;
        if (async_timing_) {
            for (int i = 0; i < 2; i++)
                if (!tev_[c->rslot][i]) HWBRJ_CHECK(hipEventCreateWithFlags(&tev_[c->rslot][i], hipEventDisableSystemFence));
            tev = tev_[c->rslot];
        }
        c->rtimed = tev != nullptr;
        if (const int rc = s_pass(*c, ovl_stream_, false, tev)) return rc;
        HWBRJ_CHECK(hipEventRecord(ovl_ev_[1], ovl_stream_));
    }
    // The S pass runs first: then the filter slices (written by k_build) and the R pool (written by
    // k_scatter_r) are the most recent writes when k_probe and k_build read them, so the Infinity
    // Cache still holds much of them. Not in the global mode (the R scatter's workgroup 0 zeroes the
    // dense count the S pass's global probe adds to) nor for basic k >= 2 (the R side borrows the
    // S-side buffers).
    c->s_first = !ovl && g.mode != MODE_GLOBAL && !c->basic_kk;
    if (c->s_first)
        if (const int rc = s_pass(*c, stream, true, nullptr)) return rc;
    if (const int rc = r_side(*c, &rs_, (uint32_t*) c->sm, jparts.as<uint32_t>() + 2 * c->s.NJ)) return rc;
    if (ovl) {
        HWBRJ_CHECK(hipStreamWaitEvent(stream, ovl_ev_[1], 0));
        HWBRJ_CHECK(mark(4, stream));
        HWBRJ_CHECK(mark(5, stream));
    } else if (!c->s_first) {
        if (const int rc = s_pass(*c, stream, true, nullptr)) return rc;
    }
    return 0;
}

// 6. The probe (survivor sub-partitioning is fused into k_probe: no ev_[7]).
int Engine::probe(const JoinCtx& c, ProbeParams* pp) {
    const bool pl = c.q.carries_s_payloads();
    *pp           = probe_params(c.g, c.s);
    pp->slices    = c.s.slice_mode ? c.rs->slices.as<uint32_t>() : nullptr;
    pp->filtered  = c.result() + 2;
    pp->surv_pos  = pl ? survpos.as<uint32_t>() : nullptr;
    pp->kbits     = c.kbits;
    pp->fmt_cnt   = pl ? nullptr : (uint32_t*) c.sm + 10;  // (u64 word 5 of the slot: zeroed by the R scatter)
    launch_probe(*pp, (uint32_t) cus_ * wg_per_cu(probe_lds_bytes(c.g, nullptr, pl)), c.in.stream);
    HWBRJ_CHECK(mark(6, c.in.stream));
    surv_fused_ = true;
    return 0;
}

// 7. The join stage, by kind: each owns its memsets, its emit kernel and its NULL-row kernels. Rows
// and matches are counted in word 0 of the ring slot.
int Engine::join_count(const JoinCtx& c, const JoinParams& jp) {
    launch_join(jp, c.s.NJ, jparts.as<uint32_t>() + c.s.NJ, c.in.stream);
    return 0;
}

// (k_join_split, which leaves job_surv zero for the next join, runs in no payload join)
int Engine::clear_job_surv(const JoinCtx& c) {
    HWBRJ_CHECK(hipMemsetAsync(jparts.as<uint32_t>() + c.s.NJ, 0, (size_t) c.s.NJ * 4, c.in.stream));
    return 0;
}

MatJoinParams Engine::mat_params(const JoinCtx& c, const JobInputs& ji) const {
    MatJoinParams mp{};
    mp.j     = ji;
    mp.r_pay = c.rs->rpay.as<uint32_t>();
    mp.bm    = pay_bitmap(c.g) ? 1u : 0u;
    mp.s_pay = ppoolS.as<uint32_t>();
    mp.out   = c.q.kind == JOIN_GROUP ? nullptr : (uint2*) c.q.out;  // (k_join_group has its own)
    mp.cap   = c.q.cap;
    mp.count = (unsigned long long*) c.result();
    return mp;
}

int Engine::join_pairs(const JoinCtx& c, const JobInputs& ji) {
    if (const int rc = clear_job_surv(c)) return rc;
    launch_join_mat(mat_params(c, ji), c.s.NJ, c.in.stream);
    return 0;
}

int Engine::join_semi(const JoinCtx& c, const JobInputs& ji) {
    const JoinReq& q      = c.q;
    hipStream_t    stream = c.in.stream;
    const bool     marks  = semi_marks(c.g, q);
    uint2*         out    = (uint2*) q.out;
    if (const int rc = clear_job_surv(c)) return rc;
    if (marks) HWBRJ_CHECK(hipMemsetAsync(smark.p, 0, c.s.LS * 4, stream));
    SemiJoinParams sj{};
    sj.j     = ji;
    sj.bm    = pay_bitmap(c.g) ? 1u : 0u;
    sj.anti  = q.anti ? 1u : 0u;
    sj.basic = c.g.mode == MODE_SLICE_BASIC ? 1u : 0u;
    sj.s_pay = ppoolS.as<uint32_t>();
    sj.mark  = marks ? smark.as<uint32_t>() : nullptr;
    sj.tabs  = d_tabs_;
    sj.out   = out;
    sj.cap   = q.cap;
    sj.count = (unsigned long long*) c.result();
    launch_join_semi(sj, c.s.NJ, stream);
    if (!q.anti) return 0;
    // every unmarked S tuple: the filter's rejects and the unmatched survivors
    SemiEmitParams se{};
    se.pool       = S_.pool.as<uint32_t>();
    se.ppool      = ppoolS.as<uint32_t>();
    se.list       = S_.list.as<uint32_t>();
    se.list_start = S_.lstart.as<uint32_t>();
    se.mark       = smark.as<uint32_t>();
    se.g          = c.g;
    se.tabs       = d_tabs_;
    se.out        = out;
    se.cap        = q.cap;
    se.count      = sj.count;
    launch_semi_emit(se, (uint32_t) cus_ * 2, stream);
    if (c.vS)  // a NULL key has no partner: {the stored key, row}
        launch_null_rows(NullRowsParams{c.vS, (const uint32_t*) c.in.dS, c.in.nS, NULL_ROWS_ANTI, 0u, out, q.cap,
                                        sj.count, nullptr},
                         (uint32_t) cus_ * 2, stream);
    return 0;
}

int Engine::join_outer(const JoinCtx& c, const JobInputs& ji) {
    const JoinReq& q      = c.q;
    hipStream_t    stream = c.in.stream;
    uint2*         out    = (uint2*) q.out;
    if (const int rc = clear_job_surv(c)) return rc;
    if (q.keep_s) HWBRJ_CHECK(hipMemsetAsync(smark.p, 0, c.s.LS * 4, stream));
    // the class counters: u64 words 6 (R-only) and 7 (S-only) of the slot (last_slot_); inner = rows - both
    unsigned long long* rows = (unsigned long long*) c.result();
    unsigned long long* cls  = rows + 6;
    OuterJoinParams     op{};
    op.m        = mat_params(c, ji);
    op.keep_s   = q.keep_s ? 1u : 0u;
    op.keep_r   = q.keep_r ? 1u : 0u;
    op.null_pay = q.null_pay;
    op.mark     = q.keep_s ? smark.as<uint32_t>() : nullptr;
    op.n_r_only = cls;
    if (q.rmark) launch_join_outer_mark(OuterMarkParams{op, q.rmark}, c.s.NJ, stream);
    else launch_join_outer(op, c.s.NJ, stream);
    if (q.keep_s) {  // every unmarked S tuple: the filter's rejects and the unmatched survivors
        OuterEmitParams oe{};
        oe.ppool      = ppoolS.as<uint32_t>();
        oe.list       = S_.list.as<uint32_t>();
        oe.list_start = S_.lstart.as<uint32_t>();
        oe.mark       = smark.as<uint32_t>();
        oe.log2F      = c.g.log2F;
        oe.null_pay   = q.null_pay;
        oe.out        = out;
        oe.cap        = q.cap;
        oe.count      = rows;
        oe.n_s_only   = cls + 1;
        launch_outer_emit(oe, (uint32_t) cus_ * 2, stream);
    }
    // NULL keys: S-only and R-only rows of the sides that are kept
    if (q.keep_s && c.vS)
        launch_null_rows(NullRowsParams{c.vS, nullptr, c.in.nS, NULL_ROWS_S, q.null_pay, out, q.cap, rows, cls + 1},
                         (uint32_t) cus_ * 2, stream);
    if (q.keep_r && c.vR)
        launch_null_rows(NullRowsParams{c.vR, nullptr, c.in.nR, NULL_ROWS_R, q.null_pay, out, q.cap, rows, cls},
                         (uint32_t) cus_ * 2, stream);
    return 0;
}

int Engine::join_group(const JoinCtx& c, const JobInputs& ji) {
    const JoinReq& q = c.q;
    if (const int rc = clear_job_surv(c)) return rc;
    GroupJoinParams gp{};
    gp.m       = mat_params(c, ji);
    gp.all     = q.all ? 1u : 0u;
    gp.agg     = q.agg;
    gp.out     = (uint4*) q.out;
    gp.n_pairs = (unsigned long long*) c.result() + 6;  // the pair counter: u64 word 6 of the slot (last_slot_)
    if (q.gacc) {
        // the accumulating probe: the same jobs fold into the build's entries and write no row. A NULL
        // R row is in no partition, so its entry keeps the identity row it was initialised with
        launch_join_group_acc(GroupAccParams{gp, q.gacc}, c.s.NJ, c.in.stream);
        return 0;
    }
    launch_join_group(gp, c.s.NJ, c.in.stream);
    // NULL keys of R are in no partition, so no job saw them: under ALL their identity rows come
    // from here, through the same row counter
    if (q.all && c.vR)
        launch_null_group_rows(NullGroupRowsParams{c.vR, c.in.nR, q.agg, gp.out, q.cap, gp.m.count},
                               (uint32_t) cus_ * 2, c.in.stream);
    return 0;
}

// Basic k >= 2. A key's k bits lie in k unrelated slices, so the S words are
// tested one bit per pass: pass j partitions the candidates by the slice of their bit j and tests
// it in LDS (k_probe_bitj), the passing words (dense) feed pass j + 1's scatter. The survivors of
// the last pass are re-partitioned by code (MODE_CODE_OF_KEY), the join's layout, so the join
// takes its bitmap path like the blocked filter's: R is partitioned by code for the join, and the
// slices are built from R's partitioned bit positions (k_bitpos, k_slice_fill).
int Engine::enqueue_basic_kk(const JoinIn& in, const Geometry& g, const JoinReq& req) {
    const void *   dR = in.dR, *dS = in.dS;
    const uint64_t nR = in.nR, nS = in.nS;
    hipStream_t    stream = in.stream;
    const int      layout = req.layout;
    Geometry       gj;  // the join layout: R and the survivors partitioned by code
    std::string    err;
    if (!plan_geometry(nullptr, nR, &gj, &err)) {
        set_last_error(err);
        return 2;
    }
    const uint32_t F = 1u << g.log2F, Fj = 1u << gj.log2F, Fm = std::max(F, Fj);
    const uint32_t NSUB = 1u << gj.log2NSUB, nseg = g.nseg, CH = probe_chunks_per_item();
    // one workgroup per CU for every scatter and bit pass: pass j's workgroup w writes region w
    // (rw words) and pass j + 1's scatter workgroup w partitions it
    const uint32_t G    = (uint32_t) cus_;
    const uint64_t nRk  = (uint64_t) g.k * nR;
    const uint64_t Ib   = ((nS / 32 + (uint64_t) G * (Fm + 1)) / CH + Fm + 1) * nseg;  // items of a pass
    const uint64_t rw   = ((Ib + G - 1) / G) * CH * 32;  // words a pass workgroup may append
    // the buffers hold the larger of the filter's and the join's partition counts; the jobs are the join's
    const JoinShape s = JoinShape::make(Fm, NSUB, Fj * NSUB, nseg, G, region_cap(nR, G, Fm),
                                        std::max(region_cap(std::max(nS, nRk), G, Fm), rw / 32 + Fm + 1), true);
    const uint64_t capR = s.capR, capS = s.capS, BSW = s.BSW;
    if (const char* why = shape_limits(s, req)) {
        set_last_error(why);
        return 3;
    }
    bool jnew = false;
    bool ok   = ensure_common(s, 1, &jnew);
    ok = ok && slices.ensure((uint64_t) F * nseg * g.seg_words * 4) && (g.k <= G || bpos.ensure(nRk * 4));
    const uint32_t NC = (g.k + 64) & ~63u;  // pass counters [0, k - 1) + the dummy [NC - 1]
    ok = ok && dense.ensure(G * rw * 4) && dense2.ensure(G * rw * 4) && kkcnt.ensure(NC * 8 + 2 * G * 4);
    if (!ok) {
        set_last_error("hipMalloc failed (device memory)");
        return 4;
    }
    if (alloc_only_) return 0;
    uint32_t  rslot      = 0;
    char*     sm         = (char*) ring_take(&rslot);
    if (!sm) return 1;
    uint64_t* d_filtered = (uint64_t*) sm + 2;
    uint64_t* cnt        = kkcnt.as<uint64_t>();  // [j]: candidates after pass j (j < k - 1); [NC - 1]: dummy
    uint32_t* wgc[2]     = {(uint32_t*) (cnt + NC), (uint32_t*) (cnt + NC) + G};  // per-workgroup counts
    HWBRJ_CHECK(hipMemsetAsync(sm, 0, 64, stream));
    HWBRJ_CHECK(hipMemsetAsync(kkcnt.p, 0, kkcnt.bytes, stream));
    if (jnew) HWBRJ_CHECK(hipMemsetAsync(jparts.p, 0, jparts.bytes, stream));
    HWBRJ_CHECK(hipMemsetAsync(jparts.as<uint32_t>() + 2 * s.NJ, 0, 4, stream));

    HWBRJ_CHECK(mark(0, stream));
    // ---------------------------------------------------------------- R: the join layout
    ScatterParams sp = scatter_params(gj, R_, capR);
    sp.src = dR;
    sp.n   = nR;
    launch_scatter(sp, layout, SIDE_R, G, stream);
    HWBRJ_CHECK(mark(1, stream));
    index_side(R_, capR, gj.log2F, (uint32_t) BSW, 1, G, stream);
    HWBRJ_CHECK(mark(2, stream));
    launch_build(build_params(rs_, gj, s), Fj, stream);
    // ---------------------------------------------------------------- the filter slices
    if (g.k <= G) {  // R's k bit positions partitioned by slice straight from the tuples
        Geometry gp = g;
        gp.mode     = MODE_BASIC_POS;
        sp          = scatter_params(gp, S_, capS);
        sp.src      = dR;
        sp.n        = nRk;
        sp.vn       = nR;
        launch_scatter(sp, layout, SIDE_R, G, stream);
    } else {
        launch_bitpos(dR, layout, nR, g, bpos.as<uint32_t>(), stream);
        sp     = scatter_params(g, S_, capS);
        sp.src = bpos.p;
        sp.n   = nRk;
        launch_scatter(sp, SRC_CODES, SIDE_R, G, stream);
    }
    index_side(S_, capS, g.log2F, (uint32_t) BSW, 1, G, stream);
    launch_slice_fill(S_.pool.as<uint32_t>(), S_.list.as<uint32_t>(), S_.lstart.as<uint32_t>(), g,
                      slices.as<uint32_t>(), stream);
    HWBRJ_CHECK(mark(3, stream));
    // ---------------------------------------------------------------- S: by the slice of bit 0
    sp     = scatter_params(g, S_, capS);
    sp.src = dS;
    sp.n   = nS;
    launch_scatter(sp, layout, SIDE_S, G, stream);
    HWBRJ_CHECK(mark(4, stream));
    index_side(S_, capS, g.log2F, CH, nseg, G, stream);
    HWBRJ_CHECK(mark(5, stream));
    // ---------------------------------------------------------------- one bit per pass
    ProbeParams pb = probe_params(g, s);  // (k_probe_bitj reads the lists, the slices and what a pass sets)
    pb.slices      = slices.as<uint32_t>();
    uint32_t* dz[2] = {dense.as<uint32_t>(), dense2.as<uint32_t>()};
    for (uint32_t j = 0; j < g.k; j++) {
        Geometry gb = g;
        gb.bitj     = j;
        if (j > 0) {  // the candidates of pass j - 1, by the slice of bit j
            gb.mode       = MODE_BASIC_BITJ;
            sp            = scatter_params(gb, S_, capS);
            sp.src        = dz[(j - 1) & 1];
            sp.seg_cnt    = wgc[(j - 1) & 1];
            sp.seg_stride = rw;
            launch_scatter(sp, SRC_CODES, SIDE_S, G, stream);
            index_side(S_, capS, g.log2F, CH, nseg, G, stream);
        }
        pb.g               = gb;
        pb.surv            = dz[j & 1];
        pb.surv_seg_stride = rw;
        pb.wg_cnt          = wgc[j & 1];
        pb.filtered        = j + 1 < g.k ? cnt + j : d_filtered;
        launch_probe_bitj(pb, G, stream);
    }
    HWBRJ_CHECK(mark(6, stream));
    // ---------------------------------------------------------------- survivors: the join layout
    {
        Geometry gc = gj;
        gc.mode     = MODE_CODE_OF_KEY;
        sp            = scatter_params(gc, S_, capS);
        sp.src        = dz[(g.k - 1) & 1];
        sp.seg_cnt    = wgc[(g.k - 1) & 1];
        sp.seg_stride = rw;
        launch_scatter(sp, SRC_CODES, SIDE_S, G, stream);
        index_side(S_, capS, gj.log2F, CH, 1, G, stream);
    }
    ProbeParams pp = probe_params(gj, s);
    pp.filtered    = cnt + NC - 1;  // (counted by the last bit pass)
    launch_probe(pp, (uint32_t) cus_ * wg_per_cu(probe_lds_bytes(gj, nullptr)), stream);
    HWBRJ_CHECK(mark(7, stream));
    surv_fused_ = false;
    // -------------------------------------------------------------------------- join
    JoinParams jp = join_params(rs_, gj, s, sm, req.jkind);
    jp.nseg       = 1;  // (the survivors were re-partitioned without segments)
    launch_join(jp, s.NJ, jparts.as<uint32_t>() + s.NJ, stream);
    TabRec t;
    t.state = kTabOther;  // (the repartitioning passes' tables: not read back)
    JoinRec r;
    r.slot  = rslot;
    r.slots = true;
    return finish(in, g, false, t, r);
}

// h = the six result words of a slot b; with slots, k_join's partial sums behind them added
static void slot_counts(const uint64_t* b, bool slots, uint64_t h[6]) {
    const size_t S = join_sum_slots(), W = join_sum_stride();
    for (int i = 0; i < 6; i++) h[i] = b[i];
    for (size_t j = 0; slots && j < S; j++) {
        h[0] += b[16 + j * W];
        h[3] += b[16 + j * W + 1];
        h[4] += b[16 + j * W + 2];
    }
}

int read_join_counts(const void* small, bool slots, hipStream_t stream, uint64_t h[6]) {
    std::vector<uint64_t> buf(16 + (slots ? join_sum_slots() * join_sum_stride() : 0));  // 128 bytes of result words, then the slots
    if (hipMemcpyAsync(buf.data(), small, buf.size() * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) {
        set_last_error("reading the join's counts failed");
        return 1;
    }
    slot_counts(buf.data(), slots, h);
    return 0;
}

void* Engine::ring_take(uint32_t* slot) {
    if (jr_.size() >= (size_t) kJoinRing && ring_collect()) return nullptr;
    *slot      = jr_next_;
    jr_next_   = (jr_next_ + 1) % kJoinRing;
    last_slot_ = (const uint64_t*) ((char*) jring_.p + (size_t) *slot * ring_slot_bytes());
    return (void*) last_slot_;
}

// The counts of every join in jr_ (all completed once ev_[8] has: they share the device's scratch,
// so each ran after the one before), read in one copy of the ring, appended to jdone_.
int Engine::ring_collect() {
    if (jr_.empty()) return 0;
    HWBRJ_CHECK(hipEventSynchronize(ev_[8]));
    const size_t          SB = ring_slot_bytes();
    std::vector<uint64_t> buf(kJoinRing * SB / 8);
    // the slots in use are consecutive mod kJoinRing: one copy of [first, last], or of the ring
    const uint32_t a = jr_.front().slot, z = jr_.back().slot;
    const size_t   off = a <= z ? (size_t) a * SB : 0, len = a <= z ? (size_t) (z - a + 1) * SB : kJoinRing * SB;
    HWBRJ_CHECK(hipMemcpy((char*) buf.data() + off, (char*) jring_.p + off, len, hipMemcpyDeviceToHost));
    for (const JoinRec& r : jr_) {
        uint64_t h[6];
        slot_counts(buf.data() + (size_t) r.slot * (SB / 8), r.slots, h);
        if (r.fmt) pack3_hint_ = (uint32_t) h[5] == 0;  // (k_probe's count, ProbeParams::fmt_cnt)
        const Geometry& g = r.g;
        hwbrj_stats_t   st;
        memset(&st, 0, sizeof(st));
        // (no filter: every S row survives, and k_probe's count is the valid rows of a masked S)
        st.filtered       = r.args || r.s_masked ? h[2] : r.nS;
        st.matches        = (int64_t) h[0];
        st.mode           = g.mode;
        st.format         = g.s_format;
        st.partitions     = 1u << g.log2F;
        st.subparts       = 1u << g.log2NSUB;
        st.slice_segments = (g.mode == MODE_SLICE_BLOCK || g.mode == MODE_SLICE_BASIC) ? g.nseg : 1;
        st.unstaged_items = r.fmt ? (uint32_t) h[5] : 0u;
        st.join_keys      = !r.kbits ? HWBRJ_JOIN_KEYS_32
                            : st.unstaged_items ? HWBRJ_JOIN_KEYS_MIXED : HWBRJ_JOIN_KEYS_PACKED;
        st.join_key_bits  = r.kbits ? r.kbits : 32u;
        // (probe / join ticks: the synchronous joins' phase split, added by wait())
        st.ms_join_probe  = (double) h[3];
        st.ms_join        = (double) h[4];
        if (r.timed) {  // the S scatter as the async schedule ran it (hwbrj_set_async_timing)
            float f = 0;
            HWBRJ_CHECK(hipEventElapsedTime(&f, tev_[r.slot][0], tev_[r.slot][1]));
            st.ms_s_scatter = f;
        }
        jdone_.push_back(st);
    }
    jr_.clear();
    return 0;
}

// Waits for the last join and collects every join since the last wait; the last one's phase times
// (synchronous joins) are read from its events.
// prepared: the join probed a prepared build (S pass first, no R side): its R boundaries ev[1..3]
// were not recorded, and stand at the end of the S lists, so the R phases are 0.
static int wait_common(hwbrj_stats_t* last, bool phases, const hipEvent_t* ev, bool sfirst, bool surv_fused,
                       bool prepared) {
    float ms[9] = {0, 0, 0, 0, (float) last->ms_s_scatter, 0, 0, 0, 0};  // (async: the timed S scatter only)
    if (phases) {  // (async joins: counts only)
        hipEvent_t e[9];
        for (int i = 0; i <= 8; i++) e[i] = ev[i];
        if (surv_fused) e[7] = ev[6];
        if (prepared) e[1] = e[2] = e[3] = ev[5];
        // phase i ends at boundary i and starts at boundary from[i] (S pass first: it starts the
        // join, the R scatter starts after the S lists, the probe after the build)
        static const int kFrom[2][9] = {{0, 0, 1, 2, 3, 4, 5, 6, 7}, {0, 5, 1, 2, 0, 4, 3, 6, 7}};
        const int* from = kFrom[sfirst ? 1 : 0];
        for (int i = 1; i <= 8; i++) HWBRJ_CHECK(hipEventElapsedTime(&ms[i], e[from[i]], e[i]));
        HWBRJ_CHECK(hipEventElapsedTime(&ms[0], e[0], e[8]));
    }
    const double pt = last->ms_join_probe, jt = last->ms_join;  // (ticks, ring_collect)
    last->ms_total      = ms[0];
    last->ms_r_scatter  = ms[1];
    last->ms_r_index    = ms[2];
    last->ms_build      = ms[3];
    last->ms_s_scatter  = ms[4];
    last->ms_s_index    = ms[5];
    last->ms_probe      = ms[6];
    last->ms_surv       = ms[7];
    last->ms_join       = ms[8];
    // the probe share of the join's workgroup time (k_join's wall_clock64 sections)
    last->ms_join_probe = jt > 0 ? ms[8] * pt / jt : 0.0;
    return 0;
}

// What wait and wait_all start with: the last join has completed and every join since the last wait
// is collected (jdone_), or why not.
int Engine::wait_pending() {
    if (!pending_) {
        ring_drop();
        set_last_error("no join has been enqueued");
        return 6;
    }
    HWBRJ_CHECK(hipEventSynchronize(ev_[8]));
    if (pending_rc_) {  // the last join stopped after some of its kernels (a failed broadcast)
        ring_drop();
        set_last_error(pending_err_);
        return pending_rc_;
    }
    return ring_collect();
}

int Engine::wait_all(hwbrj_stats_t* st, int cap, int* n) {
    HWBRJ_CHECK(hipSetDevice(device_));
    if (n) *n = 0;
    if (const int rc = wait_pending()) return rc;
    for (size_t i = 0; i < jdone_.size(); i++) {  // ticks -> ms (only the last has phase times)
        if (i + 1 == jdone_.size()) {
            if (const int rc = wait_common(&jdone_[i], pending_ev_, ev_, pending_sfirst_, surv_fused_, pending_prepared_)) return rc;
        } else {
            jdone_[i].ms_join_probe = jdone_[i].ms_join = 0;  // (the ticks: not phase times)
        }
    }
    const size_t tot = jdone_.size();
    if (tot) last_st_ = jdone_.back();
    if (n) *n = (int) tot;
    if (st)
        for (size_t i = 0; i < tot && (int) i < cap; i++) st[i] = jdone_[i];
    jdone_.clear();
    if (st && (size_t) cap < tot) {
        set_last_error("more joins than the stats array holds (the oldest were written)");
        return 7;
    }
    return 0;
}

int Engine::wait(hwbrj_stats_t* st) {
    HWBRJ_CHECK(hipSetDevice(device_));
    if (const int rc = wait_pending()) return rc;
    if (!jdone_.empty()) {  // (else: the last join was collected before; its stats again)
        last_st_ = jdone_.back();
        jdone_.clear();
        if (const int rc = wait_common(&last_st_, pending_ev_, ev_, pending_sfirst_, surv_fused_, pending_prepared_)) return rc;
    }
    if (st) *st = last_st_;
    return 0;
}

int Engine::export_filter(uint8_t* host_out, uint64_t nbytes) {
    HWBRJ_CHECK(hipSetDevice(device_));
    if (!have_filter_) {
        set_last_error("no filter has been built");
        return 5;
    }
    const Geometry& g = last_g_;
    if (nbytes != g.m / 8) {
        set_last_error("nbytes must equal m/8");
        return 6;
    }
    if (g.mode == MODE_GLOBAL) {
        HWBRJ_CHECK(hipMemcpy(host_out, bitmap.p, nbytes, hipMemcpyDeviceToHost));
        return 0;
    }
    return export_slices(slices, g, host_out, nbytes);
}

// the filter of slices sl (geometry g) in the reference layout, m / 8 bytes
int Engine::export_slices(const DevBuf& sl, const Geometry& g, uint8_t* host_out, uint64_t nbytes) {
    const uint64_t nwords = (g.m + 31) / 32;
    DevBuf tmp;
    if (!tmp.ensure(nwords * 4)) {
        set_last_error("hipMalloc failed");
        return 4;
    }
    launch_export(sl.as<uint32_t>(), g, tmp.as<uint32_t>(), nwords, own_stream_);
    HWBRJ_CHECK(hipStreamSynchronize(own_stream_));
    HWBRJ_CHECK(hipMemcpy(host_out, tmp.p, nbytes, hipMemcpyDeviceToHost));
    tmp.release();
    return 0;
}

// ------------------------------------------------------------------- prepared builds
// The R side of the one-shot join of (dR, vR, nR, args) into b's own buffers: the same plan, the same
// kernels (r_side), no ring slot and no zeroing, since it is part of no join. What the stages after
// the R side do not read (R's pool, metas, queues and lists but the sweeps' starts, and the R payload
// pool) is freed once k_build has run. The caller (hwbrj_api.cpp) has refused what a build does not
// offer; the geometry's refusals are repeated here for a caller that has not.
int Engine::build(const void* dR, const uint8_t* vR, uint64_t nR, const bloom_filter_args_t* args, hipStream_t stream,
                  Build* b, double* ms) {
    HWBRJ_CHECK(hipSetDevice(device_));
    if (!stream) stream = own_stream_;
    JoinReq q;
    q.kind    = b->rows ? JOIN_PAIRS : JOIN_COUNT;
    q.layout  = SRC_KEYS;
    q.masks.r = vR;
    JoinCtx c{JoinIn{dR, nR, nullptr, 0, args, stream}, q};
    c.vR = nR ? vR : nullptr;
    std::string err;
    if (!plan_geometry(args, nR, &c.g, &err, b->rows)) {
        set_last_error(err);
        return 2;
    }
    if (!masks_supported(c.g)) {
        set_last_error("a prepared build needs partition slices (blocked/sectorized, basic k = 1, or no filter)");
        return kRcMaskFilter;
    }
    plan(&c);
    c.bcast = false;  // (hwbrj_set_filter_broadcast does not apply: a build's slices are built here)
    if (const char* why = shape_limits(c.s, q)) {
        set_last_error(why);
        return 3;
    }
    RSide&           r = b->r;
    const JoinShape& s = c.s;
    bool ok = r.R.ensure(s.LR, s.G, s.F) && r.rjoin.ensure(s.sweeps_max * s.SLOT * 4) &&
              r.rrun.ensure(2 * s.sweeps_max * s.NSUB * 4);
    if (s.slice_mode) ok = ok && r.slices.ensure((uint64_t) s.F * s.nseg * c.g.seg_words * 4);
    if (b->rows)
        ok = ok && r.ppoolR.ensure(s.LR * 128) && r.rpay.ensure(s.sweeps_max * s.SLOT * 4) &&
             b->marks.ensure(((nR + 31) / 32) * 4) && b->cnt.ensure(16);
    if (b->rows && c.vR) ok = ok && r.rvalid.ensure((((nR + 7) / 8) + 3) & ~3ull);
    if (!ok) {
        set_last_error("hipMalloc failed (device memory)");
        return 4;
    }
    // the packing of the join keys, decided once as passes() decides it for a one-shot join
    c.kbits = !b->rows && join_pack3(c.g) && pack3_hint_ ? join_key_bits(c.g) : 0u;
    hipEvent_t e[2] = {nullptr, nullptr};
    HWBRJ_CHECK(hipEventCreate(&e[0]));
    HWBRJ_CHECK(hipEventCreate(&e[1]));
    auto run = [&]() -> int {
        HWBRJ_CHECK(hipEventRecord(e[0], stream));
        phase_ev_    = false;  // (the phase events belong to the joins)
        const int rc = r_side(c, &r, nullptr, nullptr);
        phase_ev_    = true;
        if (rc) return rc;
        if (b->rows) HWBRJ_CHECK(hipMemsetAsync(b->marks.p, 0, b->marks.bytes, stream));
        if (r.rvalid.p)  // (the dword tail past ceil(nR / 8) bytes is never read: k_null_rows)
            HWBRJ_CHECK(hipMemcpyAsync(r.rvalid.p, vR, (nR + 7) / 8, hipMemcpyDeviceToDevice, stream));
        HWBRJ_CHECK(hipEventRecord(e[1], stream));
        HWBRJ_CHECK(hipGetLastError());
        HWBRJ_CHECK(hipStreamSynchronize(stream));
        if (ms) {
            float f = 0;
            HWBRJ_CHECK(hipEventElapsedTime(&f, e[0], e[1]));
            *ms = f;
        }
        return 0;
    };
    const int rc = run();
    (void) hipEventDestroy(e[0]);
    (void) hipEventDestroy(e[1]);
    if (rc) return rc;
    for (DevBuf* d : {&r.R.pool, &r.R.meta, &r.R.used, &r.R.wgqc, &r.R.wgqe, &r.R.wgqo, &r.R.lstart, &r.R.estart,
                      &r.R.list, &r.R.col, &r.ppoolR})
        d->release();
    r.g        = c.g;
    r.s        = s;
    r.kbits    = c.kbits;
    r.nR       = nR;
    r.r_masked = c.vR != nullptr;
    b->device  = device_;
    b->has_args = args != nullptr;
    if (args) b->args = *args;
    return 0;
}

// The R rows no marking probe has matched: k_null_rows' pass over the marks, which have the layout of
// a validity bitmap (a clear bit is a row to emit, the tail past nR is masked off).
int Engine::unmatched(Build* b, uint2* out, uint64_t cap, uint64_t* n, hipStream_t stream, double* ms) {
    HWBRJ_CHECK(hipSetDevice(device_));
    if (!stream) stream = own_stream_;
    hipEvent_t e[2] = {nullptr, nullptr};
    HWBRJ_CHECK(hipEventCreate(&e[0]));
    HWBRJ_CHECK(hipEventCreate(&e[1]));
    auto run = [&]() -> int {
        HWBRJ_CHECK(hipMemsetAsync(b->cnt.p, 0, 8, stream));
        HWBRJ_CHECK(hipEventRecord(e[0], stream));
        launch_null_rows(NullRowsParams{b->marks.as<uint8_t>(), nullptr, b->r.nR, NULL_ROWS_R, 0xFFFFFFFFu, out, cap,
                                        b->cnt.as<unsigned long long>(), nullptr},
                         (uint32_t) cus_ * 2, stream);
        HWBRJ_CHECK(hipEventRecord(e[1], stream));
        HWBRJ_CHECK(hipGetLastError());
        HWBRJ_CHECK(hipMemcpyAsync(n, b->cnt.p, 8, hipMemcpyDeviceToHost, stream));
        HWBRJ_CHECK(hipStreamSynchronize(stream));
        if (ms) {
            float f = 0;
            HWBRJ_CHECK(hipEventElapsedTime(&f, e[0], e[1]));
            *ms = f;
        }
        return 0;
    };
    const int rc = run();
    (void) hipEventDestroy(e[0]);
    (void) hipEventDestroy(e[1]);
    return rc;
}

void Build::release() {
    r.release();
    for (DevBuf* d : {&marks, &cnt, &gacc[0], &gacc[1]}) d->release();
}

// The group accumulators (include/hwbrj.h, "group accumulators"): nR entries of 16 bytes, made at
// the form's first use, so a build that never accumulates holds what it held without them.
int Engine::group_acc_reset(Build* b, uint32_t agg) {
    HWBRJ_CHECK(hipSetDevice(device_));
    if (!b->gacc[agg].ensure(b->r.nR * 16)) {
        set_last_error("hipMalloc failed (device memory)");
        return 4;
    }
    launch_group_acc_init(b->gacc[agg].as<uint4>(), b->r.nR, agg, own_stream_);
    HWBRJ_CHECK(hipGetLastError());
    HWBRJ_CHECK(hipStreamSynchronize(own_stream_));
    b->gacc_ns[agg] = 0;
    return 0;
}

// One pass over the entries, with Engine::unmatched's counters: b->cnt holds {rows, pairs}. A form
// that has no accumulators yet has matched nothing: under `all` its rows are the identity rows, which
// k_group_acc_init writes straight to out[0, min(nR, cap)).
int Engine::group_rows(Build* b, uint32_t agg, bool all, uint4* out, uint64_t cap, uint64_t* n, uint64_t* pairs,
                       hipStream_t stream, double* ms) {
    HWBRJ_CHECK(hipSetDevice(device_));
    if (!stream) stream = own_stream_;
    const uint4* acc = b->gacc[agg].as<uint4>();
    hipEvent_t   e[2] = {nullptr, nullptr};
    HWBRJ_CHECK(hipEventCreate(&e[0]));
    HWBRJ_CHECK(hipEventCreate(&e[1]));
    uint64_t res[2] = {0, 0};
    auto run = [&]() -> int {
        HWBRJ_CHECK(hipMemsetAsync(b->cnt.p, 0, 16, stream));
        HWBRJ_CHECK(hipEventRecord(e[0], stream));
        if (acc) launch_group_acc_rows(acc, b->r.nR, all ? 1u : 0u, out, cap, b->cnt.as<unsigned long long>(), stream);
        else if (all) launch_group_acc_init(out, std::min<uint64_t>(b->r.nR, cap), agg, stream);
        HWBRJ_CHECK(hipEventRecord(e[1], stream));
        HWBRJ_CHECK(hipGetLastError());
        HWBRJ_CHECK(hipMemcpyAsync(res, b->cnt.p, 16, hipMemcpyDeviceToHost, stream));
        HWBRJ_CHECK(hipStreamSynchronize(stream));
        if (ms) {
            float f = 0;
            HWBRJ_CHECK(hipEventElapsedTime(&f, e[0], e[1]));
            *ms = f;
        }
        return 0;
    };
    const int rc = run();
    (void) hipEventDestroy(e[0]);
    (void) hipEventDestroy(e[1]);
    if (rc) return rc;
    *n     = acc ? res[0] : all ? b->r.nR : 0;
    *pairs = res[1];
    return 0;
}

int Engine::export_build_filter(const Build& b, uint8_t* host_out, uint64_t nbytes) {
    HWBRJ_CHECK(hipSetDevice(device_));
    if (!b.has_args) {
        set_last_error("no filter has been built");
        return 5;
    }
    if (nbytes != b.r.g.m / 8) {
        set_last_error("nbytes must equal m/8");
        return 6;
    }
    return export_slices(b.r.slices, b.r.g, host_out, nbytes);
}

// The build's filter as a selection bitmap (include/hwbrj.h hwbrj_build_filter_keys_device): one
// launch of k_filter_keys between two events, with a counter of the Engine's own (fkcnt_), so nothing
// a join owns is read or written and a pending join stays pending.
int Engine::filter_keys(const Build& b, const int32_t* dS, const uint8_t* vS, uint64_t nS, uint8_t* out,
                        uint64_t* n_pass, hipStream_t stream, double* ms) {
    HWBRJ_CHECK(hipSetDevice(device_));
    if (!stream) stream = own_stream_;
    if (!fkcnt_.ensure(8)) {
        set_last_error("hipMalloc failed (device memory)");
        return 4;
    }
    hipEvent_t e[2] = {nullptr, nullptr};
    uint64_t   n    = 0;
    auto run = [&]() -> int {  // (the events are created inside: a failure of the second still frees the first)
        HWBRJ_CHECK(hipEventCreate(&e[0]));
        HWBRJ_CHECK(hipEventCreate(&e[1]));
        HWBRJ_CHECK(hipMemsetAsync(fkcnt_.p, 0, 8, stream));
        HWBRJ_CHECK(hipEventRecord(e[0], stream));
        if (!launch_filter_keys(FilterKeysParams{(const uint32_t*) dS, vS, nS, b.r.g, b.r.slices.as<uint32_t>(), d_tabs_,
                                                 (uint32_t*) out, fkcnt_.as<unsigned long long>()},
                                (uint32_t) cus_ * 8, stream)) {
            set_last_error("the build's filter is not kept in partition slices");
            return kRcMaskFilter;
        }
        HWBRJ_CHECK(hipEventRecord(e[1], stream));
        HWBRJ_CHECK(hipGetLastError());
        HWBRJ_CHECK(hipMemcpyAsync(&n, fkcnt_.p, 8, hipMemcpyDeviceToHost, stream));
        HWBRJ_CHECK(hipStreamSynchronize(stream));
        if (ms) {
            float f = 0;
            HWBRJ_CHECK(hipEventElapsedTime(&f, e[0], e[1]));
            *ms = f;
        }
        return 0;
    };
    const int rc = run();
    for (hipEvent_t ev : e)
        if (ev) (void) hipEventDestroy(ev);
    if (rc) return rc;
    if (n_pass) *n_pass = n;
    return 0;
}

// ---- test-only table readback (include/hwbrj.h hwbrj_tables_info / hwbrj_tables_read) ----
int Engine::tables_ready() {
    HWBRJ_CHECK(hipSetDevice(device_));
    if (!jr_.empty() || !pj_q_.empty()) {  // (enqueued and not collected: its kernels may be running)
        set_last_error("a join is pending (wait for it first)");
        return 12;
    }
    if (tab_.state == kTabOther) {
        set_last_error("the last join's pipeline keeps other tables (basic k >= 2, partitioned joins)");
        return 13;
    }
    if (tab_.state != kTabJoin || !tab_.sync) {
        set_last_error("no synchronous join has completed");
        return 6;
    }
    return 0;
}

int Engine::tables_info(uint64_t* out, int n) {
    if (const int rc = tables_ready()) return rc;
    if (!out || n < HWBRJ_TI_COUNT) {
        set_last_error("out must hold HWBRJ_TI_COUNT words");
        return 7;
    }
    const TabRec&  t = tab_;
    const uint32_t F = 1u << t.g.log2F;
    uint32_t       sweeps = 0, items = 0;
    HWBRJ_CHECK(hipMemcpy(&sweeps, R_.istart.as<uint32_t>() + F, 4, hipMemcpyDeviceToHost));
    HWBRJ_CHECK(hipMemcpy(&items, S_.istart.as<uint32_t>() + F, 4, hipMemcpyDeviceToHost));
    const PathConstants c = path_constants();
    for (int i = 0; i < n; i++) out[i] = 0;
    out[HWBRJ_TI_MODE]        = (uint64_t) t.g.mode;
    out[HWBRJ_TI_FORMAT]      = (uint64_t) t.g.s_format;
    out[HWBRJ_TI_F]           = F;
    out[HWBRJ_TI_NSUB]        = 1u << t.g.log2NSUB;
    out[HWBRJ_TI_SUB_SHIFT]   = t.g.sub_shift;
    out[HWBRJ_TI_HASH_SHIFT]  = t.g.hash_shift;
    out[HWBRJ_TI_NSEG]        = t.s.nseg;
    out[HWBRJ_TI_BITMAP]      = t.bitmap;
    out[HWBRJ_TI_JKIND]       = t.jkind;
    out[HWBRJ_TI_KEY_BITS]    = t.kbits ? t.kbits : 32u;
    out[HWBRJ_TI_GRID]        = t.s.G;
    out[HWBRJ_TI_CH]          = t.s.CH;
    out[HWBRJ_TI_BSW]         = t.s.BSW;
    out[HWBRJ_TI_SLOT]        = t.s.SLOT;
    out[HWBRJ_TI_STAGE_CAP]   = t.stage_cap;
    out[HWBRJ_TI_SWEEPS]      = sweeps;
    out[HWBRJ_TI_ITEMS]       = items;
    out[HWBRJ_TI_JOBS]        = t.s.NJ;
    out[HWBRJ_TI_MAT]         = t.mat ? 1u : 0u;
    out[HWBRJ_TI_SPLIT]       = t.split ? t.split : c.join_task_surv;
    out[HWBRJ_TI_SC_ROUND]    = c.sc_round;
    out[HWBRJ_TI_SC_FLUSHES]  = c.sc_flushes;
    out[HWBRJ_TI_J_FUSED]     = c.join_fused_sweeps;
    out[HWBRJ_TI_J_FW]        = c.join_fw;
    out[HWBRJ_TI_J_FS]        = c.join_fs;
    out[HWBRJ_TI_J_WAVES]     = c.join_waves;
    out[HWBRJ_TI_J_DESC]      = c.join_desc;
    out[HWBRJ_TI_J_PIECE]     = c.join_piece;
    out[HWBRJ_TI_J_TASK_SURV] = c.join_task_surv;
    out[HWBRJ_TI_J_EXTRA]     = c.join_extra;
    out[HWBRJ_TI_J_TAIL_U]    = c.join_tail_u;
    out[HWBRJ_TI_J_TAIL_S]    = c.join_tail_s;
    out[HWBRJ_TI_J_RW]        = c.join_rw;
    out[HWBRJ_TI_J_SW]        = c.join_sw;
    out[HWBRJ_TI_M_PIECE]     = c.mat_piece;
    out[HWBRJ_TI_M_DESC]      = c.mat_desc;
    out[HWBRJ_TI_M_RCAP]      = c.mat_rcap;
    return 0;
}

int Engine::tables_read(int which, void* host_out, uint64_t cap_bytes, uint64_t* bytes) {
    if (const int rc = tables_ready()) return rc;
    const TabRec&  t = tab_;
    const uint32_t F = 1u << t.g.log2F, NSUB = 1u << t.g.log2NSUB;
    if (bytes) *bytes = 0;
    const void* src  = nullptr;
    uint64_t    need = 0;
    auto last = [&](const DevBuf& b, uint32_t* v) -> int {  // entry [F] of a u32 start table
        HWBRJ_CHECK(hipMemcpy(v, b.as<uint32_t>() + F, 4, hipMemcpyDeviceToHost));
        return 0;
    };
    uint32_t sweeps = 0, items = 0;
    if (const int rc = last(R_.istart, &sweeps)) return rc;
    if (const int rc = last(S_.istart, &items)) return rc;
    if (which >= HWBRJ_TAB_SURV_ITEM) {
        // one item's survivor region (k_probe's item regions, JoinParams::surv): the words of its
        // input chunks, at seg * seg_stride + (list_start[q] + piece * CH) * 32
        const uint32_t it = (uint32_t) (which - HWBRJ_TAB_SURV_ITEM);
        if (it >= items) {
            set_last_error("no such probe item");
            return 2;
        }
        std::vector<uint32_t> is(F + 1), ls(F + 1);
        HWBRJ_CHECK(hipMemcpy(is.data(), S_.istart.p, (F + 1) * 4, hipMemcpyDeviceToHost));
        HWBRJ_CHECK(hipMemcpy(ls.data(), S_.lstart.p, (F + 1) * 4, hipMemcpyDeviceToHost));
        const uint32_t q = (uint32_t) (std::upper_bound(is.begin(), is.end(), it) - is.begin()) - 1;
        const uint32_t npc = (is[q + 1] - is[q]) / t.s.nseg, local = it - is[q];
        const uint32_t seg = local / npc, piece = local - seg * npc;
        const uint32_t nch = std::min(t.s.CH, ls[q + 1] - ls[q] - piece * t.s.CH);
        src  = surv.as<uint32_t>() + (uint64_t) seg * t.s.seg_stride() + (uint64_t) (ls[q] + piece * t.s.CH) * 32;
        need = (uint64_t) nch * 128;
    } else {
        switch (which) {
            case HWBRJ_TAB_R_ELEM_START: src = R_.estart.p, need = (uint64_t) (F + 1) * 8; break;
            case HWBRJ_TAB_S_ELEM_START: src = S_.estart.p, need = (uint64_t) (F + 1) * 8; break;
            case HWBRJ_TAB_R_SWEEP_START: src = R_.istart.p, need = (uint64_t) (F + 1) * 4; break;
            case HWBRJ_TAB_R_RUN_CNT: src = rrun.p, need = (uint64_t) sweeps * NSUB * 4; break;
            case HWBRJ_TAB_R_RUN_OFF:
                src = rrun.as<uint32_t>() + t.s.sweeps_max * NSUB, need = (uint64_t) sweeps * NSUB * 4;
                break;
            case HWBRJ_TAB_R_KEYS: src = rjoin.p, need = (uint64_t) sweeps * t.s.SLOT * 4; break;
            case HWBRJ_TAB_S_LIST_START: src = S_.lstart.p, need = (uint64_t) (F + 1) * 4; break;
            case HWBRJ_TAB_S_ITEM_START: src = S_.istart.p, need = (uint64_t) (F + 1) * 4; break;
            case HWBRJ_TAB_SURV_CNT: src = survcnt.p, need = (uint64_t) items * NSUB * 4; break;
            case HWBRJ_TAB_SURV_OFF: src = survoff.p, need = (uint64_t) items * NSUB * 4; break;
            case HWBRJ_TAB_NPARTS:
                if (t.mat) {  // (k_join_split does not run before k_join_mat: one part per job)
                    set_last_error("the materializing join has no parts table");
                    return 13;
                }
                // nparts [NJ], then the extra-part count (jparts: nparts | job_surv | nextra)
                need = (uint64_t) (t.s.NJ + 1) * 4;
                if (bytes) *bytes = need;
                if (cap_bytes < need || !host_out) {
                    set_last_error("cap_bytes too small (*bytes holds the need)");
                    return 7;
                }
                HWBRJ_CHECK(hipMemcpy(host_out, jparts.p, (size_t) t.s.NJ * 4, hipMemcpyDeviceToHost));
                HWBRJ_CHECK(hipMemcpy((uint32_t*) host_out + t.s.NJ, jparts.as<uint32_t>() + 2 * t.s.NJ, 4,
                                      hipMemcpyDeviceToHost));
                return 0;
            default: set_last_error("unknown table"); return 2;
        }
    }
    if (bytes) *bytes = need;
    if (cap_bytes < need || (need && !host_out)) {
        set_last_error("cap_bytes too small (*bytes holds the need)");
        return 7;
    }
    if (need) HWBRJ_CHECK(hipMemcpy(host_out, src, need, hipMemcpyDeviceToHost));
    return 0;
}

// The side pass of the global-bitmap mode, once for every payload join: the table of R
// (side_slots(nR) slots) and the counters c[0, nc) in mcount, the kind's own buffers (`own`, each
// filled with its 32-bit value), the table build, then the kind's probes: launch(t, stream), t =
// the table and the counting join's filter (the side pass follows it). *ms = the device time from
// the build to the last probe.
static uint64_t side_slots(uint64_t nR) {
    uint64_t T = 2;
    while (T < 2 * nR) T <<= 1;
    return T;
}

template <class Launch>
int Engine::side_pass(const void* dR, uint64_t nR, int layout, hipStream_t stream, const char* what,
                      const std::vector<SideBuf>& own, uint64_t* c, uint32_t nc, double* ms, Launch&& launch) {
    HWBRJ_CHECK(hipSetDevice(device_));
    if (!stream) stream = own_stream_;
    const uint64_t T  = side_slots(nR);
    bool           ok = mtab.ensure(T * 8) && mcount.ensure(nc * 8);
    for (const SideBuf& b : own) ok = ok && b.buf->ensure(b.bytes);
    if (!ok) {
        set_last_error(std::string("hipMalloc failed (") + what + ")");
        return 4;
    }
    HWBRJ_CHECK(hipMemsetAsync(mtab.p, 0, T * 8, stream));
    HWBRJ_CHECK(hipMemsetAsync(mcount.p, 0, nc * 8, stream));
    for (const SideBuf& b : own)
        HWBRJ_CHECK(hipMemsetD32Async((hipDeviceptr_t) b.buf->p, (int) b.fill, b.bytes / 4, stream));
    HWBRJ_CHECK(hipEventRecord(ev_[0], stream));
    if (nR) launch_mat_build(dR, layout, nR, mtab.as<unsigned long long>(), T - 1, stream);
    SideTable t{mtab.as<unsigned long long>(), T - 1, last_g_, slices.as<uint32_t>(), bitmap.as<uint32_t>(), d_tabs_};
    if (!have_filter_) t.g.mode = MODE_NOBLOOM;
    launch(t, stream);
    HWBRJ_CHECK(hipEventRecord(ev_[8], stream));
    HWBRJ_CHECK(hipGetLastError());
    HWBRJ_CHECK(hipEventSynchronize(ev_[8]));
    HWBRJ_CHECK(hipMemcpy(c, mcount.p, nc * 8, hipMemcpyDeviceToHost));
    if (ms) {
        float f = 0;
        HWBRJ_CHECK(hipEventElapsedTime(&f, ev_[0], ev_[8]));
        *ms = f;
    }
    return 0;
}

int Engine::side(const JoinIn& in, const JoinReq& req, uint64_t* n, JoinExtras* x, double* ms) {
    JoinExtras own;
    if (!x) x = &own;
    switch (req.kind) {
        case JOIN_PAIRS: return pairs_side(in, req, n, ms);
        case JOIN_SEMI: return semi_side(in, req, n, ms);
        case JOIN_OUTER: return outer_side(in, req, n, x->cls, ms);
        case JOIN_GROUP: return group_side(in, req, n, &x->pairs, ms);
        default: set_last_error("a counting join has no side pass"); return 2;
    }
}

// (R.payload, S.payload) of every match into out[0, cap)
int Engine::pairs_side(const JoinIn& in, const JoinReq& q, uint64_t* n, double* ms) {
    return side_pass(in.dR, in.nR, q.layout, in.stream, "materialization table", {}, n, 1, ms,
                     [&](const SideTable& t, hipStream_t s) {
                         if (in.nR && in.nS)
                             launch_pair_probe(in.dS, q.layout, in.nS, in.dR, t, 0u, 0u, nullptr, (uint2*) q.out, q.cap,
                                               mcount.as<unsigned long long>(), s);
                     });
}

int Engine::semi_side(const JoinIn& in, const JoinReq& q, uint64_t* n, double* ms) {
    return side_pass(in.dR, in.nR, q.layout, in.stream, "existence table", {}, n, 1, ms,
                     [&](const SideTable& t, hipStream_t s) {
                         if (in.nS)
                             launch_semi_probe(in.dS, q.layout, in.nS, t, q.anti ? 1u : 0u, (uint2*) q.out, q.cap,
                                               mcount.as<unsigned long long>(), s);
                     });
}

int Engine::outer_side(const JoinIn& in, const JoinReq& q, uint64_t* n, uint64_t cls[3], double* ms) {
    tab_.state = kTabOther;  // (an outer join's tables are not read back, in this mode either)
    const size_t fbytes = (size_t) std::max<uint64_t>(side_slots(in.nR) / 8, 4);  // one bit per table slot
    std::vector<SideBuf> own;
    if (q.keep_r) own.push_back({&smark, fbytes, 0u});
    uint64_t  c[3];
    const int rc = side_pass(
        in.dR, in.nR, q.layout, in.stream, "outer join table", own, c, 3, ms, [&](const SideTable& t, hipStream_t s) {
            uint32_t*           rflag = q.keep_r ? smark.as<uint32_t>() : nullptr;
            unsigned long long* cnt   = mcount.as<unsigned long long>();
            if (in.nS)
                launch_pair_probe(in.dS, q.layout, in.nS, in.dR, t, q.keep_s ? 1u : 0u, q.null_pay, rflag,
                                  (uint2*) q.out, q.cap, cnt, s);
            if (q.keep_r && in.nR)
                launch_outer_rtab(in.dR, q.layout, t.tab, t.mask + 1, rflag, q.null_pay, (uint2*) q.out, q.cap, cnt, s);
        });
    if (rc) return rc;
    *n     = c[0];
    cls[0] = c[0] - c[1] - c[2];
    cls[1] = c[1];
    cls[2] = c[2];
    return 0;
}

int Engine::group_side(const JoinIn& in, const JoinReq& q, uint64_t* n, uint64_t* pairs, double* ms) {
    if (q.layout == SRC_KEYS && in.nS && !q.s_val) {
        set_last_error("key columns: a group join needs S's value column");
        return 2;
    }
    tab_.state = kTabOther;  // (a group join's tables are not read back, in this mode either)
    const size_t rows = (size_t) std::max<uint64_t>(in.nR, 1);  // one count and one sum (or min and max) per R row
    const bool   minmax = q.agg == GRP_COUNT_MINMAX;
    std::vector<SideBuf> own{{&gcnt, rows * 4, 0u}};
    if (minmax) own.insert(own.end(), {{&gmin, rows * 4, (uint32_t) INT32_MAX}, {&gmax, rows * 4, (uint32_t) INT32_MIN}});
    else own.push_back({&gsum, rows * 8, 0u});
    uint64_t  c[2];
    const int rc = side_pass(in.dR, in.nR, q.layout, in.stream, "group join table", own, c, 2, ms,
                                [&](const SideTable& t, hipStream_t s) {
        const GroupAcc a{gcnt.as<uint32_t>(), gsum.as<unsigned long long>(), gmin.as<int32_t>(), gmax.as<int32_t>()};
        if (in.nR && in.nS) launch_group_probe(in.dS, q.s_val, q.layout, in.nS, t, a, q.agg, s);
        if (in.nR)
            launch_group_rows(in.dR, q.layout, in.nR, a, q.agg, q.all ? 1u : 0u, (uint4*) q.out, q.cap,
                              mcount.as<unsigned long long>(), s);
    });
    if (rc) return rc;
    *n     = c[0];
    *pairs = c[1];
    return 0;
}

int Engine::generate(uint2* d_out, uint64_t n, uint64_t offset, uint64_t count, uint32_t nthreads,
                     uint64_t maxid, uint64_t threshold, double selectivity, uint64_t seed,
                     hipStream_t stream) {
    HWBRJ_CHECK(hipSetDevice(device_));
    std::vector<GenPlan> plan(1);
    if (make_gen_plan(&plan[0], n, nthreads, maxid, threshold, selectivity)) {
        set_last_error("invalid generator parameters");
        return 2;
    }
    if (!stream) stream = own_stream_;
    HWBRJ_CHECK(hipMemcpyAsync(d_plan_, plan.data(), sizeof(GenPlan), hipMemcpyHostToDevice, stream));
    if (offset > n || count > n - offset) {
        set_last_error("generator range outside the relation");
        return 2;
    }
    launch_gen(d_out, offset, count, d_plan_, make_perm(n, seed), stream);
    HWBRJ_CHECK(hipGetLastError());
    HWBRJ_CHECK(hipStreamSynchronize(stream));
    return 0;
}

// ----------------------------------------------------------------- per-device singletons
static std::mutex g_mu;
static Engine*    g_engines[64] = {};

Engine* engine_for_current_device() {
    int        dev = 0;
    hipError_t e   = hipGetDevice(&dev);
    if (e != hipSuccess) {  // a runtime not yet initialised in this library's HIP instance
        (void) hipInit(0);
        e = hipGetDevice(&dev);
    }
    if (e != hipSuccess || dev < 0 || dev >= 64) {
        set_last_error(std::string("no HIP device (hipGetDevice: ") + hipGetErrorString(e) + ")");
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_engines[dev]) g_engines[dev] = new Engine(dev);
    return g_engines[dev];
}

}  // namespace hwbrj
