// hwbrj_kernels.h -- kernel parameter blocks and launch wrappers (internal C++ interface between
// the HIP kernels and the host engine in hwbrj_engine.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <stddef.h>
#include <stdint.h>

#include "hwbrj_common.h"

namespace hwbrj {

// What a scatter reads: {key, payload} tuples, 4-byte codes, or a column of 4-byte keys (hashed as
// the tuples' keys are). SRC_KEYS is also the input layout of a whole counting join (Engine::run).
// SRC_KEYS_VAL: a key column with a value column of the same length beside it (ScatterParams::
// src_val), the payload scatter of S only: element i carries payload src_val[i] (the group joins on
// key columns).
// SRC_KEYS_MASK: a key column with a validity bitmap beside it (ScatterParams::valid): a row whose
// bit is clear is a NULL key, which the scatter places nowhere (the counting scatter and the
// row-index payload scatter, either side; launch_scatter only: the Engine's layouts are the first
// and the third).
// SRC_KEYS_VAL_MASK: SRC_KEYS_VAL with one or two validity bitmaps (ScatterValParams::vmask: the key
// column's, the value column's, or both): a row is placed iff its bit is set in each (the group joins
// on key columns with NULL keys and NULL values; launch_scatter only, as SRC_KEYS_MASK).
enum Source : int {
    SRC_TUPLES = 0, SRC_CODES = 1, SRC_KEYS = 2, SRC_KEYS_VAL = 3, SRC_KEYS_MASK = 4, SRC_KEYS_VAL_MASK = 5
};

struct ScatterParams {
    const void*      src;          // uint2 tuples {key, payload}, uint32 codes or uint32 keys
    uint64_t         n;            // element count (ignored when n_dev != nullptr)
    const uint64_t*  n_dev;        // optional device-resident element count
    uint32_t*        pool;         // [G * cap][32] chunk words
    uint32_t*        ppool;        // [G * cap][32] the words' payloads (materialization), or nullptr
    uint32_t*        meta;         // [G * cap] 16-bit entries (meta16): partition | (count - 1) << 10
    uint32_t*        wg_used;      // [G] chunks used by each workgroup
    uint32_t*        wgq_chunks;   // [G][F] chunks of partition q in workgroup wg's region
    uint32_t*        wgq_elems;    // [G][F] elements of partition q in workgroup wg's region
    uint64_t         cap;          // chunk capacity of one workgroup region
    union {                        // (one slot: no source uses both, and every field keeps the
                                   // kernel-argument offset it had before src_val)
        const uint32_t* seg_cnt;   // SRC_CODES from per-workgroup segments: workgroup w partitions
                                   // src + w * seg_stride (elements), seg_cnt[w] of them; or nullptr
        const void*     src_val;   // SRC_KEYS_VAL: the n uint32 values beside src's keys, 16-byte
                                   // aligned as src
        const uint8_t*  valid;     // SRC_KEYS_MASK: src's validity bitmap, ceil(n / 8) bytes: row i is
                                   // bit i & 7 of byte i >> 3, set = valid (bits past n: not read)
    };
    uint64_t         seg_stride;
    uint64_t         vn;           // MODE_BASIC_POS: tuples / keys of src (n = k * vn elements, k <= grid)
    // the join's per-call zeroing, done by workgroup 0 instead of memset dispatches: zero_small[0, 16)
    // (counts) and *zero_word (the join's extra-task count), each when not nullptr
    uint32_t*        zero_small;
    uint32_t*        zero_word;
    Geometry         g;
    const CrcTables* tabs;
};
// SRC_KEYS_VAL_MASK: the value-column scatter's bitmaps, which cannot use `valid` (src_val's slot).
// They stand behind the last field of ScatterParams in a type of their own, the argument of the
// k_scatter_spvm kernels alone: appended to ScatterParams itself they would grow every scatter
// kernel's argument block and move the hidden arguments (the grid size) behind it, that is, change
// the code of every existing scatter. launch_scatter(p, SRC_KEYS_VAL_MASK, ...) takes p as this type.
// vmask[0]: a bitmap of the n rows (ScatterParams::valid's layout), never nullptr; vmask[1]: a second
// one, or nullptr (one bitmap: the key column's or the value column's, the kernel cannot tell).
struct ScatterValParams : ScatterParams {
    const uint8_t* vmask[2];
};

// Packed join keys between the build / probe and the join (BuildParams::kbits): on when the join
// key v = code >> hash_shift fits 24 bits and the run formats are private to k_join (not the
// materializing join, which reads codes, nor the partitioned join, which ships survivor words).
// Keys are a bit stream of kbits-bit fields: 18 bits when hash_shift = 14 (the bitmap path's keys,
// every north-star job: 16 keys per 9 dwords), else 24 (4 keys per 12 bytes); 0 = 32-bit codes.
#ifndef HWBRJ_PACK3
#define HWBRJ_PACK3 1
#endif
#ifndef HWBRJ_PACK18
#define HWBRJ_PACK18 1  // 0: 24-bit keys for the hash_shift = 14 launches too (A/B)
#endif
inline bool join_pack3(const Geometry& g) { return HWBRJ_PACK3 != 0 && g.sub_shift > 0 && g.hash_shift >= 8; }
inline uint32_t join_key_bits(const Geometry& g) {
    return !join_pack3(g) ? 0u : (HWBRJ_PACK18 && g.hash_shift == 14) ? 18u : 24u;
}

// Joins enqueued without phase events (hwbrj_join_device_async: the timed back-to-back joins) run
// their S pass on a second stream beside the R side, joined before the probe (A/B: 0 = one stream,
// S pass first). Synchronous joins keep one stream, so their phase times stay separate.
#ifndef HWBRJ_OVL_ASYNC
#define HWBRJ_OVL_ASYNC 1
#endif
#ifndef HWBRJ_PJ_OVL
#define HWBRJ_PJ_OVL 1  // async partitioned joins: the S shard's partitioning on a second stream
#endif

struct BuildParams {
    Geometry         g;
    const CrcTables* tabs;
    const uint32_t*  pool;
    const uint32_t*  list;        // chunk lists (entry = chunk id | count << 27)
    const uint32_t*  list_start;  // [F + 1]
    const uint64_t*  elem_start;  // [F + 1]
    uint32_t*        slices;      // [F][nseg][seg_words]
    const uint32_t*  sweep_start; // [F + 1] first build sweep of each partition
    uint32_t*        out_codes;   // [sweeps][kBSlot]: each sweep's R codes sorted by sub
    uint32_t*        run_cnt;     // [sweeps][NSUB] codes of each (sweep, sub) run
    uint32_t*        run_off;     // [sweeps][NSUB] run offset inside the sweep's slot
    uint32_t         q_base;      // partition of workgroup 0 (list/sweep tables indexed from it)
    const uint32_t*  ppool;       // payloads of pool's words (materialization), or nullptr
    uint32_t*        out_pay;     // [sweeps][kBSlot]: the payloads of out_codes (ppool set)
    uint32_t         no_slices;   // 1: join runs only (the slices arrive by broadcast from rank 0)
    uint32_t         kbits;       // 18 / 24: out_codes hold the slot's keys (code >> hash_shift) as a
                                  // stream of kbits-bit fields from its byte 0 (join_key_bits; not
                                  // PAY); 0: 32-bit codes
};

struct ProbeParams {
    Geometry         g;
    const CrcTables* tabs;
    const uint32_t*  pool;
    const uint32_t*  list;        // chunk lists (entry = chunk id | count << 27)
    const uint32_t*  list_start;  // [F + 1]
    const uint32_t*  item_start;  // [F + 1]
    const uint32_t*  slices;
    uint32_t*        surv;        // item region at (seg * surv_seg_stride + list_pos * 32), by sub
    uint64_t         surv_seg_stride;
    uint32_t*        surv_cnt;    // [items][NSUB] survivors of each (item, sub) run
    uint32_t*        surv_off;    // [items][NSUB] run offset inside the item region
    uint64_t*        filtered;    // += survivors ("S-tuples after filter")
    uint32_t*        job_surv;    // [F * NSUB] += survivors of each join job (zero on entry)
    uint32_t         stage_cap;   // survivor stage words (set by launch_probe)
    uint32_t*        surv_pos;    // materialization: each survivor's chunk position (its payload's
                                  // index in the S payload pool), parallel to surv; or nullptr
    uint32_t*        wg_cnt;      // k_probe_bitj: words appended to workgroup w's region
                                  // (surv + w * surv_seg_stride)
    uint32_t         kbits;       // 18 / 24: staged items store their join keys (code >> hash_shift)
                                  // as a stream of kbits-bit fields from the item region's byte 0,
                                  // flagged by bit 31 of their surv_off entries (unstaged items keep
                                  // 32-bit codes); 0: 32-bit codes
    uint32_t*        fmt_cnt;     // kbits: += the unstaged items (zeroed by the R scatter), or nullptr
};

struct JoinParams {
    const uint32_t* r_codes;      // build sweep slots (BuildParams::out_codes)
    const uint32_t* r_sweep_start;  // [F + 1]
    const uint32_t* r_cnt;        // [sweeps][NSUB]
    const uint32_t* r_off;        // [sweeps][NSUB]
    const uint32_t* surv;         // survivor runs written by k_probe
    const uint32_t* surv_cnt;
    const uint32_t* surv_off;
    const uint32_t* item_start;   // S items [F + 1]
    const uint32_t* list_start;   // S lists [F + 1]
    uint64_t        surv_seg_stride;
    uint32_t        nseg, CH, log2NSUB, hash_shift;
    uint32_t        slot;         // r_codes words per build sweep
    uint32_t        bitmap;       // 1: keys fit the direct-address bitmap (32 - hash_shift <= 18)
    uint64_t*       jsum;         // kJoinSumSlots partial sums, one per 128-byte line (zeroed by
                                  // k_join_split, summed by the host)
    uint32_t        jobs;         // F * NSUB (set by launch_join)
    uint32_t*       nparts;       // [jobs] parts of each job (k_join_split)
    uint2*          extra;        // [join_extra_tasks()] {job, part} of the further parts
    uint32_t*       nextra;       // parts requested beyond part 0 (zeroed before the join)
    uint32_t        split_surv;   // survivors per join part (0: the default, kJoinTaskSurv)
    uint32_t        jkind;        // per-partition join: 0 bucket chaining's role (bitmap / hash
                                  // table, PRO), 1 histogram join (PRH), 2 + 16-byte compares (PRHO)
    const uint64_t* item_base;    // [items] survivor region of each item (partitioned multi-GPU
                                  // join: received runs), or nullptr (k_probe's item regions)
    uint32_t        r_kbits;      // 18 / 24: r_codes hold packed join keys (BuildParams::kbits), and so
                                  // do the survivor runs flagged by bit 31 of surv_off; 0: codes
    const uint32_t* fmt_cnt;      // ProbeParams::fmt_cnt (the launch's survivor-run formats), or nullptr
    uint32_t        timing;       // 1: accumulate the probe / total ticks (result[3], result[4]) for
                                  // ms_join_probe (synchronous joins; 0: one count add per workgroup)
};

// What every (q, sub) job of the payload joins reads (k_join_mat, k_join_semi, k_join_outer,
// k_join_group): the R codes of the build sweeps and their run descriptors, the survivors with their
// chunk positions and run descriptors, and the job geometry.
struct JobInputs {
    const uint32_t* r_codes;
    const uint32_t* r_sweep_start;  // [F + 1]
    const uint32_t* r_cnt;
    const uint32_t* r_off;
    uint32_t        slot;
    const uint32_t* surv;
    const uint32_t* surv_pos;       // ProbeParams::surv_pos
    const uint32_t* surv_cnt;
    const uint32_t* surv_off;
    const uint32_t* item_start;
    const uint32_t* list_start;
    uint64_t        surv_seg_stride;
    uint32_t        nseg, CH, log2NSUB, hash_shift;
    uint32_t        xcd8;           // 1: XCD-aware job order (F a multiple of 8; set by the launch_join_* wrappers)
};

// The materializing join (k_join_mat): R codes + payloads of the build sweeps, survivors + their
// chunk positions, {R.payload, S.payload} pairs appended to out (up to cap; count = all pairs).
struct MatJoinParams {
    JobInputs       j;
    const uint32_t* r_pay;          // BuildParams::out_pay
    uint32_t        bm;             // 1: job keys v = code >> hash_shift < 2^17 (the bitmap path)
    const uint32_t* s_pay;          // S payload pool (ScatterParams::ppool of the S pass)
    uint2*          out;
    uint64_t        cap;
    unsigned long long* count;      // += pairs (zero on entry)
};

// The existence join (k_join_semi): R codes of the build sweeps (no payloads), survivors + their
// chunk positions. SEMI: {key, S.payload} of every survivor whose key is in R appended to out (up
// to cap; count = all rows). ANTI: the matching survivors' chunk positions marked in `mark` (one
// bit per S chunk position), for k_semi_emit.
struct SemiJoinParams {
    JobInputs       j;
    uint32_t        bm;             // 1: job keys v = code >> hash_shift < 2^17 (the bitmap path)
    uint32_t        anti;           // 1: mark only (k_semi_emit writes the rows)
    uint32_t        basic;          // 1: the words are bmix(key) (MODE_SLICE_BASIC), else codes
    const uint32_t* s_pay;          // S payload pool
    uint32_t*       mark;           // [S chunks] bit i of word c: position 32 c + i matched (zero on
                                    // entry; anti or !bm), or nullptr
    const CrcTables* tabs;
    uint2*          out;
    uint64_t        cap;
    unsigned long long* count;      // += rows (zero on entry)
};
void   launch_join_semi(const SemiJoinParams& p, uint32_t jobs, hipStream_t st);
// ANTI's emission pass (k_semi_emit): {key, payload} of every S tuple of the chunk lists whose
// position is not marked, appended to out (up to cap; *count += rows)
struct SemiEmitParams {
    const uint32_t*  pool;        // S chunk words
    const uint32_t*  ppool;       // their payloads
    const uint32_t*  list;        // S chunk lists
    const uint32_t*  list_start;  // [F + 1]
    const uint32_t*  mark;
    Geometry         g;
    const CrcTables* tabs;
    uint2*           out;
    uint64_t         cap;
    unsigned long long* count;
};
void   launch_semi_emit(const SemiEmitParams& p, uint32_t grid, hipStream_t st);

// The outer join (k_join_outer): the materializing join's inputs and pairs (m), and
//  - keep_s: every survivor with a partner marks its chunk position in `mark` (one bit per S chunk
//    position, zero on entry); k_outer_emit then writes {null_pay, S.payload} of every unmarked one;
//  - keep_r: {R.payload, null_pay} of every R tuple of the job that no survivor matched, appended to
//    m.out through m.count like the pairs; *n_r_only += those rows.
struct OuterJoinParams {
    MatJoinParams       m;
    uint32_t            keep_s, keep_r;
    uint32_t            null_pay;
    uint32_t*           mark;      // [S chunks], or nullptr (!keep_s)
    unsigned long long* n_r_only;  // zero on entry
};
void   launch_join_outer(const OuterJoinParams& p, uint32_t jobs, hipStream_t st);
// The marking probe of a prepared build (k_join_outer_mark): the outer join's pairs and S marks (o;
// o.keep_r is not read), and every R tuple of a job with at least one partner ORs bit r_payload & 31
// of dword r_payload >> 5 into rmark, the build's one bit per R row. No R-only row is written. The
// pointer stands behind OuterJoinParams in a type of its own, the argument of that kernel alone
// (as ScatterValParams): k_join_outer's argument block is what it was.
struct OuterMarkParams {
    OuterJoinParams o;
    uint32_t*       rmark;  // [ceil(|R| / 32)]
};
void   launch_join_outer_mark(const OuterMarkParams& p, uint32_t jobs, hipStream_t st);
// The outer join's S-only rows (k_outer_emit): {null_pay, payload} of every S tuple of the chunk
// lists whose position is not marked, appended to out (up to cap; *count and *n_s_only += rows).
// Reads the lists (for the chunks' counts), the payloads and the marks: not the words.
struct OuterEmitParams {
    const uint32_t*     ppool;       // S payloads
    const uint32_t*     list;        // S chunk lists
    const uint32_t*     list_start;  // [F + 1]
    const uint32_t*     mark;
    uint32_t            log2F;
    uint32_t            null_pay;
    uint2*              out;
    uint64_t            cap;
    unsigned long long* count;
    unsigned long long* n_s_only;
};
void   launch_outer_emit(const OuterEmitParams& p, uint32_t grid, hipStream_t st);
// The NULL rows of a key column with a validity bitmap (k_null_rows): one row for every i < n whose
// bit is clear, appended to out (up to cap) through the row counter of the join's own emit kernels;
// *count and, when not nullptr, *n_class += rows. kind: NULL_ROWS_ANTI {keys[i], i} (the anti join:
// a NULL S row has no partner), NULL_ROWS_S {null_pay, i} and NULL_ROWS_R {i, null_pay} (the outer
// join's S-only and R-only rows). valid: 4-byte aligned, ceil(n / 8) bytes, no byte past them is read.
enum NullRowsKind : uint32_t { NULL_ROWS_ANTI = 0, NULL_ROWS_S = 1, NULL_ROWS_R = 2 };
struct NullRowsParams {
    const uint8_t*      valid;
    const uint32_t*     keys;      // NULL_ROWS_ANTI: the column (else not read)
    uint64_t            n;         // rows (< 2^31)
    uint32_t            kind;
    uint32_t            null_pay;
    uint2*              out;
    uint64_t            cap;
    unsigned long long* count;
    unsigned long long* n_class;
};
void   launch_null_rows(const NullRowsParams& p, uint32_t grid, hipStream_t st);

// The group join (k_join_group): the materializing join's inputs (m; m.out is not used), no pairs.
// Every R tuple of a job accumulates, in LDS, the number of the job's survivors with its key and the
// sum of their payloads (each sign-extended from int32); after the survivors of a piece its row
// {R.payload, count, sum} (hwbrj_group_row_t as one uint4) is appended to out through m.count, up to
// m.cap rows: every R tuple (all), or those with count > 0. *n_pairs += the counts.
// agg = GRP_COUNT_MINMAX: the accumulator is {count, min, max} of the payloads as int32 (the identities
// INT32_MAX and INT32_MIN where count is 0) and the row {R.payload, count, min, max}
// (hwbrj_group_minmax_row_t as one uint4); everything else is the same.
enum GroupAgg : uint32_t { GRP_COUNT_SUM = 0, GRP_COUNT_MINMAX = 1 };
struct GroupJoinParams {
    MatJoinParams       m;
    uint32_t            all;
    uint32_t            agg;      // GroupAgg
    uint4*              out;
    unsigned long long* n_pairs;  // zero on entry
};
void   launch_join_group(const GroupJoinParams& p, uint32_t jobs, hipStream_t st);
// The accumulating group probe of a prepared build (k_join_group_acc): k_join_group's job with g.all
// off, but at the end of a piece no row is written: every R tuple with a count folds its LDS
// accumulator into acc[R.payload], the build's entry of that R row, which has the row's own layout
// ({row, count, sum} or {row, count, min, max} as one uint4). g.out and g.m.cap are not read;
// *g.m.count += the R tuples with a partner in this batch, *g.n_pairs += their counts. The pointer
// stands behind GroupJoinParams in a type of its own, the argument of that kernel alone (as
// OuterMarkParams): k_join_group's argument block is what it was.
struct GroupAccParams {
    GroupJoinParams g;
    uint4*          acc;  // [|R|]
};
void   launch_join_group_acc(const GroupAccParams& p, uint32_t jobs, hipStream_t st);
// The accumulators' two streaming passes, the same for both forms since an entry is stored as its
// row. init: the identity rows {i, 0, 0, 0} (GRP_COUNT_SUM) or {i, 0, INT32_MAX, INT32_MIN}
// (GRP_COUNT_MINMAX) into rows[0, n). rows: the entries of acc[0, n) (all of them, or those with a
// count) appended to out, up to cap; res[0] += rows, res[1] += their counts. Neither reads R.
void   launch_group_acc_init(uint4* rows, uint64_t n, uint32_t agg, hipStream_t st);
void   launch_group_acc_rows(const uint4* acc, uint64_t n, uint32_t all, uint4* out, uint64_t cap,
                             unsigned long long* res, hipStream_t st);
// The group join's rows of R's NULL keys (k_null_group_rows; GROUP_ALL with a bitmap on R's key
// column): the identity row {i, 0, 0} (GRP_COUNT_SUM) or {i, 0, INT32_MAX, INT32_MIN}
// (GRP_COUNT_MINMAX) of every row i < n whose bit is clear, appended to out (up to cap) through the row
// counter k_join_group adds to (GroupJoinParams::m.count); *count += rows, no pairs. valid: 4-byte
// aligned, ceil(n / 8) bytes, no byte past them is read.
struct NullGroupRowsParams {
    const uint8_t*      valid;
    uint64_t            n;    // rows (< 2^31)
    uint32_t            agg;  // GroupAgg
    uint4*              out;
    uint64_t            cap;
    unsigned long long* count;
};
void   launch_null_group_rows(const NullGroupRowsParams& p, uint32_t grid, hipStream_t st);

void   launch_gen(uint2* out, uint64_t offset, uint64_t count, const GenPlan* d_plan, const Perm& perm,
                  hipStream_t st);
void   launch_zipf(const int32_t* rnd, uint64_t cnt, uint64_t row0, const double* lut,
                   const uint32_t* alphabet, uint32_t size, uint2* out, uint64_t n_above,
                   uint32_t above_base, const Perm& perm, hipStream_t st);
// src (here and in launch_bitpos): SRC_TUPLES (uint2 {key, payload}) or SRC_KEYS (uint32 keys)
void   launch_build_global(const void* R, int src, uint64_t n, const Geometry& g, const CrcTables* tabs,
                           uint32_t* bm, hipStream_t st);
void   launch_probe_global(const void* S, int src, uint64_t n, const Geometry& g, const CrcTables* tabs,
                           const uint32_t* bm, uint32_t* out, uint64_t* out_count, hipStream_t st);
// basic k >= 2: every R key's k bit positions (element j * n + i), then the slices from their
// partitioned chunk lists
void   launch_bitpos(const void* R, int src, uint64_t n, const Geometry& g, uint32_t* out, hipStream_t st);
void   launch_slice_fill(const uint32_t* pool, const uint32_t* list, const uint32_t* list_start,
                         const Geometry& g, uint32_t* slices, hipStream_t st);
size_t scatter_lds_bytes(uint32_t log2F);
size_t scatter_pay_lds_bytes(uint32_t log2F);  // (ScatterParams::ppool set)
enum { SIDE_R = 0, SIDE_S = 1 };  // which relation a scatter partitions (kernel name; S uses g.s_format)
// (src = SRC_KEYS_VAL: SIDE_S with p.ppool and p.src_val set, nothing else; SRC_KEYS_VAL_MASK: the
// same with p a ScatterValParams)
void   launch_scatter(const ScatterParams& p, int src, int side, uint32_t grid, hipStream_t st);
// k_plan: per-(wg, q) list offsets + per-partition chunk / element totals (colc, cole);
// k_list_fill: scans the totals into list / element / item starts [F + 1] and fills the lists.
void   launch_list_fill(const uint32_t* meta, const uint32_t* wg_used, uint64_t cap,
                        uint32_t log2F, const uint32_t* wgq_off, const uint32_t* colc,
                        const uint64_t* cole, uint32_t CH, uint32_t nseg, uint32_t* list_start,
                        uint64_t* elem_start, uint32_t* item_start, uint32_t* list, uint32_t grid,
                        hipStream_t st);
bool   launch_plan(const uint32_t* wgq_chunks, const uint32_t* wgq_elems, uint32_t G,
                   uint32_t log2F, uint32_t* wgq_off, uint32_t* colc, uint64_t* cole,
                   hipStream_t st);
uint32_t probe_chunks_per_item();
size_t   probe_lds_bytes(const Geometry& g, uint32_t* stage_cap, bool pay = false);
size_t slice_lds_bytes(const Geometry& g);
uint32_t build_chunks_per_sweep();  // R chunks per k_build sweep
uint32_t build_sweep_slot();        // out_codes words per k_build sweep
void   launch_build(const BuildParams& p, uint32_t F, hipStream_t st);
void   launch_probe(const ProbeParams& p, uint32_t grid, hipStream_t st);
// basic k >= 2 (k_probe_bitj): bit g.bitj of the words partitioned by its slice, passing words
// appended densely to p.surv; p.filtered += their count
size_t probe_bitj_lds_bytes(const Geometry& g);
void   launch_probe_bitj(const ProbeParams& p, uint32_t grid, hipStream_t st);
// splits skewed jobs (job_surv: survivors per job from k_probe, cleared here) and runs the join
void   launch_join(const JoinParams& p, uint32_t jobs, uint32_t* job_surv, hipStream_t st);
uint32_t join_extra_tasks();
// k_join's partial sums (JoinParams::jsum): join_sum_slots() slots of join_sum_stride() u64 words,
// word 0 matches, 1 probe ticks, 2 total ticks (P.timing); the host adds them up
uint32_t join_sum_slots();
uint32_t join_sum_stride();
uint32_t join_bitmap_log2();  // k_join's bitmap path: job keys v < 2^join_bitmap_log2()
// The kernel constants the data-dependent paths of the scatter, k_join and k_join_mat depend on
// (hwbrj_tables_info: tests derive their shapes from these instead of hard-coding them)
struct PathConstants {
    uint32_t sc_round, sc_flushes;                    // kScRound; kScK * kScThreads flush tasks per round
    uint32_t join_waves, join_fused_sweeps, join_fw, join_fs;  // fused path: kJoinWaves * JFR sweeps, JFW, JFS
    uint32_t join_desc, join_piece, join_task_surv, join_extra, join_tail_u, join_tail_s;
    uint32_t join_rw, join_sw;                        // walk: words per lane of an R / a survivor run
    uint32_t mat_piece, mat_desc, mat_rcap;           // k_join_mat: kMatPiece, kMatDesc, kMatRCap
};
PathConstants path_constants();
void   launch_join_mat(const MatJoinParams& p, uint32_t jobs, hipStream_t st);

// The side passes of the global-bitmap mode (K12): every payload join there is a pass of its own
// after a counting join. launch_mat_build fills an open-addressing table of R (zero on entry,
// mask + 1 slots); every probe then streams S against it through one walk (side_walk), with the
// counting join's filter as a pre-test (g.mode = MODE_NOBLOOM: none). 8-byte rows are appended to
// out[0, cap) through one LDS stage per workgroup (SideStage); the counters also count the rows beyond
// cap. src: SRC_TUPLES, or SRC_KEYS: uint32 key columns whose payload is the row index.
struct SideTable {
    const unsigned long long* tab;
    uint64_t                  mask;
    Geometry                  g;  // the filter: g, slices, bm, tabs
    const uint32_t*           slices;
    const uint32_t*           bm;
    const CrcTables*          tabs;
};
void   launch_mat_build(const void* R, int src, uint64_t n, unsigned long long* tab, uint64_t mask,
                        hipStream_t st);
// Pairs and the outer join: {R.payload, S.payload} of every match; {null_pay, S.payload} for an S
// tuple without a partner (keep_s), and a bit per table slot that was hit (rflag, or nullptr);
// cnt[0] += rows, cnt[1] += S-only rows. Pairs alone: keep_s = 0 and rflag = nullptr (cnt: one word).
void   launch_pair_probe(const void* S, int src, uint64_t n, const void* R, const SideTable& t, uint32_t keep_s,
                         uint32_t null_pay, uint32_t* rflag, uint2* out, uint64_t cap, unsigned long long* cnt,
                         hipStream_t st);
// {R.payload, null_pay} of the table's entries whose slot has no bit in rflag; cnt[0] and cnt[2] += rows
void   launch_outer_rtab(const void* R, int src, const unsigned long long* tab, uint64_t slots,
                         const uint32_t* rflag, uint32_t null_pay, uint2* out, uint64_t cap,
                         unsigned long long* cnt, hipStream_t st);
// The existence join: the walk stops at the first hit; rows {key, payload} on a hit (anti = 0) or on none
void   launch_semi_probe(const void* S, int src, uint64_t n, const SideTable& t, uint32_t anti, uint2* out,
                         uint64_t cap, unsigned long long* count, hipStream_t st);
// The group joins (agg: GroupAgg): every S tuple adds 1 to cnt[row] and its sign-extended payload to
// sum[row] (GRP_COUNT_SUM; both zero on entry), or takes mn[row] and mx[row] with it (GRP_COUNT_MINMAX;
// INT32_MAX and INT32_MIN on entry), of every table entry with its key:
// one element per R row. launch_group_rows then writes the rows of R[0, n) (all of them, or those
// with cnt > 0) to out, up to cap; res[0] += rows, res[1] += their counts.
// SRC_KEYS: S's payloads are the uint32 value column Sv (SRC_TUPLES: not read).
struct GroupAcc {
    uint32_t*           cnt;
    unsigned long long* sum;  // GRP_COUNT_SUM
    int32_t *           mn, *mx;  // GRP_COUNT_MINMAX
};
void   launch_group_probe(const void* S, const void* Sv, int src, uint64_t n, const SideTable& t,
                          const GroupAcc& a, uint32_t agg, hipStream_t st);
void   launch_group_rows(const void* R, int src, uint64_t n, const GroupAcc& a, uint32_t agg, uint32_t all,
                         uint4* out, uint64_t cap, unsigned long long* res, hipStream_t st);

// partitioned multi-GPU join (K13): chunks in list order + rebased entries; receiver lists;
// survivor runs of items packed per destination
// partitioned join, device-side item tables: probe items -> region, survivor totals, their
// exclusive scan sofs [I + 1] and sofs at every partition's first item (bound [F + 1]); received
// items -> exclusive scan of their totals (wscan [n + 1]); the owner's join tables per
// (owned partition, source) pair (tab: first received item, items, first output item)
void   launch_pj_items(const uint32_t* item_start, const uint32_t* list_start, const uint32_t* cnt,
                       uint32_t items_max, uint32_t F, uint32_t nseg, uint32_t CH, uint64_t seg_words, uint32_t NSUB,
                       uint64_t* region, uint32_t* tot, uint64_t* bsum, uint64_t* sofs, uint64_t* bound,
                       hipStream_t st);
// (BI > 0: the async join's padded blocks of BI items / BW words per source, ritems[j] valid items)
void   launch_pj_recv_scan(const uint32_t* cnt, uint32_t n, uint32_t NSUB, uint32_t* tot, uint64_t* bsum,
                           uint64_t* wscan, hipStream_t st, uint32_t BI = 0, const uint32_t* ritems = nullptr);
void   launch_pj_item_tables(const uint32_t* tab, uint32_t pairs, uint32_t W, const uint32_t* rcnt,
                             const uint64_t* wscan, uint32_t NSUB, uint64_t* ibase, uint32_t* icnt, uint32_t* ioff,
                             uint32_t* jobs, hipStream_t st, uint32_t BI = 0, uint64_t BW = 0);
// the async partitioned join's fixed exchange blocks (hwbrj_pjoin_async.cpp; k_pjx_*): R chunks
// gathered into blocks of BR per destination, the owner's R tables from the received counts, the
// survivors packed into blocks of BI items / BW words, the owner's survivor tables, and the exchange
// sizes of the join for the next plan ({flag, R block, item block, word block} maxima)
// (own >= 0: this rank's own block written straight into the receive buffers own_out / own_ent)
void   launch_pjx_gather(const uint32_t* pool, const uint32_t* list, const uint32_t* lstart, uint32_t F, uint32_t QL,
                         uint32_t W, uint64_t BR, void* out, uint32_t* ent, int own, void* own_out, uint32_t* own_ent,
                         uint64_t* flag, hipStream_t st);
void   launch_pjx_rtab(const uint64_t* rc, uint32_t W, uint32_t QL, uint32_t NC, uint64_t BR, uint32_t bsw,
                       int64_t* tab, uint32_t* lsO, uint32_t* swO, uint64_t* flag, hipStream_t st);
void   launch_pjx_surv_pack(const uint32_t* surv, const uint64_t* region, const uint32_t* tot, const uint64_t* sofs,
                            const uint32_t* item_start, const uint64_t* bound, const uint32_t* cnt, uint32_t F,
                            uint32_t QL, uint32_t NSUB, uint64_t BI, uint64_t BW, uint32_t* out, uint32_t* out_cnt,
                            int own, uint32_t* own_out, uint32_t* own_cnt, uint64_t* flag, hipStream_t st);
void   launch_pjx_stab(const uint64_t* rc, uint32_t W, uint32_t QL, uint32_t NC, uint64_t BI, uint64_t BW,
                       uint32_t* tab2, uint32_t* istart, uint32_t* ritems, uint64_t* flag, hipStream_t st);
void   launch_pjx_stat(const uint64_t* rc1, const uint64_t* rc2, const uint32_t* ls, const uint32_t* is,
                       const uint64_t* bd, uint32_t W, uint32_t QL, uint32_t NC, const uint64_t* flag, uint64_t* out,
                       hipStream_t st);
// The synchronous partitioned join's own block (this rank to itself) written straight into the
// receive buffers: elements in [lo, hi) go to out / ent at index + delta (lo = hi: none).
struct PjOwn {
    uint32_t  lo = 0, hi = 0;
    int64_t   delta = 0;
    void*     out = nullptr;
    uint32_t* ent = nullptr;
};
void   launch_pj_gather(const uint32_t* pool, const uint32_t* list, uint32_t n, void* out, uint32_t* ent,
                        hipStream_t st, const PjOwn& own = PjOwn{});
// the native transport's per-destination counts message (k_pj_counts), built on the device
void   launch_pj_counts(const uint32_t* starts, const uint64_t* bound, uint32_t W, uint32_t QL, uint32_t NC,
                        uint64_t status, uint64_t extra, uint64_t extra2, uint64_t* out, hipStream_t st);
void   launch_pj_relist(const uint32_t* rent, const int64_t* tab, uint32_t pairs, uint32_t* list,
                        hipStream_t st);
void   launch_pj_surv_pack(const uint32_t* surv, const uint64_t* region, const uint32_t* tot,
                           const uint64_t* soff, uint32_t n, uint32_t* out, hipStream_t st,
                           const PjOwn& own = PjOwn{});
void   launch_export(const uint32_t* slices, const Geometry& g, uint32_t* out, uint64_t nwords,
                     hipStream_t st);
// A build's filter applied to a key column (k_filter_keys): bit i of out (a validity bitmap of
// ceil(n / 32) dwords, the bits past n clear) = row i is valid and keys[i] passes the filter of the
// partition slices (g: MODE_SLICE_BLOCK or MODE_SLICE_BASIC); *count += the set bits. valid: nullptr
// (every row valid) or ceil(n / 8) bytes, 4-byte aligned, no byte past them read; it may be out
// itself. keys: 16-byte aligned, n < 2^32. grid: the most workgroups to launch. Returns false, with
// nothing launched, for a geometry no prepared build has (not MODE_SLICE_BLOCK and not basic k = 1).
struct FilterKeysParams {
    const uint32_t*     keys;
    const uint8_t*      valid;
    uint64_t            n;
    Geometry            g;
    const uint32_t*     slices;
    const CrcTables*    tabs;
    uint32_t*           out;
    unsigned long long* count;
};
bool   launch_filter_keys(const FilterKeysParams& p, uint32_t grid, hipStream_t st);
// a streaming copy of bytes (multiple of 16) from src to dst, grid workgroups of contiguous ranges
// (hwbrj_copy_bandwidth)
void   launch_copy_bw(const void* src, void* dst, uint64_t bytes, int grid, hipStream_t st);

// every compile-time switch of hwbrj_kernels.hip that differs from the product default ("" for the
// product build); hwbrj_version() appends it
const char* kernel_build_knobs();

// Test hooks (hwbrj_set_test_hook, include/hwbrj.h): explicit process-wide settings that force
// rarely taken paths (no result changes) or inject a failure; all off by default.
struct TestHooks {
    uint32_t join_split    = 0;   // HWBRJ_HOOK_JOIN_SPLIT: survivors per join part (0: the default)
    int      pj_fail_rank  = -1;  // HWBRJ_HOOK_PJ_FAIL_RANK: this rank fails the shard check
    int      bcast_nonroot = 0;   // HWBRJ_HOOK_BCAST_NONROOT: the broadcast join as a non-root rank
    int      pj_plan_div   = 0;   // HWBRJ_HOOK_PJ_PLAN_DIV: async plans' blocks divided by it (overflow)
    int      pj_async_fail = 0;   // HWBRJ_HOOK_PJ_ASYNC_FAIL: async joins run in the failed mode
};
TestHooks& test_hooks();

}  // namespace hwbrj
