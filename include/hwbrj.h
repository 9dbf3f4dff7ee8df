/*
 * hwbrj.h -- C-ABI of libhwbrj.so, the MI355X drop-in for the reference's bloom radix join.
 *
 * Reference interfaces replaced (paths relative to the Briimbo/HwBloomRadixJoin root):
 *   tuple_t, relation_t, threadresult_t, result_t   src/types.h:37-63 (KEY_8B off: 8-byte tuples)
 *   bloom_filter_variant_t, bloom_filter_args_t     src/bloom_filter.h:10, :50-55
 *   BPRO                                            src/parallel_radix_join_bloom.h:34-36
 *                                                   (impl. src/parallel_radix_join_bloom.c:1781-1787)
 *   PRO                                             src/parallel_radix_join.h:33-34 (impl. :1697-1700)
 *   assert_args                                     src/bloom_filter.h:80-81 (impl. bloom_filter.c:25-34)
 *
 * BPRO/PRO keep the reference's contract: caller-owned host relations, a malloc'd result_t the
 * caller frees, the reference's stdout lines ("S-tuples after filter", the timing block), and
 * print + exit(EXIT_FAILURE) on fatal errors. Inputs are copied to HBM (hipMemcpy) outside the
 * timed region, like the reference allocates its tmp buffers before its timer starts.
 *
 * The hwbrj_* entry points are this build's additions: the same join on device-resident data,
 * generators, and test hooks. They return 0 on success and a nonzero code otherwise
 * (message in hwbrj_last_error()).
 */
#ifndef HWBRJ_H
#define HWBRJ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- reference-compatible types (layouts identical to src/types.h, src/bloom_filter.h) ----
 * A translation unit may include the reference's own headers beside this one (its src/main.c
 * relinked against this library): each type is then defined once.
 *   - src/types.h (guard TYPES_H), in either order: this block defines TYPES_H, so a later
 *     types.h is empty, and an earlier one makes this block empty.
 *   - src/bloom_filter.h (guard BLOOM_FILTER_H): include it BEFORE this header (main.c's include
 *     order); its BASIC/BLOCKED enum and bloom_filter_args_t are then used as they are, and the
 *     sectorized variant is HWBRJ_SECTORIZED.
 * This library is the reference's default build (32-bit keys, 8-byte tuples): KEY_8B is refused. */
#ifdef KEY_8B
#error "libhwbrj joins 8-byte tuples (src/types.h without KEY_8B); KEY_8B is not supported"
#endif
#ifndef TYPES_H
#define TYPES_H
typedef int32_t intkey_t;
typedef int32_t value_t;

typedef struct tuple_t    tuple_t;
typedef struct relation_t relation_t;
typedef struct result_t       result_t;
typedef struct threadresult_t threadresult_t;

struct tuple_t {
    intkey_t key;
    value_t  payload;
};

struct relation_t {
    tuple_t * tuples;
    uint64_t  num_tuples;
};

struct threadresult_t {
    int64_t  nresults;
    void *   results;
    uint32_t threadid;
};

struct result_t {
    int64_t          totalresults;
    threadresult_t * resultlist; /* NULL: results are counted, not materialized (reference default) */
    int              nthreads;
};
#endif /* TYPES_H */

#ifndef BLOOM_FILTER_H
/* BASIC = 0 and BLOCKED = 1 as in the reference. SECTORIZED is this build's extension
 * (DESIGN.md "Filter variants"); the reference has no such variant. */
typedef enum { BASIC = 0, BLOCKED = 1, SECTORIZED = 2 } bloom_filter_variant_t;

typedef struct bloom_filter_args_t {
    bloom_filter_variant_t variant;
    uint64_t               m; /* filter size in bits (power of 2, <= 2^32) */
    uint64_t               k; /* hashes per key */
    uint64_t               B; /* block size in bits (power of 2, divides m) */
} bloom_filter_args_t;

void assert_args(bloom_filter_args_t * args);
#endif /* BLOOM_FILTER_H */
#define HWBRJ_SECTORIZED ((bloom_filter_variant_t) 2)

/* ---- drop-in operator boundary ---- */
result_t * BPRO(relation_t * relR, relation_t * relS, int nthreads,
                bloom_filter_args_t * bloom_filter_args);
result_t * PRO(relation_t * relR, relation_t * relS, int nthreads);
/* The reference's other partitioned-join entries (src/main.c:331-339). They differ in the
 * per-partition join function plugged into join_init_run: the histogram join (Kim et al.) for
 * BPRH / PRH, with SIMD compares for BPRHO / PRHO (here: k_join's histogram variants, see
 * hwbrj_join_device_algo), or in running single-threaded (BRJ / RJ: the BPRO / PRO operator on
 * the MI355X). The counts are the same.
 *   BPRH, BPRHO   src/parallel_radix_join_bloom.h:68-87 (impl. :1789-1804)
 *   BRJ           src/parallel_radix_join_bloom.c:1806-1930
 *   PRH, PRHO, RJ src/parallel_radix_join.h:49-82 */
result_t * BPRH(relation_t * relR, relation_t * relS, int nthreads,
                bloom_filter_args_t * bloom_filter_args);
result_t * BPRHO(relation_t * relR, relation_t * relS, int nthreads,
                 bloom_filter_args_t * bloom_filter_args);
result_t * BRJ(relation_t * relR, relation_t * relS, int nthreads,
               bloom_filter_args_t * bloom_filter_args);
result_t * PRH(relation_t * relR, relation_t * relS, int nthreads);
result_t * PRHO(relation_t * relR, relation_t * relS, int nthreads);
result_t * RJ(relation_t * relR, relation_t * relS, int nthreads);
/* The same two operators under prefixed names, for linking next to the reference's own
 * parallel_radix_join*.o (which also define BPRO/PRO): see INTEGRATION.md. */
result_t * hwbrj_BPRO(relation_t * relR, relation_t * relS, int nthreads,
                      bloom_filter_args_t * bloom_filter_args);
result_t * hwbrj_PRO(relation_t * relR, relation_t * relS, int nthreads);

/* ---- device-resident entry points (this build) ---- */
typedef struct hwbrj_stats_t {
    uint64_t filtered;      /* "S-tuples after filter" (= |S| without a filter) */
    int64_t  matches;       /* "Results" */
    int      mode;          /* 0 nobloom, 1 slice-blocked, 2 slice-basic, 3 global fallback */
    int      format;        /* S partition words: 0 codes, 1 packed (code + bit) */
    uint32_t partitions;    /* F */
    uint32_t subparts;      /* join sub-partitions per partition */
    uint32_t slice_segments;
    /* device time (ms, HIP events on the join stream) */
    double   ms_total;
    double   ms_r_scatter;  /* R -> partitions */
    double   ms_r_index;
    double   ms_build;      /* filter slices + R sub-partitioning (or global build) */
    double   ms_s_scatter;  /* S -> partitions (the dominant, HBM-bound kernel) */
    double   ms_s_index;
    double   ms_probe;      /* filter probe + survivor compaction */
    double   ms_surv;       /* survivor sub-partitioning: fused into the probe (k_probe), ~0 */
    double   ms_join;
    double   ms_join_probe; /* the survivor-probing share of ms_join (k_join's probe sections),
                               printed as PROBE-TIME-USECS; synchronous joins only (0 for async) */
    /* The key format between the build / probe and the join ("Join keys"):
     * HWBRJ_JOIN_KEYS_32 32-bit codes, _PACKED packed keys (join_key_bits each), _MIXED packed keys with the survivor
     * runs of unstaged probe items in 32-bit codes. It follows the last waited join on the device
     * (after a join with unstaged items the next one does not pack). */
    int      join_keys;
    uint32_t unstaged_items; /* probe items whose survivors overflowed the probe's LDS stage */
    uint32_t join_key_bits;  /* bits per packed join key: 18 (the bitmap path's keys, hash_shift 14;
                                the north star), 24, or 32 for 32-bit codes */
} hwbrj_stats_t;
enum { HWBRJ_JOIN_KEYS_32 = 0, HWBRJ_JOIN_KEYS_PACKED = 1, HWBRJ_JOIN_KEYS_MIXED = 2 };

/* Join device-resident tuple arrays (tuple_t layout). args == NULL runs PRO (no filter).
 * stream: a hipStream_t (NULL = the library's own stream). The call is synchronous. */
int hwbrj_join_device(const tuple_t * d_R, uint64_t nR, const tuple_t * d_S, uint64_t nS,
                      const bloom_filter_args_t * args, void * stream, hwbrj_stats_t * stats);
/* The same join with the reference's per-partition join function chosen (join_init_run's
 * JoinFunction, src/parallel_radix_join_bloom.c:1789-1804): HWBRJ_ALGO_PRO bucket chaining
 * (:259-329; here an LDS bitmap or counting hash table), HWBRJ_ALGO_PRH the histogram join of
 * Kim et al. (:350-419), HWBRJ_ALGO_PRHO its SIMD form (:441-555; 16-byte LDS compares). The host
 * entries BPRH / BPRHO / PRH / PRHO use them. Counts are identical. */
enum { HWBRJ_ALGO_PRO = 0, HWBRJ_ALGO_PRH = 1, HWBRJ_ALGO_PRHO = 2 };
int hwbrj_join_device_algo(const tuple_t * d_R, uint64_t nR, const tuple_t * d_S, uint64_t nS,
                           const bloom_filter_args_t * args, int algorithm, void * stream,
                           hwbrj_stats_t * stats);
/* The same join, enqueued on `stream` without waiting (back-to-back joins then run without host
 * gaps); the inputs must stay valid until it completes. hwbrj_join_wait() waits for the last join
 * enqueued on this device and fills stats with its counts. An async join records no phase events
 * (each would idle the GPU between the kernels around it), so its ms_* fields are 0; the
 * synchronous entry points measure the phases. */
int hwbrj_join_device_async(const tuple_t * d_R, uint64_t nR, const tuple_t * d_S, uint64_t nS,
                            const bloom_filter_args_t * args, void * stream);
int hwbrj_join_wait(hwbrj_stats_t * stats);
/* Every join enqueued on this device since the last hwbrj_join_wait / hwbrj_join_wait_all (or
 * synchronous join), oldest first, each with its own counts: stats[i] is join i's filtered /
 * matches / mode / join_keys (ms_* only for the last one, and only if it was synchronous). The
 * reference checks every run's count (src/parallel_radix_join_bloom.c:1696-1707 sums each thread's);
 * here every join of a back-to-back run keeps its counts in a device ring of 64 result slots, and an
 * enqueue that finds all 64 in use first collects them on the host (one wait). *n_joins = the
 * number of joins; returns 7 when it exceeds capacity (the oldest `capacity` are written). */
int hwbrj_join_wait_all(hwbrj_stats_t * stats, int capacity, int * n_joins);
/* on != 0: async joins bracket their S scatter (k_scatter_s, the dominant kernel) with timing
 * events on the side stream that runs it beside the R side, and hwbrj_join_wait / _wait_all report
 * its device time as ms_s_scatter of every async join (the other ms_* stay 0). For measuring the
 * kernel in the schedule the back-to-back joins run (bench.py's roofline); off by default, so the
 * timed joins carry no markers. */
int hwbrj_set_async_timing(int on);

/* The counting join on key columns: d_Rkeys / d_Skeys are device arrays of nR / nS int32 keys, the
 * layout a columnar caller already has (no {key, payload} interleaving pass; the counting join
 * never reads payloads, and its scatters read 4 instead of 8 bytes per element). Both sides are
 * columns. The contract is hwbrj_join_device_algo's / hwbrj_join_device_async's in every clause
 * not named here: args == NULL runs PRO; every filter configuration; HWBRJ_ALGO_*; the stream;
 * stats and phase times; the size limits and their codes. The async form is collected by
 * hwbrj_join_wait / hwbrj_join_wait_all and shares the 64-slot result ring with the tuple joins,
 * so the two kinds may be enqueued in any mix. After the synchronous form, hwbrj_tables_info /
 * hwbrj_tables_read answer as after hwbrj_join_device_algo with the same arguments (the partition
 * words do not depend on the input layout).
 * Alignment: a non-empty column must start at a 16-byte boundary (the scatter reads four keys per
 * 16-byte load). A misaligned pointer is refused before any device call: 2 is returned,
 * hwbrj_last_error() says "align", and *stats is not written. A caller sharding a column must
 * therefore cut it at multiples of 4 keys.
 * The pair, existence and outer joins on key columns return row indices (hwbrj_join_keys_pairs_device,
 * hwbrj_join_keys_semi_device, hwbrj_join_keys_outer_device, below), and the group joins on key
 * columns aggregate a value column of S (hwbrj_join_keys_group_device,
 * hwbrj_join_keys_group_minmax_device, below). Not offered on key columns: a value column for R or
 * more than one for S, values other than int32, async forms of the row-index and group joins, the
 * host BPRO family and the partitioned joins; those take tuples only. Validity bitmaps (NULL keys)
 * are offered by the hwbrj_join_keys_*_nulls_device entries below, the group joins with a bitmap for
 * S's value column among them (hwbrj_join_keys_group_nulls_device,
 * hwbrj_join_keys_group_minmax_nulls_device), and not for the async form, a bit offset into the
 * bitmap, or the global-bitmap and basic k >= 2 configurations. */
int hwbrj_join_keys_device(const int32_t * d_Rkeys, uint64_t nR, const int32_t * d_Skeys, uint64_t nS,
                           const bloom_filter_args_t * args, int algorithm, void * stream,
                           hwbrj_stats_t * stats);
int hwbrj_join_keys_device_async(const int32_t * d_Rkeys, uint64_t nR, const int32_t * d_Skeys,
                                 uint64_t nS, const bloom_filter_args_t * args, void * stream);

/* The join with result materialization (the reference's JOIN_RESULT_MATERIALIZE output,
 * src/parallel_radix_join_bloom.c:307-312): d_out[i] = {R.payload, S.payload} of every match, in
 * no particular order. One pass of the partitioned pipeline with every tuple's payload carried
 * beside its word (stats: its counts and phase times); the global-bitmap configurations (basic
 * k = 0, B < 8) run the counting join and a pairs pass instead. capacity is in pairs; with too
 * small a capacity the first `capacity` pairs are written and 7 is returned with *n_out = the
 * match count. ms_materialize (optional) receives the device time of the pairs' production. */
int hwbrj_join_materialize_device(const tuple_t * d_R, uint64_t nR, const tuple_t * d_S,
                                  uint64_t nS, const bloom_filter_args_t * args, tuple_t * d_out,
                                  uint64_t capacity, uint64_t * n_out, void * stream,
                                  hwbrj_stats_t * stats, double * ms_materialize);
/* The existence joins of S against R: d_out receives whole S tuples {key, payload}, in no
 * particular order. HWBRJ_JOIN_SEMI: every S row whose key occurs in R, each exactly once however
 * many R rows share the key. HWBRJ_JOIN_ANTI: every S row whose key does not occur in R (NOT
 * EXISTS). S rows that are equal as tuples are each written, so the output is a sub-multiset of S
 * and SEMI and ANTI together are S. args == NULL runs without a filter; every filter
 * configuration of hwbrj_join_materialize_device is accepted (the global-bitmap ones run the
 * counting join and a side pass). The pipeline is the materializing join's with S's payloads only
 * (R needs none); under ANTI the S tuples the filter rejects never enter sub-partitioning or the
 * join: the join marks the survivors that have a partner and one pass over the partitioned S
 * writes every unmarked tuple ("Existence joins").
 * capacity is in rows: rows beyond it are not written, *n_out always holds the full row count and
 * 7 is returned when it exceeds capacity; capacity 0 with d_out NULL is the count-only form.
 * stats->filtered is "S-tuples after filter" as the counting join of the same arguments reports it
 * (under ANTI too), stats->matches the row count. ms (optional) receives the device time. An
 * unknown kind returns 2 before any device call. Synchronous and single-GPU; it collects pending
 * async joins like the other synchronous entries, and hwbrj_tables_info / hwbrj_tables_read answer
 * 13 after it. */
enum { HWBRJ_JOIN_SEMI = 0, HWBRJ_JOIN_ANTI = 1 };
int hwbrj_join_semi_device(const tuple_t * d_R, uint64_t nR, const tuple_t * d_S, uint64_t nS,
                           const bloom_filter_args_t * args, int kind, tuple_t * d_out,
                           uint64_t capacity, uint64_t * n_out, void * stream,
                           hwbrj_stats_t * stats, double * ms);
/* The outer joins of R and S: d_out receives rows {R.payload, S.payload}, in no particular order.
 * Inner rows: every matching pair, exactly the multiset hwbrj_join_materialize_device returns
 * (duplicate R keys and duplicate S keys give the product). HWBRJ_OUTER_S: also one row
 * {null_payload, S.payload} for every S row whose key does not occur in R (the rows the filter
 * rejects, the survivors that are false positives and the rows of partitions without R alike), each
 * exactly once. HWBRJ_OUTER_R: instead one row {R.payload, null_payload} for every R row whose key
 * does not occur in S; every R tuple gets its own row, so three R rows sharing an unmatched key give
 * three rows. HWBRJ_OUTER_FULL: both. null_payload is the caller's marker: the library does not
 * check that it is absent from the payloads and never reads it back.
 * n_class (optional) receives {inner rows, S-only rows (0 under OUTER_R), R-only rows (0 under
 * OUTER_S)}. args == NULL runs without a filter; every filter configuration of
 * hwbrj_join_materialize_device is accepted (the global-bitmap ones run the counting join and a
 * side pass). One pass of the materializing pipeline: the join marks the S positions that have a
 * partner and flags the R tuples that have one, writes the unflagged R tuples itself, and one pass
 * over the partitioned S payloads writes the unmarked S rows ("Outer joins").
 * capacity is in rows: rows beyond it are not written, *n_out always holds the full row count and
 * 7 is returned when it exceeds capacity; capacity 0 with d_out NULL is the count-only form.
 * stats->filtered is "S-tuples after filter" as the counting join of the same arguments reports
 * it, stats->matches the row count. ms (optional) receives the device time. An unknown kind returns
 * 2 before any device call and without writing *n_out. Synchronous and single-GPU; it collects
 * pending async joins like the other synchronous entries, and hwbrj_tables_info /
 * hwbrj_tables_read answer 13 after it. */
enum { HWBRJ_OUTER_S = 0, HWBRJ_OUTER_R = 1, HWBRJ_OUTER_FULL = 2 };
int hwbrj_join_outer_device(const tuple_t * d_R, uint64_t nR, const tuple_t * d_S, uint64_t nS,
                            const bloom_filter_args_t * args, int kind, int32_t null_payload,
                            tuple_t * d_out, uint64_t capacity, uint64_t * n_out,
                            uint64_t * n_class /* [3], optional */, void * stream,
                            hwbrj_stats_t * stats, double * ms);
/* The pair, existence and outer joins on key columns (hwbrj_join_keys_device's layout): the result
 * is row indices, the gather maps a columnar caller applies to its other columns. Every element's
 * payload is its position in its column, computed by the scatter from the position and never read,
 * so no {key, arange} interleaving pass is needed and the payload scatters read 4 instead of 8 bytes
 * per element. Each entry keeps the contract of its tuple counterpart (hwbrj_join_materialize_device,
 * hwbrj_join_semi_device, hwbrj_join_outer_device) in every clause not named here: capacity in rows,
 * *n_out always the full count, 7 when it exceeds capacity, capacity 0 with d_out NULL as the
 * count-only form, an unknown kind returning 2 without writing *n_out, args == NULL running PRO,
 * every filter configuration (the global-bitmap ones run the counting join on key columns and a side
 * pass), stats, ms, synchronous, collecting pending async joins, and hwbrj_tables_info /
 * hwbrj_tables_read answering as after the tuple form.
 *  - pairs: rows {R row, S row}, exactly the multiset hwbrj_join_materialize_device returns on
 *    {key, row index} tuples.
 *  - semi: rows {key, S row} (a tuple row, as the tuple form writes; the second column is the
 *    gather map), kind HWBRJ_JOIN_SEMI or HWBRJ_JOIN_ANTI.
 *  - outer: rows {R row, S row}, the missing side -1 (a row index is never negative, so there is no
 *    null_payload argument); kind and n_class as in hwbrj_join_outer_device.
 * Refused before any device call: a non-empty column that does not start at a 16-byte boundary (2,
 * "align" in hwbrj_last_error(), nothing written; hwbrj_join_keys_device's rule), nR or nS of 2^31 or
 * more (3, the message names the side: row indices are int32), capacity > 0 with d_out NULL (2). */
int hwbrj_join_keys_pairs_device(const int32_t * d_Rkeys, uint64_t nR, const int32_t * d_Skeys,
                                 uint64_t nS, const bloom_filter_args_t * args, tuple_t * d_out,
                                 uint64_t capacity, uint64_t * n_out, void * stream,
                                 hwbrj_stats_t * stats, double * ms);
int hwbrj_join_keys_semi_device(const int32_t * d_Rkeys, uint64_t nR, const int32_t * d_Skeys,
                                uint64_t nS, const bloom_filter_args_t * args, int kind,
                                tuple_t * d_out, uint64_t capacity, uint64_t * n_out, void * stream,
                                hwbrj_stats_t * stats, double * ms);
int hwbrj_join_keys_outer_device(const int32_t * d_Rkeys, uint64_t nR, const int32_t * d_Skeys,
                                 uint64_t nS, const bloom_filter_args_t * args, int kind,
                                 tuple_t * d_out, uint64_t capacity, uint64_t * n_out,
                                 uint64_t * n_class /* [3], optional */, void * stream,
                                 hwbrj_stats_t * stats, double * ms);
/* Key columns with validity bitmaps: the counting, pair, existence and outer joins on key columns
 * (above) with one bitmap per side, the second half of a columnar key column. A NULL key matches
 * nothing (SQL), so no compaction pass and no index map are needed before the join: row indices are
 * always positions in the caller's columns.
 * The bitmap: d_Rvalid / d_Svalid are device memory in Arrow's layout, row i is bit i & 7 of byte
 * i >> 3 and a set bit means valid. A bitmap holds ceil(n / 8) bytes; no byte past them is read, and
 * the bits past n in the last byte are ignored whatever they hold. A NULL pointer means that side has
 * no NULL keys. With both pointers NULL an entry runs exactly what its counterpart runs (the same
 * kernels, no further loads). There is no bit offset: row 0 is bit 0 of byte 0.
 * Alignment: a non-NULL bitmap of a non-empty column must start at a 4-byte boundary (the NULL-row
 * pass reads it a dword at a time). Otherwise 2 is returned before any device call, "align" is in
 * hwbrj_last_error(), and nothing is written. A caller sharding a masked column must therefore cut it
 * at multiples of 32 rows (which also keeps the key column's multiple of 4).
 * Each result is what the counterpart returns on the valid rows only, with their original row
 * indices, plus:
 *  - count, pairs: nothing more. stats->filtered and stats->matches are the counting join's on the
 *    valid rows; the filter is built from the valid R keys only.
 *  - semi: the valid S rows with a partner among the valid R rows.
 *  - anti: every other S row, each NULL S row included (NOT EXISTS); the key field of a NULL row's
 *    output is whatever the column stores at that position. NULL R rows play no part.
 *  - outer: NULL S rows are S-only rows {-1, S row} under HWBRJ_OUTER_S and HWBRJ_OUTER_FULL, NULL R
 *    rows are R-only rows {R row, -1} under HWBRJ_OUTER_R and HWBRJ_OUTER_FULL, and n_class counts
 *    them in its S-only and R-only entries.
 * The NULL rows are subject to the capacity rule like any others. Every other clause is the
 * counterpart's (capacity, kinds, the 16-byte alignment of the key columns, the 2^31 limits, args ==
 * NULL running PRO, HWBRJ_ALGO_*, synchronous, collecting pending async joins, hwbrj_tables_*).
 * Filters: with a non-NULL bitmap the partition-slice configurations (blocked and sectorized with
 * B >= 8, basic k = 1) and args == NULL are supported, the ones where the pass-1 scatters are the
 * only readers of the columns; the global-bitmap configurations and basic k >= 2 return 9 before any
 * device call (hwbrj_join_partitioned's code for an unsupported filter). With both bitmaps NULL those
 * configurations behave as the counterpart does.
 * The group joins take bitmaps too, one more for S's value column: hwbrj_join_keys_group_nulls_device
 * and hwbrj_join_keys_group_minmax_nulls_device, after the group joins on key columns below.
 * Not offered with validity bitmaps: COUNT(*) beside the aggregates of a nullable value column, the
 * tuple group joins, an async form, tuple relations, a bit offset into the bitmap, the global-bitmap
 * and basic k >= 2 configurations, the host BPRO family and the partitioned joins. */
int hwbrj_join_keys_nulls_device(const int32_t * d_Rkeys, const uint8_t * d_Rvalid, uint64_t nR,
                                 const int32_t * d_Skeys, const uint8_t * d_Svalid, uint64_t nS,
                                 const bloom_filter_args_t * args, int algorithm, void * stream,
                                 hwbrj_stats_t * stats);
int hwbrj_join_keys_pairs_nulls_device(const int32_t * d_Rkeys, const uint8_t * d_Rvalid, uint64_t nR,
                                       const int32_t * d_Skeys, const uint8_t * d_Svalid, uint64_t nS,
                                       const bloom_filter_args_t * args, tuple_t * d_out,
                                       uint64_t capacity, uint64_t * n_out, void * stream,
                                       hwbrj_stats_t * stats, double * ms);
int hwbrj_join_keys_semi_nulls_device(const int32_t * d_Rkeys, const uint8_t * d_Rvalid, uint64_t nR,
                                      const int32_t * d_Skeys, const uint8_t * d_Svalid, uint64_t nS,
                                      const bloom_filter_args_t * args, int kind, tuple_t * d_out,
                                      uint64_t capacity, uint64_t * n_out, void * stream,
                                      hwbrj_stats_t * stats, double * ms);
int hwbrj_join_keys_outer_nulls_device(const int32_t * d_Rkeys, const uint8_t * d_Rvalid, uint64_t nR,
                                       const int32_t * d_Skeys, const uint8_t * d_Svalid, uint64_t nS,
                                       const bloom_filter_args_t * args, int kind, tuple_t * d_out,
                                       uint64_t capacity, uint64_t * n_out,
                                       uint64_t * n_class /* [3], optional */, void * stream,
                                       hwbrj_stats_t * stats, double * ms);
/* The group join of R and S (join and aggregate per build-side row: SELECT R.payload, COUNT(*),
 * SUM(S.payload) ... GROUP BY R-row): d_out receives one row per R row, not per key, in no
 * particular order. count is the number of S rows whose key equals the R row's key, sum the sum of
 * their payloads, each sign-extended from int32 (0 if there are none); three R rows sharing a key
 * give three rows, each with the full count and sum. HWBRJ_GROUP_ALL writes every R row, so the row
 * count is nR and the rows without a partner carry count = 0, sum = 0; HWBRJ_GROUP_MATCHED writes
 * only the rows with count > 0. The sum is exact: nS must be below 2^32 (3 is returned otherwise),
 * so |sum| < 2^63. n_pairs (optional) receives the sum of the counts, which is `matches` of the
 * counting join with the same arguments. args == NULL runs without a filter; every filter
 * configuration of hwbrj_join_materialize_device is accepted (the global-bitmap ones run the
 * counting join and a side pass). It is the materializing pipeline up to the join; the join then
 * accumulates per R tuple on chip and writes no pair ("Group joins"), so the output is
 * bounded by nR whatever the skew.
 * capacity is in rows: rows beyond it are not written, *n_out always holds the full row count and
 * 7 is returned when it exceeds capacity; capacity 0 with d_out NULL is the count-only form. d_out
 * must be 16-byte aligned. stats->filtered is "S-tuples after filter" as the counting join of the
 * same arguments reports it, stats->matches the row count. ms (optional) receives the device time.
 * An unknown kind returns 2 before any device call and without writing *n_out. Synchronous and
 * single-GPU; it collects pending async joins like the other synchronous entries, and
 * hwbrj_tables_info / hwbrj_tables_read answer 13 after it. */
typedef struct hwbrj_group_row_t {   /* 16 bytes */
    int32_t  r_payload;
    uint32_t count;                  /* S rows whose key equals this R row's key */
    int64_t  sum;                    /* sum of their payloads, each sign-extended from int32; 0 if none */
} hwbrj_group_row_t;
enum { HWBRJ_GROUP_MATCHED = 0, HWBRJ_GROUP_ALL = 1 };
int hwbrj_join_group_device(const tuple_t * d_R, uint64_t nR, const tuple_t * d_S, uint64_t nS,
                            const bloom_filter_args_t * args, int kind,
                            hwbrj_group_row_t * d_out, uint64_t capacity, uint64_t * n_out,
                            uint64_t * n_pairs /* optional */, void * stream,
                            hwbrj_stats_t * stats, double * ms);
/* The group join's MIN / MAX form (SELECT R.payload, COUNT(*), MIN(S.payload), MAX(S.payload) ...
 * GROUP BY R-row): hwbrj_join_group_device with another row. count is the number of S rows whose
 * key equals the R row's key, min and max the smallest and the largest of their payloads, compared
 * as signed int32. A row without a partner (only under HWBRJ_GROUP_ALL) carries the identities of
 * the two operations, min = INT32_MAX and max = INT32_MIN, so min > max marks an empty group. No
 * null marker of the caller's is taken: count == 0 already says that the group is empty, and a
 * caller who streams S in batches combines the partial rows of an R row with a plain min and max
 * (and a sum of the counts), without a special case. Every other clause is
 * hwbrj_join_group_device's: kind (an unknown one returns 2 before any device call and without
 * writing *n_out), one row per R row in no particular order, R rows sharing a key each carrying the
 * full count, min and max; capacity in rows, *n_out the full row count, 7 when it exceeds capacity,
 * capacity 0 with d_out NULL as the count-only form; d_out 16-byte aligned (2 otherwise: a row is
 * one 16-byte store); nS below 2^32 (3 otherwise: the count is 32 bits); n_pairs (optional) the sum
 * of the counts; stats->filtered the counting join's value and stats->matches the row count; args
 * == NULL and every filter configuration of hwbrj_join_materialize_device; synchronous, single-GPU,
 * collects pending async joins, and hwbrj_tables_info / hwbrj_tables_read answer 13 after it.
 * COUNT, SUM, MIN and MAX together take both entries ("Group joins: MIN/MAX"). */
typedef struct hwbrj_group_minmax_row_t {   /* 16 bytes */
    int32_t  r_payload;
    uint32_t count;                  /* S rows whose key equals this R row's key */
    int32_t  min;                    /* smallest of their payloads (signed); INT32_MAX if count == 0 */
    int32_t  max;                    /* largest of their payloads (signed);  INT32_MIN if count == 0 */
} hwbrj_group_minmax_row_t;
int hwbrj_join_group_minmax_device(const tuple_t * d_R, uint64_t nR, const tuple_t * d_S, uint64_t nS,
                                   const bloom_filter_args_t * args, int kind,
                                   hwbrj_group_minmax_row_t * d_out, uint64_t capacity,
                                   uint64_t * n_out, uint64_t * n_pairs /* optional */,
                                   void * stream, hwbrj_stats_t * stats, double * ms);
/* The group joins on key columns (hwbrj_join_keys_device's layout) with S's aggregated value in a
 * third column: d_Svals[i] is the value of the S row whose key is d_Skeys[i]. The rows are the tuple
 * entries' rows: r_payload is the R row index (the gather map for R's other columns, as in the
 * row-index joins above), and count, sum, min and max are over d_Svals[i] of the S rows i whose key
 * equals the R row's key. The result is exactly what hwbrj_join_group_device /
 * hwbrj_join_group_minmax_device return on the tuples R = {d_Rkeys[i], i} and S = {d_Skeys[i],
 * d_Svals[i]}, without the pass that interleaves them: the S scatter reads each key with its value,
 * two 16-byte loads per four rows. An aggregate of S row indices would mean nothing, so none is
 * produced and S is not held to 2^31 rows. Each entry keeps its tuple counterpart's contract in every
 * clause not named here: the kinds (an unknown one returns 2 without writing *n_out), capacity in
 * rows, *n_out always the full row count, 7 when it exceeds capacity, capacity 0 with d_out NULL as
 * the count-only form, d_out 16-byte aligned, n_pairs, stats->filtered and stats->matches, ms, args
 * == NULL running PRO, every filter configuration (the global-bitmap ones run the counting join on
 * key columns and the side pass), synchronous, single-GPU, collecting pending async joins, and
 * hwbrj_tables_info / hwbrj_tables_read answering 13 afterwards.
 * Refused before any device call: a non-empty column of the three that does not start at a 16-byte
 * boundary (2, "align" in hwbrj_last_error(), nothing written; hwbrj_join_keys_device's rule, and the
 * value column is loaded as the keys are), nS > 0 with d_Svals NULL (2), nR of 2^31 or more (3, the
 * message names R: the R row index is int32), nS of 2^32 or more (3, the group join's own rule). */
int hwbrj_join_keys_group_device(const int32_t * d_Rkeys, uint64_t nR, const int32_t * d_Skeys,
                                 const int32_t * d_Svals, uint64_t nS,
                                 const bloom_filter_args_t * args, int kind,
                                 hwbrj_group_row_t * d_out, uint64_t capacity, uint64_t * n_out,
                                 uint64_t * n_pairs /* optional */, void * stream,
                                 hwbrj_stats_t * stats, double * ms);
int hwbrj_join_keys_group_minmax_device(const int32_t * d_Rkeys, uint64_t nR, const int32_t * d_Skeys,
                                        const int32_t * d_Svals, uint64_t nS,
                                        const bloom_filter_args_t * args, int kind,
                                        hwbrj_group_minmax_row_t * d_out, uint64_t capacity,
                                        uint64_t * n_out, uint64_t * n_pairs /* optional */,
                                        void * stream, hwbrj_stats_t * stats, double * ms);
/* The group joins on key columns with validity bitmaps: NULL keys on either side and NULL values in
 * S's value column. Three optional bitmaps in the layout of the hwbrj_join_keys_*_nulls_device entries
 * above (row i is bit i & 7 of byte i >> 3, set = valid, ceil(n / 8) bytes, bits past n ignored, no
 * byte past them read, a NULL pointer = no NULLs, no bit offset): d_Rvalid for R's keys, d_Svalid for
 * S's keys and d_Svals_valid for S's values.
 *  - An S row takes part in the join iff its key bit and its value bit are both set. A NULL key
 *    matches nothing; a NULL value is ignored by SUM / MIN / MAX, as in SQL, and is not counted: count
 *    is COUNT(S.val), sum / min / max are over the same rows, count == 0 (and min > max) means the
 *    aggregate is NULL, and n_pairs is the sum of the counts. COUNT(*) over a nullable value column
 *    is what the same call returns without d_Svals_valid; it is not produced beside the aggregates,
 *    because a 16-byte row has no field for it.
 *  - A NULL R row matches nothing. Under HWBRJ_GROUP_ALL it still gets its row, {R row, 0, 0}, or
 *    {R row, 0, INT32_MAX, INT32_MIN} in the MIN / MAX form, so the row count stays nR; under
 *    HWBRJ_GROUP_MATCHED it gets none. These rows are subject to the capacity rule like any others.
 *  - r_payload is the row's position in the caller's column: no compaction pass, no index map.
 *  - stats->filtered and stats->matches are the group join's values on the participating rows:
 *    filtered is the counting join's value on the compacted columns (the filter is built from the
 *    valid R keys only), and with args == NULL and any S bitmap it is the number of participating S
 *    rows.
 * Filters as for the other bitmap entries: the partition-slice configurations (blocked / sectorized
 * with B >= 8, basic k = 1) and args == NULL; the global-bitmap and basic k >= 2 configurations return
 * 9 before any device call when any bitmap is non-NULL. With all three bitmaps NULL an entry runs
 * exactly what hwbrj_join_keys_group_device / hwbrj_join_keys_group_minmax_device run (the same
 * kernels, no further loads). A non-NULL bitmap of a non-empty column must start at a 4-byte boundary:
 * otherwise 2, "align" in hwbrj_last_error(), nothing written. Every other clause is the
 * counterpart's: the kinds (2 for an unknown one, *n_out unwritten), capacity in rows, *n_out always
 * the full row count, 7 above capacity, capacity 0 with d_out NULL as the count-only form, d_out and
 * the three columns 16-byte aligned, nR < 2^31, nS < 2^32, synchronous, collecting pending async
 * joins, hwbrj_tables_* answering 13 afterwards.
 * Not offered: the tuple group joins with NULLs, an async form, a bit offset into a bitmap. */
int hwbrj_join_keys_group_nulls_device(const int32_t * d_Rkeys, const uint8_t * d_Rvalid, uint64_t nR,
                                       const int32_t * d_Skeys, const uint8_t * d_Svalid,
                                       const int32_t * d_Svals, const uint8_t * d_Svals_valid,
                                       uint64_t nS, const bloom_filter_args_t * args, int kind,
                                       hwbrj_group_row_t * d_out, uint64_t capacity, uint64_t * n_out,
                                       uint64_t * n_pairs /* optional */, void * stream,
                                       hwbrj_stats_t * stats, double * ms);
int hwbrj_join_keys_group_minmax_nulls_device(const int32_t * d_Rkeys, const uint8_t * d_Rvalid,
                                              uint64_t nR, const int32_t * d_Skeys,
                                              const uint8_t * d_Svalid, const int32_t * d_Svals,
                                              const uint8_t * d_Svals_valid, uint64_t nS,
                                              const bloom_filter_args_t * args, int kind,
                                              hwbrj_group_minmax_row_t * d_out, uint64_t capacity,
                                              uint64_t * n_out, uint64_t * n_pairs /* optional */,
                                              void * stream, hwbrj_stats_t * stats, double * ms);
/* ---- Prepared builds: build R once, probe it with many S batches (key columns) ----
 * Every join entry above takes both relations and redoes the whole R side (R's scatter, its lists,
 * the build sweeps, the filter slices, the R payloads of the row-index joins) in every call. A caller
 * who streams S in batches builds R once instead: hwbrj_build_keys_device runs exactly the R side of
 * the one-shot join of the same (d_Rkeys, d_Rvalid, args) and keeps what the later stages read in
 * device buffers the build owns; the hwbrj_probe_keys_* entries then run the S pass, the probe and
 * the join of their one-shot counterpart against it.
 *  - purpose: HWBRJ_BUILD_COUNT is the counting join's R side (the packing of the join keys is
 *    decided once, at build time, as a one-shot join decides it, and never changes afterwards);
 *    HWBRJ_BUILD_ROWS is the R side of the joins that return rows, with R's row indices as payloads
 *    and one mark bit per R row, clear after the build (the marking probes below).
 *  - d_Rvalid: R's validity bitmap in the layout and under the alignment rule of the
 *    hwbrj_join_keys_*_nulls_device entries, or NULL: no NULL keys.
 *  - Filters: args == NULL, blocked / sectorized with B >= 8, basic k = 1. The global-bitmap and
 *    basic k >= 2 configurations return 9 before any device call (their pipelines read R again).
 *  - Refused before any device call, *build unwritten: an unknown purpose (2), build == NULL (2), a
 *    non-empty key column that does not start at a 16-byte boundary or a non-NULL bitmap of a
 *    non-empty column that does not start at a 4-byte boundary (2, "align" in hwbrj_last_error()),
 *    nR >= 2^31 under HWBRJ_BUILD_ROWS (3). On any failure *build is left unwritten.
 *  - Synchronous. R's column and bitmap are not read again after it returns: the caller may free or
 *    overwrite them. *ms (optional): the build's device time.
 *  - A build belongs to the caller and to the device that was current when it was made (another
 *    current device: 2 from every entry that takes it). Any number may be alive. hwbrj_release, every
 *    other join entry and the partitioned joins leave them intact; only hwbrj_build_free frees one
 *    (NULL: 0, nothing done). hwbrj_set_filter_broadcast does not apply: slices are built locally.
 * hwbrj_build_info writes the HWBRJ_BI_* words (n >= HWBRJ_BI_COUNT, else 7); BYTES is the device
 * memory the build holds now: what only the build sweeps read (R's chunk pool, metas and lists) is
 * freed before hwbrj_build_keys_device returns. hwbrj_build_export_filter is hwbrj_export_filter for
 * the build's filter: the same bytes as after the one-shot join of the same R and args (5 for a build
 * without a filter, 6 unless nbytes == m / 8).
 * Not offered: tuple relations, async probes, the global-bitmap and basic k >= 2 configurations, the
 * partitioned joins. (Group aggregates over all batches: the group accumulators below.) */
typedef struct hwbrj_build_t hwbrj_build_t; /* opaque; owns its device buffers */
enum { HWBRJ_BUILD_COUNT = 0, HWBRJ_BUILD_ROWS = 1 };
enum {
    HWBRJ_BI_NR = 0, HWBRJ_BI_PURPOSE, HWBRJ_BI_MODE, HWBRJ_BI_F, HWBRJ_BI_NSUB, HWBRJ_BI_KEY_BITS,
    HWBRJ_BI_DEVICE, HWBRJ_BI_BYTES, HWBRJ_BI_MASKED /* R had a bitmap */, HWBRJ_BI_COUNT
};
int hwbrj_build_keys_device(const int32_t * d_Rkeys, const uint8_t * d_Rvalid, uint64_t nR,
                            const bloom_filter_args_t * args, int purpose, void * stream,
                            hwbrj_build_t ** build, double * ms /* optional */);
int hwbrj_build_free(hwbrj_build_t * build);
int hwbrj_build_info(const hwbrj_build_t * build, uint64_t * out, int n);
int hwbrj_build_export_filter(const hwbrj_build_t * build, uint8_t * host_out, uint64_t nbytes);
/* The probes: synchronous, key columns only. Each returns exactly what its one-shot counterpart
 * (hwbrj_join_keys_nulls_device, _pairs_, _semi_, _outer_, _group_, _group_minmax_) returns on the R
 * the build was made from and this S batch: the same rows as a multiset (R rows as positions in the
 * caller's R column, S rows as positions in this batch), the same *n_out, n_class and n_pairs, the
 * same capacity rule (7 above capacity, the count-only form), the same refusals in the same order,
 * and the same stats->filtered, matches, mode, format, partitions, subparts, join_keys and
 * join_key_bits. ms_r_scatter, ms_r_index and ms_build are 0 and ms_total covers the probe only.
 *  - hwbrj_probe_keys_device needs a HWBRJ_BUILD_COUNT build, the five others a HWBRJ_BUILD_ROWS
 *    build (the semi probe reads R's codes only); a NULL build or the wrong purpose: 2 before any
 *    device call.
 *  - After a probe hwbrj_tables_info / hwbrj_tables_read answer 13, and hwbrj_export_filter answers
 *    as if no filter had been built: the filter belongs to the build.
 *  - A probe collects pending async joins like every synchronous entry.
 * hwbrj_probe_keys_outer_device takes two more kinds (the one-shot entries refuse them with 2), for
 * right and full outer joins streamed over batches, where an R row unmatched in one batch may match
 * in a later one: HWBRJ_PROBE_MARK_INNER, the inner pairs of this batch, and HWBRJ_PROBE_MARK_S, the
 * inner pairs plus this batch's S-only rows (HWBRJ_OUTER_S's result, NULL S rows included). Both also
 * set the build's mark bit of every R row with a partner in this batch; no R-only row is written per
 * batch and n_class[2] is 0. hwbrj_build_unmatched_device then writes {R row, -1} of every R row
 * whose mark is clear (NULL R rows included: they never match), in no particular order, under the
 * usual capacity rule (*n_out the full count, 7 above capacity, capacity 0 with d_out NULL counts
 * only), and leaves the marks as they are; hwbrj_build_reset_marks clears them. A streamed full outer
 * join is one HWBRJ_PROBE_MARK_S probe per batch and one hwbrj_build_unmatched_device call; a
 * streamed right outer join uses HWBRJ_PROBE_MARK_INNER; the streamed R-side anti join is the final
 * call alone. Both need a HWBRJ_BUILD_ROWS build (2 otherwise). */
enum { HWBRJ_PROBE_MARK_INNER = 3, HWBRJ_PROBE_MARK_S = 4 };
int hwbrj_probe_keys_device(const hwbrj_build_t * build, const int32_t * d_Skeys, const uint8_t * d_Svalid,
                            uint64_t nS, int algorithm, void * stream, hwbrj_stats_t * stats);
int hwbrj_probe_keys_pairs_device(hwbrj_build_t * build, const int32_t * d_Skeys, const uint8_t * d_Svalid,
                                  uint64_t nS, tuple_t * d_out, uint64_t capacity, uint64_t * n_out,
                                  void * stream, hwbrj_stats_t * stats, double * ms);
int hwbrj_probe_keys_semi_device(hwbrj_build_t * build, const int32_t * d_Skeys, const uint8_t * d_Svalid,
                                 uint64_t nS, int kind, tuple_t * d_out, uint64_t capacity,
                                 uint64_t * n_out, void * stream, hwbrj_stats_t * stats, double * ms);
int hwbrj_probe_keys_outer_device(hwbrj_build_t * build, const int32_t * d_Skeys, const uint8_t * d_Svalid,
                                  uint64_t nS, int kind, tuple_t * d_out, uint64_t capacity,
                                  uint64_t * n_out, uint64_t * n_class /* [3], optional */, void * stream,
                                  hwbrj_stats_t * stats, double * ms);
int hwbrj_probe_keys_group_device(hwbrj_build_t * build, const int32_t * d_Skeys, const uint8_t * d_Svalid,
                                  const int32_t * d_Svals, const uint8_t * d_Svals_valid, uint64_t nS,
                                  int kind, hwbrj_group_row_t * d_out, uint64_t capacity, uint64_t * n_out,
                                  uint64_t * n_pairs /* optional */, void * stream, hwbrj_stats_t * stats,
                                  double * ms);
int hwbrj_probe_keys_group_minmax_device(hwbrj_build_t * build, const int32_t * d_Skeys,
                                         const uint8_t * d_Svalid, const int32_t * d_Svals,
                                         const uint8_t * d_Svals_valid, uint64_t nS, int kind,
                                         hwbrj_group_minmax_row_t * d_out, uint64_t capacity,
                                         uint64_t * n_out, uint64_t * n_pairs /* optional */, void * stream,
                                         hwbrj_stats_t * stats, double * ms);
int hwbrj_build_unmatched_device(hwbrj_build_t * build, tuple_t * d_out, uint64_t capacity, uint64_t * n_out,
                                 void * stream, double * ms /* optional */);
int hwbrj_build_reset_marks(hwbrj_build_t * build);
/* Group accumulators kept across batches (a HWBRJ_BUILD_ROWS build; 2 otherwise). The two group
 * probes above return each batch's partial rows, which the caller must combine per R row. For SELECT
 * R.row, COUNT, SUM | MIN, MAX ... GROUP BY R row over a streamed S the build keeps the aggregates
 * itself: one 16-byte entry per R row and form (agg: HWBRJ_AGG_SUM, hwbrj_group_row_t, or
 * HWBRJ_AGG_MINMAX, hwbrj_group_minmax_row_t), stored as the row it will become and starting at the
 * identity row HWBRJ_GROUP_ALL writes for a row without a partner ({i, 0, 0}, or {i, 0, INT32_MAX,
 * INT32_MIN}). The entries of a form are allocated and initialised at its first accumulating probe or
 * its first hwbrj_build_group_reset: until then the build holds, and HWBRJ_BI_BYTES reports, what it
 * did without them; afterwards BYTES includes them. The two forms are independent and a build may hold
 * both. hwbrj_build_free frees them; hwbrj_release, every other entry (the MATCHED / ALL group probes
 * and the marking probes among them) and other builds leave them alone.
 *  - hwbrj_probe_keys_group_accum_device folds one S batch into the entries of form agg inside the
 *    join kernel and writes no row: no output, no capacity. The batch, its bitmaps and the
 *    participation rule (key bit and value bit both set) are hwbrj_probe_keys_group_device's, and so
 *    are the refusals and their order (NULL build or wrong purpose 2, alignment 2, d_Svals NULL with
 *    nS > 0 2, an unknown agg 2, nS >= 2^32 3, another current device 2), all before any device call
 *    and with nothing written. *n_rows (optional): the R rows with at least one partner in this batch,
 *    and *n_pairs (optional) the pairs of this batch: *n_out and *n_pairs of the HWBRJ_GROUP_MATCHED
 *    probe of the same batch, whose stats this probe's are too (matches = *n_rows, the R phases 0).
 *    Counts are 32 bits and sums 64: the build keeps, per form, the sum of the nS of its accumulating
 *    probes since the last reset, and a probe that would bring it to 2^32 or more returns 3 before
 *    any device call and changes nothing (hwbrj_last_error() names the total). nS = 0 is accepted and
 *    changes no entry. Synchronous; collects pending async joins; hwbrj_tables_* answer 13 afterwards.
 *    Accumulating probes of one build must not overlap: each is synchronous, and a caller with
 *    several threads serialises them per build (an entry is updated without atomics).
 *  - hwbrj_build_group_rows_device writes the rows of everything accumulated since the build or the
 *    last reset: under HWBRJ_GROUP_ALL all nR entries (a NULL R row carries its identity row, since
 *    nothing ever matched it), under HWBRJ_GROUP_MATCHED those with count > 0, in no particular order.
 *    The group join's capacity rule: capacity in rows, *n_out always the full count, 7 above capacity,
 *    capacity 0 with d_out NULL counts only, d_out 16-byte aligned, an unknown kind or agg 2 without
 *    writing *n_out. *n_pairs (optional): the sum of the counts. The entries stay as they are, so a
 *    second call returns the same rows. A form never touched answers as after a reset. R's column is
 *    not read.
 *  - hwbrj_build_group_reset restores the identity rows and the form's running nS (NULL build, a
 *    counting build or an unknown agg: 2). */
enum { HWBRJ_AGG_SUM = 0, HWBRJ_AGG_MINMAX = 1 };
int hwbrj_probe_keys_group_accum_device(hwbrj_build_t * build, const int32_t * d_Skeys,
                                        const uint8_t * d_Svalid, const int32_t * d_Svals,
                                        const uint8_t * d_Svals_valid, uint64_t nS, int agg,
                                        uint64_t * n_rows /* optional */, uint64_t * n_pairs /* optional */,
                                        void * stream, hwbrj_stats_t * stats, double * ms);
int hwbrj_build_group_rows_device(hwbrj_build_t * build, int agg, int kind, void * d_out, uint64_t capacity,
                                  uint64_t * n_out, uint64_t * n_pairs /* optional */, void * stream,
                                  double * ms /* optional */);
int hwbrj_build_group_reset(hwbrj_build_t * build, int agg);
/* The build's filter as a selection bitmap over a key column, for a scan that pushes the filter
 * sideways: one streaming pass over d_Skeys, no partitioning, no survivors, no join. The result is a
 * validity bitmap in the layout every hwbrj_probe_keys_* entry takes as d_Svalid, and a Bloom filter
 * has no false negatives, so a probe given it returns the rows it returns without it; bitmaps of
 * several builds (a star join: one key column of S per dimension) intersect by plain AND.
 *  - Bit i of d_out (bit i & 7 of byte i >> 3) is set iff row i is valid (d_Svalid NULL, or its bit i
 *    set) and d_Skeys[i] passes the filter the build made from R's valid keys: the reference's
 *    contains of the build's variant, m, k, B and seed 42 (src/bloom_filter.c:73-141), false positives
 *    included. The set rows are exactly the rows stats->filtered of hwbrj_probe_keys_device counts for
 *    the same build, batch and bitmap; *n_pass (optional) is their number.
 *  - d_out holds 4 * ceil(nS / 32) bytes and starts at a 4-byte boundary. All of them are written,
 *    the bits past nS in the last dword as 0, and no byte past them.
 *  - Of d_Svalid no byte past ceil(nS / 8) is read and bits past nS are ignored; d_Skeys follows the
 *    key columns' 16-byte rule and no key past nS is read.
 *  - d_out == d_Svalid is allowed when that buffer has d_out's size: each dword of d_Svalid is read
 *    by the thread that overwrites it, before its store (a star join ANDs column after column into one
 *    bitmap this way). Any other overlap of the two is the caller's error.
 *  - Either purpose serves (HWBRJ_BUILD_COUNT or HWBRJ_BUILD_ROWS), with byte-identical results.
 *  - Refused in this order, before any device call and with nothing written: build NULL (2, "build is
 *    NULL"); a build made with args == NULL (5, as hwbrj_build_export_filter); a non-empty key column
 *    off a 16-byte boundary (2, "align"); a non-NULL d_Svalid off a 4-byte boundary with nS > 0 (2,
 *    "align"); d_out off a 4-byte boundary with nS > 0 (2, "align"); nS > 0 with d_out NULL (2);
 *    nS >= 2^32 (3); a current device other than the build's (2).
 *  - nS = 0 returns 0 with *n_pass = 0 and writes nothing to d_out, which may then be NULL.
 *  - Synchronous: on return the bitmap is complete. stream NULL: the library's own. *ms (optional):
 *    the device time of the pass. As every entry of a device's engine it is not thread-safe: calls on
 *    one device, whatever their streams, share one row counter and must not overlap.
 *  - Nothing of the join state is read or written: pending async joins stay pending and are collected
 *    later with their own counts, hwbrj_tables_info, hwbrj_tables_read and hwbrj_export_filter answer
 *    after it as before it, and the build's marks and accumulators are untouched.
 * Not offered: tuple relations, an async form, a bit offset, a compacted row-index list, builds
 * without a filter, the one-shot entries' filter. */
int hwbrj_build_filter_keys_device(const hwbrj_build_t * build, const int32_t * d_Skeys,
                                   const uint8_t * d_Svalid, uint64_t nS, uint8_t * d_out,
                                   uint64_t * n_pass /* optional */, void * stream,
                                   double * ms /* optional */);
/* Host BPRO/PRO (and the PRH/PRHO/RJ entries) fill result_t.resultlist with the reference's
 * chained result buffers (src/tuple_buffer.h) when on (default: on iff HWBRJ_MATERIALIZE is set). */
void hwbrj_set_materialize(int on);
/* Host BPRO/PRO (and the PRH/PRHO/BRJ/RJ entries) range-shard S into `gpus` shards, shard g on
 * visible device g mod hwbrj_device_count(), R replicated (the reference's per-thread chunking of S,
 * src/parallel_radix_join_bloom.c:1646-1670, one host thread per device); counts are summed.
 * 0 (default) takes HWBRJ_GPUS from the environment, else 1. More shards than devices run one after
 * the other on each device (a G-GPU rehearsal on fewer GPUs). Returns 0, or 2 for gpus < 0. */
int  hwbrj_set_gpus(int gpus);

/* ---- partitioned multi-GPU join (this build) ----
 * Rank `rank` of `world` holds an R shard and an S shard (any split, e.g. range shards). Radix
 * partition q of the F partitions belongs to rank q / (F / world). Every rank scatters its R shard,
 * sends each partition's chunks to the owner, which builds that partition's filter slice and join
 * runs; the slices are all-gathered (the filter bitmap broadcast, in 1/world pieces), every rank
 * scatters and probes its S shard against the whole filter and sends each partition's survivors
 * to the owner, which joins them. stats->filtered: this rank's S survivors; stats->matches: the
 * matches of its partitions (the sums over ranks are the join's counts). nR_total = |R| over all
 * ranks (the filter geometry depends on it). Supported: blocked/sectorized filters, basic k = 1
 * and no filter (args NULL); returns 9 otherwise. world must divide F (a power of two <= F).
 *
 * The transport is the caller's (RCCL through torch.distributed, gloo, peer copies). Every call is
 * synchronous; device buffers are the caller's, named by slot (hwbrj_pj_slot_t). */
typedef enum {
    HWBRJ_PJ_R_SEND = 0, HWBRJ_PJ_R_SEND_ENT, HWBRJ_PJ_R_RECV, HWBRJ_PJ_R_RECV_ENT,
    HWBRJ_PJ_SLICES, HWBRJ_PJ_S_SEND, HWBRJ_PJ_S_RECV, HWBRJ_PJ_M_SEND, HWBRJ_PJ_M_RECV,
    HWBRJ_PJ_NSLOTS
} hwbrj_pj_slot_t;

typedef struct hwbrj_exchange_t {
    void * ctx;
    /* device buffer `slot` of at least `bytes` bytes (kept until the next request for the slot) */
    void * (*buffer)(void * ctx, int slot, uint64_t bytes);
    /* host all-to-all: send[j n .. (j + 1) n) goes to rank j, recv[j n ..) comes from rank j */
    int (*alltoall_u64)(void * ctx, const uint64_t * send, uint64_t * recv, uint64_t n);
    /* device all-to-all of byte blocks between slot buffers: [soff[j], soff[j] + sbytes[j]) of
     * send_slot goes to rank j; rank j's block lands at roff[j] of recv_slot (rbytes[j] bytes) */
    int (*alltoallv)(void * ctx, int send_slot, const uint64_t * soff, const uint64_t * sbytes,
                     int recv_slot, const uint64_t * roff, const uint64_t * rbytes);
    /* device all-gather in place: block j = [j bytes, (j + 1) bytes) of slot, from rank j */
    int (*allgather)(void * ctx, int slot, uint64_t bytes);
} hwbrj_exchange_t;

int hwbrj_join_partitioned(const hwbrj_exchange_t * x, int rank, int world, const tuple_t * d_R,
                           uint64_t nR, uint64_t nR_total, const tuple_t * d_S, uint64_t nS,
                           const bloom_filter_args_t * args, hwbrj_stats_t * stats);

/* ---- native RCCL transport (this build) ----
 * One communicator per device (one rank per GPU). hwbrj_comm_unique_id fills the 128-byte
 * ncclUniqueId on one rank; the caller hands the bytes to every rank (torch.distributed, MPI, a
 * file), and each calls hwbrj_comm_init on its device. librccl.so.1 is loaded at the first call
 * (HWBRJ_RCCL_LIB overrides the path); 31 = it could not be loaded, 30 = an RCCL error, 32 = no
 * communicator.
 *   hwbrj_join_partitioned_rccl  hwbrj_join_partitioned over the communicator: the R-chunk and
 *                                survivor all-to-alls (grouped ncclSend / ncclRecv) and the slice
 *                                all-gather (in-place ncclAllGather) run on the join's stream;
 *                                only the per-rank counts that size the all-to-alls reach the host.
 *   hwbrj_set_filter_broadcast   the replicated design (hwbrj_join_device*, S sharded, R on every
 *                                rank) with the north_star's bitmap broadcast: rank 0 builds the
 *                                filter slices, ncclBroadcast sends them to every rank on the join
 *                                stream; the other ranks only sub-partition R for the join. Off by
 *                                default (every rank rebuilds the slices from its R).
 *                                Slice modes only (blocked/sectorized, basic k = 1); a collective:
 *                                every rank must enqueue the same joins. */
int hwbrj_comm_unique_id(uint8_t * unique_id_out /* 128 bytes */);
int hwbrj_comm_init(const uint8_t * unique_id /* 128 bytes */, int world, int rank);
int hwbrj_comm_destroy(void);
int hwbrj_comm_info(int * world, int * rank);
int hwbrj_set_filter_broadcast(int on);
int hwbrj_join_partitioned_rccl(const tuple_t * d_R, uint64_t nR, uint64_t nR_total,
                                const tuple_t * d_S, uint64_t nS, const bloom_filter_args_t * args,
                                hwbrj_stats_t * stats);
/* The same join enqueued without host waits (no reference counterpart; the reference joins one
 * relation pair per process run). Every variable all-to-all is padded to a plan's block bounds
 * (the largest blocks of an earlier synchronous join of the same shapes + 12.5 % + 64, agreed by
 * all ranks), so counts messages, padded exchanges, the owner's tables, build, probe and join are
 * all enqueued on the join stream and up to 8 joins can be in flight. The first call (and the call
 * after a plan was dropped) runs synchronously and makes the plan. A block that does not fit sets
 * a device flag that is max-reduced over the ranks at the end of the join: its wait reruns it
 * synchronously on every rank (same counts; a new plan). A rank whose shard sizes or filter
 * differ from the plan's takes part with empty messages and flags the join the same way.
 * A collective: every rank makes the same calls in the same order (hwbrj_release and
 * hwbrj_comm_destroy included: they drop the joins in flight and the plan's buffers). The inputs
 * must stay valid and unchanged until the join's wait returns.
 *   hwbrj_join_partitioned_wait  collects the oldest enqueued join (FIFO): 0 or its error; stats:
 *                                counts, and ms_total = its device time between its first and last
 *                                operation on the join stream (0 phase times)
 *   hwbrj_pj_async_info          out[16]: plan valid, BR (chunks), BI (items), BW (words), async
 *                                joins, synchronous plan joins, overflow reruns, plans made, joins
 *                                in flight, the last rerun's flag (1 overflow, 2 a rank in the
 *                                failed mode), the last join's largest R / item / word block. */
int hwbrj_join_partitioned_rccl_async(const tuple_t * d_R, uint64_t nR, uint64_t nR_total,
                                      const tuple_t * d_S, uint64_t nS,
                                      const bloom_filter_args_t * args);
/* The async join over the caller's transport (the hwbrj_exchange_t callbacks of
 * hwbrj_join_partitioned): the same plan, padded layout, device tables, overflow flag and failed
 * mode, with the exchanges made by the callbacks (host-synchronous, so this form has host waits;
 * it is what lets several ranks share one GPU in tests). The exchange's callbacks and context must
 * stay valid until the join's wait returns. Collected by hwbrj_join_partitioned_wait. */
int hwbrj_join_partitioned_async(const hwbrj_exchange_t * x, int rank, int world, const tuple_t * d_R,
                                 uint64_t nR, uint64_t nR_total, const tuple_t * d_S, uint64_t nS,
                                 const bloom_filter_args_t * args);
int hwbrj_join_partitioned_wait(hwbrj_stats_t * stats);
int hwbrj_pj_async_info(uint64_t * out /* 16 */);

/* Fill d_out / out with the reference generator's key multiset (src/generator.c:304-415 with
 * `nthreads` generator threads) in a seeded permuted order; payload = row index. */
int hwbrj_generate_device(tuple_t * d_out, uint64_t n, uint32_t nthreads, uint64_t maxid,
                          uint64_t threshold, double selectivity, uint64_t seed, void * stream);
/* Rows [offset, offset + count) of the same n-row relation (for range-sharding S over ranks). */
int hwbrj_generate_device_range(tuple_t * d_out, uint64_t n, uint64_t offset, uint64_t count,
                                uint32_t nthreads, uint64_t maxid, uint64_t threshold,
                                double selectivity, uint64_t seed, void * stream);
int hwbrj_generate_host(tuple_t * out, uint64_t n, uint32_t nthreads, uint64_t maxid,
                        uint64_t threshold, double selectivity, uint64_t seed, int host_threads);

/* ---- the reference's rand()-driven generators, on the host, bit-exact ----
 * Each seeds its own restatement of glibc rand() (srand(seed), src/generator.c:75-81) and draws in
 * the reference's order, so keys AND order equal the reference's relation for the same seed.
 *   hwbrj_create_relation_nonunique          src/generator.c:585-605 (random_gen, :271-279):
 *                                            keys in [0, maxid), payload = row
 *   hwbrj_create_relation_nonunique_from_pk  src/generator.c:608-646 (--non-unique S)
 *   hwbrj_create_relation_fk_from_pk         src/generator.c:531-582 (--full-range S)
 *   hwbrj_create_relation_zipf               src/generator.c:659-676 + src/genzipf.c:28-158 (-z S);
 *                                            payload = row (the reference leaves it uninitialised)
 *   hwbrj_nonunique_threshold                src/main.c:421-427 (threshold for R and S) */
uint64_t hwbrj_nonunique_threshold(uint64_t r_size, double selectivity, int full_range);
int      hwbrj_create_relation_nonunique(tuple_t * out, uint64_t n, int64_t maxid, uint32_t seed);
int      hwbrj_create_relation_nonunique_from_pk(tuple_t * out, uint64_t n, const tuple_t * pk,
                                                 uint64_t npk, int64_t threshold,
                                                 double selectivity, uint32_t seed);
int      hwbrj_create_relation_fk_from_pk(tuple_t * out, uint64_t n, const tuple_t * pk,
                                          uint64_t npk, int64_t threshold, double selectivity,
                                          uint32_t seed);
int      hwbrj_create_relation_zipf(tuple_t * out, uint64_t n, uint64_t alphabet_size,
                                    double theta, uint32_t seed, int host_threads);
/* The -z relation generated straight into HBM (binary searches on the GPU): selectivity = 1 gives
 * exactly hwbrj_create_relation_zipf's relation. selectivity < 1 is this build's extension for
 * BASELINE config 5 (the reference ignores -q with -z): floor(n (1 - q)) rows chosen by a seeded
 * permutation get unique keys above the alphabet. stream: hipStream_t or NULL. */
int      hwbrj_create_relation_zipf_device(tuple_t * d_out, uint64_t n, uint64_t alphabet_size,
                                           double theta, uint32_t seed, double selectivity,
                                           int host_threads, void * stream);
/* The first n values rand() returns after srand(seed) (test hook for the restatement). */
int      hwbrj_rand_stream(uint32_t seed, int32_t * out, uint64_t n);

/* Relation files, the reference's PERSIST_RELATIONS output (the only on-disk format; the CLI's
 * --persist writes R.tbl / S.tbl / Out.tbl like a -DPERSIST_RELATIONS reference build):
 *   hwbrj_write_relation         src/generator.c:250-263 write_relation ("#KEY, VAL" header,
 *                                "key payload" lines); -R / -S read it back
 *   hwbrj_write_result_relation  src/tuple_buffer.h:155-236 write_result_relation: the pairs of a
 *                                materializing BPRO / PRO result ("R.payload S.payload", no header) */
int hwbrj_write_relation(const relation_t * rel, const char * filename);
int hwbrj_write_result_relation(const result_t * res, const char * filename);

/* The filter built by the last join, in the reference's byte layout (src/bloom_filter.c:143-171:
 * m/8 bytes, bit h of a block at byte h>>3, bit h&7). nbytes must be m/8. */
int hwbrj_export_filter(uint8_t * host_out, uint64_t nbytes);

/* Test-only readback of the tables the last collected synchronous join on this device left in HBM
 * (hwbrj_join_device, hwbrj_join_device_algo, hwbrj_join_materialize_device), so tests can check
 * every stage's output and tell which k_join path each (partition, sub) job must have taken. Both
 * calls only copy device memory to the host: no kernel is launched, nothing on the device is
 * written. They return 0, or
 *    6  no synchronous join has completed on this device (or its buffers were released)
 *   12  a join is pending (enqueued and not yet waited for): nothing is read
 *   13  the last join's pipeline keeps other tables: basic k >= 2 (the repartitioning passes) and
 *       the partitioned multi-GPU joins; also HWBRJ_TAB_NPARTS after a materializing join
 *    7  out / host_out too small (hwbrj_tables_read: *bytes holds the need)
 *    2  unknown table, or no such item
 *   hwbrj_tables_info  out[HWBRJ_TI_COUNT] (n = capacity in words): that join's geometry and launch
 *                      shape, and the kernel constants its data-dependent paths depend on.
 *   hwbrj_tables_read  table `which` in the compact layout the kernels index; *bytes = its size.
 *                      F, NSUB, sweeps, items, jobs, slot: the words of hwbrj_tables_info. */
enum {
    HWBRJ_TI_MODE = 0,    /* hwbrj_stats_t.mode */
    HWBRJ_TI_FORMAT,      /* hwbrj_stats_t.format */
    HWBRJ_TI_F,           /* partitions */
    HWBRJ_TI_NSUB,        /* join sub-partitions per partition */
    HWBRJ_TI_SUB_SHIFT,   /* sub = (code >> sub_shift) & (NSUB - 1); 0: the partition is no code digit */
    HWBRJ_TI_HASH_SHIFT,  /* job key v = code >> hash_shift */
    HWBRJ_TI_NSEG,        /* slice segments (probe items per piece) */
    HWBRJ_TI_BITMAP,      /* 1: the join's direct-address bitmap holds the job keys */
    HWBRJ_TI_JKIND,       /* HWBRJ_ALGO_* */
    HWBRJ_TI_KEY_BITS,    /* bits per R key of the build's sweep slots: 18, 24, or 32 (codes) */
    HWBRJ_TI_GRID,        /* scatter workgroups G */
    HWBRJ_TI_CH,          /* chunks per probe item */
    HWBRJ_TI_BSW,         /* chunks per build sweep */
    HWBRJ_TI_SLOT,        /* words per build sweep slot */
    HWBRJ_TI_STAGE_CAP,   /* survivors a probe item can stage (more: an unstaged item, 32-bit codes) */
    HWBRJ_TI_SWEEPS,      /* build sweeps over all partitions */
    HWBRJ_TI_ITEMS,       /* probe items over all partitions */
    HWBRJ_TI_JOBS,        /* F * NSUB */
    HWBRJ_TI_MAT,         /* 1: the materializing join (k_join_mat) */
    HWBRJ_TI_SPLIT,       /* survivors per join part (HWBRJ_HOOK_JOIN_SPLIT, else kJoinTaskSurv) */
    /* kernel constants (hwbrj_kernels.hip) */
    HWBRJ_TI_SC_ROUND,    /* kScRound: elements per scatter workgroup round */
    HWBRJ_TI_SC_FLUSHES,  /* kScK * kScThreads: flush tasks of a round before its "rare" loop */
    HWBRJ_TI_J_FUSED,     /* kJoinWaves * HWBRJ_JFR: sweeps of a fused-path job (at most) */
    HWBRJ_TI_J_FW,        /* HWBRJ_JFW: fused path, R words per lane before tail_run */
    HWBRJ_TI_J_FS,        /* HWBRJ_JFS: fused path, survivor runs per wave loaded with R's */
    HWBRJ_TI_J_WAVES,     /* kJoinWaves */
    HWBRJ_TI_J_DESC,      /* kJoinDesc: run descriptors per batch */
    HWBRJ_TI_J_PIECE,     /* kJoinPiece: R keys per hash-table piece */
    HWBRJ_TI_J_TASK_SURV, /* kJoinTaskSurv */
    HWBRJ_TI_J_EXTRA,     /* kJoinExtra: extra parts the task table holds */
    HWBRJ_TI_J_TAIL_U,    /* kJoinTailU */
    HWBRJ_TI_J_TAIL_S,    /* kJoinTailS */
    HWBRJ_TI_J_RW,        /* HWBRJ_JRW: walk, words per lane of an R run before tail_run */
    HWBRJ_TI_J_SW,        /* HWBRJ_JSW: ... of a survivor run */
    HWBRJ_TI_M_PIECE,     /* kMatPiece: k_join_mat's R tuples per piece, survivors per batch */
    HWBRJ_TI_M_DESC,      /* kMatDesc: its run descriptors per batch */
    HWBRJ_TI_M_RCAP,      /* kMatRCap: R tuples of a job on its bitmap path (at most) */
    HWBRJ_TI_COUNT
};
enum {
    HWBRJ_TAB_R_ELEM_START = 0, /* u64 [F + 1]  first R element of each partition */
    HWBRJ_TAB_S_ELEM_START,     /* u64 [F + 1]  S elements (the global-bitmap mode: its survivors) */
    HWBRJ_TAB_R_SWEEP_START,    /* u32 [F + 1]  first build sweep of each partition */
    HWBRJ_TAB_R_RUN_CNT,        /* u32 [sweeps][NSUB]  keys of each (sweep, sub) run */
    HWBRJ_TAB_R_RUN_OFF,        /* u32 [sweeps][NSUB]  its key offset inside the sweep's slot */
    HWBRJ_TAB_R_KEYS,           /* u32 [sweeps][slot]  the sweep slots, raw (packed keys or codes) */
    HWBRJ_TAB_S_LIST_START,     /* u32 [F + 1]  first S chunk-list entry of each partition */
    HWBRJ_TAB_S_ITEM_START,     /* u32 [F + 1]  first probe item of each partition */
    HWBRJ_TAB_SURV_CNT,         /* u32 [items][NSUB]  survivors of each (item, sub) run */
    HWBRJ_TAB_SURV_OFF,         /* u32 [items][NSUB]  its key offset in the item region; bit 31: packed */
    HWBRJ_TAB_NPARTS,           /* u32 [jobs + 1]  parts of each job, then the extra parts requested */
    HWBRJ_TAB_SURV_ITEM = 64    /* + item: u32 words of that probe item's survivor region, raw */
};
int hwbrj_tables_info(uint64_t * out, int n);
int hwbrj_tables_read(int which, void * host_out, uint64_t cap_bytes, uint64_t * bytes);

/* Cycles per second of the counter behind BPRO's "RUNTIME TOTAL, BUILD, PART (cycles)" line (the
 * reference's rdtsc timers, src/rdtsc.h:35-68), calibrated once against the steady clock. */
uint64_t hwbrj_tsc_hz(void);

/* Measurement utility (no reference counterpart): the device's streaming copy rate, for the
 * roofline's measured-copy figure beside the spec peak. Copies `bytes` (a
 * multiple of 16) between two fresh device buffers `reps` times; *gbps = (read + write bytes) /
 * the median copy time. Returns 0, or an error code (device memory). */
int hwbrj_copy_bandwidth(uint64_t bytes, int reps, double * gbps);

/* Scalar hashes on the host (test hooks): crc32c(seed,key) and CrapWow(seed,key). */
uint32_t hwbrj_hash_crc(uint32_t seed, int32_t key);
uint32_t hwbrj_hash_crapwow(uint32_t seed, int32_t key);

int          hwbrj_device_count(void);
int          hwbrj_set_device(int device);
void         hwbrj_release(void); /* free all device buffers */
const char * hwbrj_last_error(void);
/* "hwbloomradixjoin_amd <version> (gfx950)"; a build whose kernels were compiled with any
 * non-default switch (tuning A/Bs, dev ablations) appends " knobs: NAME=value ..." naming them,
 * and so does every test hook that is set (hwbrj_set_test_hook). */
const char * hwbrj_version(void);

/* Test hooks (no reference counterpart): process-wide settings that force rarely taken paths or
 * inject a failure, so tests can reach them on one GPU. All are off (0 / -1) by default; none
 * changes a result except HWBRJ_HOOK_BCAST_NONROOT = 2, which exists to show that it would.
 *   HWBRJ_HOOK_JOIN_SPLIT     value > 0: the join's skew split cuts every (partition, sub) job
 *                             above `value` survivors into parts (counts unchanged).
 *   HWBRJ_HOOK_PJ_FAIL_RANK   rank `value` of a partitioned join fails its shard-size check
 *                             (code 3), as an oversized shard would; -1 = off.
 *   HWBRJ_HOOK_BCAST_NONROOT  with hwbrj_set_filter_broadcast(1): this rank runs the broadcast
 *                             join's non-root side (k_build writes no filter slices; they come
 *                             from ncclBroadcast, which at world 1 leaves the buffer as it is).
 *                             1 = as is, 2 = the slice buffer zeroed first (the filter is then
 *                             empty unless something writes it: the counts must drop). Honoured
 *                             only on a communicator of world 1 (a test setting; ignored by a
 *                             real multi-rank broadcast).
 *   HWBRJ_HOOK_PJ_PLAN_DIV    value > 0: the async partitioned join's plans get their block bounds
 *                             divided by `value`, so the next async join overflows and is rerun
 *                             synchronously (counts unchanged).
 *   HWBRJ_HOOK_PJ_ASYNC_FAIL  1: this rank runs every async partitioned join in the failed mode
 *                             (empty messages, failed status), as after a shape change: every rank
 *                             reruns the join synchronously (counts unchanged).
 * Returns 0, or 2 for an unknown hook or a value out of range. */
enum {
    HWBRJ_HOOK_JOIN_SPLIT     = 1,
    HWBRJ_HOOK_PJ_FAIL_RANK   = 2,
    HWBRJ_HOOK_BCAST_NONROOT  = 3,
    HWBRJ_HOOK_PJ_PLAN_DIV    = 4,
    HWBRJ_HOOK_PJ_ASYNC_FAIL  = 5
};
int          hwbrj_set_test_hook(int hook, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* HWBRJ_H */
