// hwbrj_api.cpp -- the C-ABI of libhwbrj.so (include/hwbrj.h): the drop-in BPRO / PRO operator
// boundary with the reference's stdout contract, plus device-resident entry points.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <x86intrin.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "hwbrj_engine.h"

namespace hwbrj {

static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }

}  // namespace hwbrj

using namespace hwbrj;

// include/hwbrj.h's opaque build: Engine's Build behind a tag that tells a build from any other pointer
struct hwbrj_build_t : hwbrj::Build {};

extern "C" {

const char* hwbrj_last_error(void) { return g_last_error.c_str(); }
// "<name> <version> (gfx950) src <hash>", then " knobs: ..." naming every compile-time switch of
// the kernels that differs from the product default. The hash is the Makefile's stamp of the
// product sources and flags ("dev" otherwise).
#ifndef HWBRJ_SRC_SHA
#define HWBRJ_SRC_SHA "dev"
#endif
// Test hooks that are set (hwbrj_set_test_hook) are named too, so a bench line or a PMC stamp of a
// process that set one shows it.
const char* hwbrj_version(void) {
    static const std::string base = kernel_build_knobs();
    // one immutable string per distinct hook state, never freed: a pointer returned earlier stays
    // valid whatever hooks are set later
    static std::mutex            mu;
    static std::set<std::string> interned;
    std::lock_guard<std::mutex>  lk(mu);
    std::string        k = base;
    const TestHooks&   h = test_hooks();
    auto add = [&](const std::string& w) { k += (k.empty() ? "" : " ") + w; };
    if (h.join_split) add("HWBRJ_HOOK_JOIN_SPLIT=" + std::to_string(h.join_split));
    if (h.pj_fail_rank >= 0) add("HWBRJ_HOOK_PJ_FAIL_RANK=" + std::to_string(h.pj_fail_rank));
    if (h.bcast_nonroot) add("HWBRJ_HOOK_BCAST_NONROOT=" + std::to_string(h.bcast_nonroot));
    if (h.pj_plan_div) add("HWBRJ_HOOK_PJ_PLAN_DIV=" + std::to_string(h.pj_plan_div));
    if (h.pj_async_fail) add("HWBRJ_HOOK_PJ_ASYNC_FAIL=" + std::to_string(h.pj_async_fail));
    const std::string v = std::string("hwbloomradixjoin_amd 0.6 (gfx950) src " HWBRJ_SRC_SHA) +
                          (k.empty() ? "" : " knobs: " + k);
    return interned.insert(v).first->c_str();
}

int hwbrj_set_test_hook(int hook, int64_t value) {
    TestHooks& h = test_hooks();
    switch (hook) {
        case HWBRJ_HOOK_JOIN_SPLIT:
            if (value < 0 || value > 0xFFFFFFFFll) break;
            h.join_split = (uint32_t) value;
            return 0;
        case HWBRJ_HOOK_PJ_FAIL_RANK:
            h.pj_fail_rank = (int) value;
            return 0;
        case HWBRJ_HOOK_BCAST_NONROOT:
            if (value < 0 || value > 2) break;
            h.bcast_nonroot = (int) value;
            return 0;
        case HWBRJ_HOOK_PJ_PLAN_DIV:
            if (value < 0 || value > 1000000) break;
            h.pj_plan_div = (int) value;
            return 0;
        case HWBRJ_HOOK_PJ_ASYNC_FAIL:
            if (value < 0 || value > 1) break;
            h.pj_async_fail = (int) value;
            return 0;
        default:
            set_last_error("unknown test hook");
            return 2;
    }
    set_last_error("test hook value out of range");
    return 2;
}

int hwbrj_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int hwbrj_set_device(int device) {
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) {
        set_last_error(std::string("hipSetDevice: ") + hipGetErrorString(e));
        return 1;
    }
    return 0;
}

void hwbrj_release(void) {
    Engine* e = engine_for_current_device();
    if (e) e->release();
}

// The rate of the cycle counter behind "RUNTIME TOTAL, BUILD, PART (cycles)" (the reference's
// rdtsc timers, src/rdtsc.h:35-68), measured once against the steady clock over 50 ms.
uint64_t hwbrj_tsc_hz(void) {
    static const uint64_t hz = [] {
        const auto     t0 = std::chrono::steady_clock::now();
        const uint64_t c0 = __rdtsc();
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
        const uint64_t c1 = __rdtsc();
        const double   s  = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return (uint64_t) ((double) (c1 - c0) / s);
    }();
    return hz;
}

int hwbrj_copy_bandwidth(uint64_t bytes, int reps, double* gbps) {
    if (!gbps || reps < 1 || bytes < 16 || bytes % 16) {
        set_last_error("hwbrj_copy_bandwidth: bytes must be a positive multiple of 16, reps >= 1");
        return 1;
    }
    void *a = nullptr, *b = nullptr;
    if (hipMalloc(&a, bytes) != hipSuccess || hipMalloc(&b, bytes) != hipSuccess) {
        if (a) (void) hipFree(a);
        set_last_error("hwbrj_copy_bandwidth: hipMalloc failed");
        return 6;
    }
    hipStream_t st = nullptr;
    hipEvent_t  e0 = nullptr, e1 = nullptr;
    int         rc = 0;
    std::vector<float> ms;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
        hipEventCreate(&e1) != hipSuccess || hipMemsetAsync(a, 1, bytes, st) != hipSuccess) {
        rc = 3;
    } else {
        int dev = 0, cus = 256;
        (void) hipGetDevice(&dev);
        (void) hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        launch_copy_bw(a, b, bytes, cus, st);  // warm-up (page mapping, clocks)
        for (int r = 0; r < reps && rc == 0; r++) {
            float t = 0;
            (void) hipEventRecord(e0, st);
            launch_copy_bw(a, b, bytes, cus, st);
            (void) hipEventRecord(e1, st);
            if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess) rc = 3;
            ms.push_back(t);
        }
    }
    if (rc == 0) {
        std::sort(ms.begin(), ms.end());
        *gbps = 2.0 * (double) bytes / (ms[ms.size() / 2] * 1e-3) / 1e9;
    } else {
        set_last_error(std::string("hwbrj_copy_bandwidth: ") + hipGetErrorString(hipGetLastError()));
    }
    if (e0) (void) hipEventDestroy(e0);
    if (e1) (void) hipEventDestroy(e1);
    if (st) (void) hipStreamDestroy(st);
    (void) hipFree(a);
    (void) hipFree(b);
    return rc;
}

uint32_t hwbrj_hash_crc(uint32_t seed, int32_t key) { return crc_f_bitwise(seed ^ (uint32_t) key); }
uint32_t hwbrj_hash_crapwow(uint32_t seed, int32_t key) { return crapwow(seed, (uint32_t) key); }

// A counting join's request
static JoinReq count_req(int algorithm, int layout, const KeyMasks& masks = KeyMasks{}) {
    JoinReq q;
    q.jkind  = algorithm;
    q.layout = layout;
    q.masks  = masks;
    return q;
}

int hwbrj_join_device(const tuple_t* d_R, uint64_t nR, const tuple_t* d_S, uint64_t nS,
                      const bloom_filter_args_t* args, void* stream, hwbrj_stats_t* stats) {
    Engine* e = engine_for_current_device();
    if (!e) return 10;  // (last error set by engine_for_current_device)
    return e->run(JoinIn{d_R, nR, d_S, nS, args, (hipStream_t) stream}, count_req(0, SRC_TUPLES), stats);
}

int hwbrj_join_device_algo(const tuple_t* d_R, uint64_t nR, const tuple_t* d_S, uint64_t nS,
                           const bloom_filter_args_t* args, int algorithm, void* stream,
                           hwbrj_stats_t* stats) {
    Engine* e = engine_for_current_device();
    if (!e) return 10;
    return e->run(JoinIn{d_R, nR, d_S, nS, args, (hipStream_t) stream}, count_req(algorithm, SRC_TUPLES), stats);
}

int hwbrj_join_device_async(const tuple_t* d_R, uint64_t nR, const tuple_t* d_S, uint64_t nS,
                            const bloom_filter_args_t* args, void* stream) {
    Engine* e = engine_for_current_device();
    if (!e) return 10;  // (last error set by engine_for_current_device)
    return e->run_async(JoinIn{d_R, nR, d_S, nS, args, (hipStream_t) stream});
}

// Key columns: a non-empty column starts at a 16-byte boundary (the scatter's 16-byte loads and its
// workgroup ranges in units of 4 keys). Checked before any device call.
static bool keys_aligned(const int32_t* d_Rkeys, uint64_t nR, const int32_t* d_Skeys, uint64_t nS) {
    const bool bad_r = nR && ((uintptr_t) d_Rkeys & 15u), bad_s = nS && ((uintptr_t) d_Skeys & 15u);
    if (!bad_r && !bad_s) return true;
    set_last_error(std::string("key column ") + (bad_r ? "R" : "S") +
                   " is not 16-byte aligned (shard a column at multiples of 4 keys)");
    return false;
}

int hwbrj_join_keys_device(const int32_t* d_Rkeys, uint64_t nR, const int32_t* d_Skeys, uint64_t nS,
                           const bloom_filter_args_t* args, int algorithm, void* stream,
                           hwbrj_stats_t* stats) {
    if (!keys_aligned(d_Rkeys, nR, d_Skeys, nS)) return 2;
    Engine* e = engine_for_current_device();
    if (!e) return 10;
    return e->run(JoinIn{d_Rkeys, nR, d_Skeys, nS, args, (hipStream_t) stream}, count_req(algorithm, SRC_KEYS), stats);
}

int hwbrj_join_keys_device_async(const int32_t* d_Rkeys, uint64_t nR, const int32_t* d_Skeys,
                                 uint64_t nS, const bloom_filter_args_t* args, void* stream) {
    if (!keys_aligned(d_Rkeys, nR, d_Skeys, nS)) return 2;
    Engine* e = engine_for_current_device();
    if (!e) return 10;
    return e->run_async(JoinIn{d_Rkeys, nR, d_Skeys, nS, args, (hipStream_t) stream}, 0, SRC_KEYS);
}

int hwbrj_join_partitioned(const hwbrj_exchange_t* x, int rank, int world, const tuple_t* d_R,
                           uint64_t nR, uint64_t nR_total, const tuple_t* d_S, uint64_t nS,
                           const bloom_filter_args_t* args, hwbrj_stats_t* stats) {
    if (!x || !x->buffer || !x->alltoall_u64 || !x->alltoallv || !x->allgather) {
        set_last_error("incomplete exchange (hwbrj_exchange_t)");
        return 2;
    }
    Engine* e = engine_for_current_device();
    if (!e) return 10;
    return e->join_partitioned(x, rank, world, (const uint2*) d_R, nR, nR_total, (const uint2*) d_S, nS,
                               args, stats);
}

int hwbrj_join_wait(hwbrj_stats_t* stats) {
    Engine* e = engine_for_current_device();
    if (!e) return 10;
    return e->wait(stats);
}

int hwbrj_set_async_timing(int on) {
    Engine* e = engine_for_current_device();
    if (!e) return 10;
    e->set_async_timing(on != 0);
    return 0;
}

int hwbrj_join_wait_all(hwbrj_stats_t* stats, int capacity, int* n_joins) {
    if (capacity < 0 || (capacity > 0 && !stats)) {
        set_last_error("stats must hold capacity >= 0 entries");
        return 2;
    }
    Engine* e = engine_for_current_device();
    if (!e) return 10;
    return e->wait_all(stats, capacity, n_joins);
}

// Every payload join runs its partitioned pipeline (Engine::run: st->matches rows, st->ms_total); the
// global-bitmap mode (basic k = 0 or B < 8: kRcMatGlobal) falls back to the counting join (its
// filter and its "S-tuples after filter") plus the kind's side pass (Engine::side: *n rows, *ms its
// device time). *n = all rows (also beyond the capacity), and st->matches with it; *x: the kind's
// extra counts.
// Pairs in the global-bitmap mode: the side pass writes the first cap pairs whatever the count
// (k_pair_probe's row stage holds every store to out[0, cap)); only the count-only form, cap = 0,
// stays a count.
// b: a probe of a prepared build (always the partitioned pipeline: a build has no global-bitmap mode).
static int pipeline_or_side_pass(Engine* e, const JoinIn& in, const JoinReq& req, hwbrj_stats_t* st, uint64_t* n,
                                 JoinExtras* x, double* ms, const Build* b = nullptr) {
    int rc = e->run(in, req, st, x, b);
    if (rc == 0) {
        *n = (uint64_t) st->matches;
        if (ms) *ms = st->ms_total;
        return 0;
    }
    if (rc != kRcMatGlobal) return rc;
    rc = e->run(in, count_req(0, req.layout), st);
    if (rc) return rc;
    if (req.kind == JOIN_PAIRS) {
        *n = (uint64_t) st->matches;
        if (req.cap == 0) return 0;  // (count only: nothing could be written)
        uint64_t m = 0;
        rc         = e->side(in, req, &m, x, ms);
        if (rc == 0 && m != *n) {
            set_last_error("materialized pairs differ from the counted matches");
            return 8;
        }
        return rc;
    }
    rc = e->side(in, req, n, x, ms);
    if (rc) return rc;
    st->matches = (int64_t) *n;
    return 0;
}

// The shared tail of the payload joins' entries, after their argument checks: the join, the kind's
// extra counts (n_class: the outer join's three; n_pairs: the group join's), then the caller's outputs
// and the capacity rule (what: "match" or "row"). *ms = the device time of the rows' production.
// The build of a probe belongs to the current device (after the entry's argument checks)
static int build_device_ok(const Build* b, Engine* e) {
    if (!b || b->device == e->device()) return 0;
    set_last_error("the build belongs to another device than the current one");
    return 2;
}

static int payload_join(const JoinIn& in, const JoinReq& req, const char* what, uint64_t* n_out, hwbrj_stats_t* stats,
                        double* ms, uint64_t* n_class = nullptr, uint64_t* n_pairs = nullptr,
                        const Build* b = nullptr) {
    Engine* e = engine_for_current_device();
    if (!e) return 10;  // (last error set by engine_for_current_device)
    if (const int rc = build_device_ok(b, e)) return rc;
    hwbrj_stats_t st;
    uint64_t      n = 0;
    JoinExtras    x;
    if (const int rc = pipeline_or_side_pass(e, in, req, &st, &n, &x, ms, b)) return rc;
    if (n_class)
        for (int i = 0; i < 3; i++) n_class[i] = x.cls[i];
    if (n_pairs) *n_pairs = x.pairs;
    if (stats) *stats = st;
    if (n_out) *n_out = n;
    if (n > req.cap) {
        set_last_error(std::string("output capacity below the ") + what + " count (*n_out holds the count)");
        return 7;
    }
    return 0;
}

// What every payload request shares: the kind, the output, the layout (SRC_TUPLES, or SRC_KEYS: d_R
// and d_S are int32 key columns and every payload is the row index) and the bitmaps
static JoinReq payload_req(JoinKind kind, void* d_out, uint64_t capacity, int layout, const KeyMasks& masks) {
    JoinReq q = count_req(0, layout, masks);
    q.kind    = kind;
    q.out     = d_out;
    q.cap     = capacity;
    return q;
}

// The materializing join (JOIN_PAIRS).
static int join_pairs(const void* d_R, uint64_t nR, const void* d_S, uint64_t nS,
                      const bloom_filter_args_t* args, tuple_t* d_out, uint64_t capacity, uint64_t* n_out,
                      void* stream, hwbrj_stats_t* stats, double* ms_materialize, int layout,
                      const KeyMasks& masks = KeyMasks{}, const Build* b = nullptr) {
    return payload_join(JoinIn{d_R, nR, d_S, nS, args, (hipStream_t) stream},
                        payload_req(JOIN_PAIRS, d_out, capacity, layout, masks), "match", n_out, stats, ms_materialize,
                        nullptr, nullptr, b);
}

int hwbrj_join_materialize_device(const tuple_t* d_R, uint64_t nR, const tuple_t* d_S, uint64_t nS,
                                  const bloom_filter_args_t* args, tuple_t* d_out,
                                  uint64_t capacity, uint64_t* n_out, void* stream,
                                  hwbrj_stats_t* stats, double* ms_materialize) {
    return join_pairs(d_R, nR, d_S, nS, args, d_out, capacity, n_out, stream, stats, ms_materialize, SRC_TUPLES);
}

// Key columns with row indices as payloads (hwbrj_join_keys_pairs / _semi / _outer_device): the
// columns' alignment rule, and rows that fit the int32 row index. Checked before any device call.
static int keys_rows_ok(const int32_t* d_Rkeys, uint64_t nR, const int32_t* d_Skeys, uint64_t nS) {
    if (!keys_aligned(d_Rkeys, nR, d_Skeys, nS)) return 2;
    if (nR >= (1ull << 31) || nS >= (1ull << 31)) {
        set_last_error(std::string("key column ") + (nR >= (1ull << 31) ? "R" : "S") +
                       " has 2^31 rows or more (row indices are int32)");
        return 3;
    }
    return 0;
}

int hwbrj_join_keys_pairs_device(const int32_t* d_Rkeys, uint64_t nR, const int32_t* d_Skeys, uint64_t nS,
                                 const bloom_filter_args_t* args, tuple_t* d_out, uint64_t capacity,
                                 uint64_t* n_out, void* stream, hwbrj_stats_t* stats, double* ms) {
    if (const int rc = keys_rows_ok(d_Rkeys, nR, d_Skeys, nS)) return rc;
    if (capacity > 0 && !d_out) {
        set_last_error("d_out must hold capacity rows");
        return 2;
    }
    return join_pairs(d_Rkeys, nR, d_Skeys, nS, args, d_out, capacity, n_out, stream, stats, ms, SRC_KEYS);
}

// The existence join: the partitioned pipeline with S's payloads (JOIN_SEMI); the
// global-bitmap mode runs the counting join (its filter and its "S-tuples after filter") and the
// existence side pass.
static int join_semi(const void* d_R, uint64_t nR, const void* d_S, uint64_t nS,
                     const bloom_filter_args_t* args, int kind, tuple_t* d_out, uint64_t capacity,
                     uint64_t* n_out, void* stream, hwbrj_stats_t* stats, double* ms, int layout,
                     const KeyMasks& masks = KeyMasks{}, const Build* b = nullptr) {
    if (kind != HWBRJ_JOIN_SEMI && kind != HWBRJ_JOIN_ANTI) {  // (before any device call)
        set_last_error("unknown existence join kind (HWBRJ_JOIN_SEMI, HWBRJ_JOIN_ANTI)");
        return 2;
    }
    if (capacity > 0 && !d_out) {
        set_last_error("d_out must hold capacity rows");
        return 2;
    }
    JoinReq req = payload_req(JOIN_SEMI, d_out, capacity, layout, masks);
    req.anti    = kind == HWBRJ_JOIN_ANTI;
    return payload_join(JoinIn{d_R, nR, d_S, nS, args, (hipStream_t) stream}, req, "row", n_out, stats, ms, nullptr,
                        nullptr, b);
}

int hwbrj_join_semi_device(const tuple_t* d_R, uint64_t nR, const tuple_t* d_S, uint64_t nS,
                           const bloom_filter_args_t* args, int kind, tuple_t* d_out, uint64_t capacity,
                           uint64_t* n_out, void* stream, hwbrj_stats_t* stats, double* ms) {
    return join_semi(d_R, nR, d_S, nS, args, kind, d_out, capacity, n_out, stream, stats, ms, SRC_TUPLES);
}

int hwbrj_join_keys_semi_device(const int32_t* d_Rkeys, uint64_t nR, const int32_t* d_Skeys, uint64_t nS,
                                const bloom_filter_args_t* args, int kind, tuple_t* d_out, uint64_t capacity,
                                uint64_t* n_out, void* stream, hwbrj_stats_t* stats, double* ms) {
    if (const int rc = keys_rows_ok(d_Rkeys, nR, d_Skeys, nS)) return rc;
    return join_semi(d_Rkeys, nR, d_Skeys, nS, args, kind, d_out, capacity, n_out, stream, stats, ms, SRC_KEYS);
}

// The outer join: the materializing pipeline with marks over S and matched flags over R
// (JOIN_OUTER); the global-bitmap mode runs the counting join (its filter and its "S-tuples
// after filter") and the outer side pass.
static int join_outer(const void* d_R, uint64_t nR, const void* d_S, uint64_t nS,
                      const bloom_filter_args_t* args, int kind, int32_t null_payload, tuple_t* d_out,
                      uint64_t capacity, uint64_t* n_out, uint64_t* n_class, void* stream,
                      hwbrj_stats_t* stats, double* ms, int layout, const KeyMasks& masks = KeyMasks{},
                      Build* b = nullptr) {
    // (the marking kinds belong to the probes of a prepared build: its marks outlive the call)
    const bool marking = b && (kind == HWBRJ_PROBE_MARK_INNER || kind == HWBRJ_PROBE_MARK_S);
    if (kind != HWBRJ_OUTER_S && kind != HWBRJ_OUTER_R && kind != HWBRJ_OUTER_FULL && !marking) {  // (before any device call)
        set_last_error(b ? "unknown outer probe kind (HWBRJ_OUTER_S, _R, _FULL, HWBRJ_PROBE_MARK_INNER, _S)"
                         : "unknown outer join kind (HWBRJ_OUTER_S, HWBRJ_OUTER_R, HWBRJ_OUTER_FULL)");
        return 2;
    }
    if (capacity > 0 && !d_out) {
        set_last_error("d_out must hold capacity rows");
        return 2;
    }
    JoinReq req  = payload_req(JOIN_OUTER, d_out, capacity, layout, masks);
    req.keep_s   = marking ? kind == HWBRJ_PROBE_MARK_S : kind != HWBRJ_OUTER_R;
    req.keep_r   = !marking && kind != HWBRJ_OUTER_S;
    req.rmark    = marking ? b->marks.as<uint32_t>() : nullptr;
    req.null_pay = (uint32_t) null_payload;
    return payload_join(JoinIn{d_R, nR, d_S, nS, args, (hipStream_t) stream}, req, "row", n_out, stats, ms, n_class,
                        nullptr, b);
}

int hwbrj_join_outer_device(const tuple_t* d_R, uint64_t nR, const tuple_t* d_S, uint64_t nS,
                            const bloom_filter_args_t* args, int kind, int32_t null_payload, tuple_t* d_out,
                            uint64_t capacity, uint64_t* n_out, uint64_t* n_class, void* stream,
                            hwbrj_stats_t* stats, double* ms) {
    return join_outer(d_R, nR, d_S, nS, args, kind, null_payload, d_out, capacity, n_out, n_class, stream, stats, ms,
                      SRC_TUPLES);
}

// (the missing side of a row is -1: a row index is never negative)
int hwbrj_join_keys_outer_device(const int32_t* d_Rkeys, uint64_t nR, const int32_t* d_Skeys, uint64_t nS,
                                 const bloom_filter_args_t* args, int kind, tuple_t* d_out, uint64_t capacity,
                                 uint64_t* n_out, uint64_t* n_class, void* stream, hwbrj_stats_t* stats,
                                 double* ms) {
    if (const int rc = keys_rows_ok(d_Rkeys, nR, d_Skeys, nS)) return rc;
    return join_outer(d_Rkeys, nR, d_Skeys, nS, args, kind, -1, d_out, capacity, n_out, n_class, stream, stats, ms,
                      SRC_KEYS);
}

// Key columns with validity bitmaps (hwbrj_join_keys_*_nulls_device). Checked before any device call,
// after the counterpart's own rules: a bitmap of a non-empty column starts at a 4-byte boundary
// (k_null_rows reads it a dword at a time), and a bitmap needs a filter whose scatters are the only
// readers of the columns (masks_supported: 9 otherwise). Both bitmaps NULL: neither check, and the
// counterpart's call.
// d_Svvalid: the bitmap of S's value column (the group joins on key columns), under the same rules.
static int masks_ok(const uint8_t* d_Rvalid, uint64_t nR, const uint8_t* d_Svalid, uint64_t nS,
                    const bloom_filter_args_t* args, bool pl, const uint8_t* d_Svvalid = nullptr) {
    if (!d_Rvalid && !d_Svalid && !d_Svvalid) return 0;
    const bool bad_r = d_Rvalid && nR && ((uintptr_t) d_Rvalid & 3u), bad_s = d_Svalid && nS && ((uintptr_t) d_Svalid & 3u);
    const bool bad_v = d_Svvalid && nS && ((uintptr_t) d_Svvalid & 3u);
    if (bad_r || bad_s || bad_v) {
        set_last_error(std::string("validity bitmap of ") + (bad_r ? "R" : bad_s ? "S" : "S's value column") +
                       " is not 4-byte aligned (shard a masked column at multiples of 32 rows)");
        return 2;
    }
    Geometry    g;
    std::string err;
    if (!plan_geometry(args, nR, &g, &err, pl)) {
        set_last_error(err);
        return 2;
    }
    if (!masks_supported(g)) {
        set_last_error("validity bitmaps need partition slices (blocked/sectorized, basic k = 1, or no filter)");
        return kRcMaskFilter;
    }
    return 0;
}

int hwbrj_join_keys_nulls_device(const int32_t* d_Rkeys, const uint8_t* d_Rvalid, uint64_t nR, const int32_t* d_Skeys,
                                 const uint8_t* d_Svalid, uint64_t nS, const bloom_filter_args_t* args, int algorithm,
                                 void* stream, hwbrj_stats_t* stats) {
    if (!keys_aligned(d_Rkeys, nR, d_Skeys, nS)) return 2;
    if (const int rc = masks_ok(d_Rvalid, nR, d_Svalid, nS, args, false)) return rc;
    Engine* e = engine_for_current_device();
    if (!e) return 10;
    return e->run(JoinIn{d_Rkeys, nR, d_Skeys, nS, args, (hipStream_t) stream},
                  count_req(algorithm, SRC_KEYS, KeyMasks{d_Rvalid, d_Svalid}), stats);
}

int hwbrj_join_keys_pairs_nulls_device(const int32_t* d_Rkeys, const uint8_t* d_Rvalid, uint64_t nR,
                                       const int32_t* d_Skeys, const uint8_t* d_Svalid, uint64_t nS,
                                       const bloom_filter_args_t* args, tuple_t* d_out, uint64_t capacity,
                                       uint64_t* n_out, void* stream, hwbrj_stats_t* stats, double* ms) {
    if (const int rc = keys_rows_ok(d_Rkeys, nR, d_Skeys, nS)) return rc;
    if (const int rc = masks_ok(d_Rvalid, nR, d_Svalid, nS, args, true)) return rc;
    if (capacity > 0 && !d_out) {  // (after the bitmaps' checks, as in the semi and outer entries)
        set_last_error("d_out must hold capacity rows");
        return 2;
    }
    return join_pairs(d_Rkeys, nR, d_Skeys, nS, args, d_out, capacity, n_out, stream, stats, ms, SRC_KEYS,
                      KeyMasks{d_Rvalid, d_Svalid});
}

int hwbrj_join_keys_semi_nulls_device(const int32_t* d_Rkeys, const uint8_t* d_Rvalid, uint64_t nR,
                                      const int32_t* d_Skeys, const uint8_t* d_Svalid, uint64_t nS,
                                      const bloom_filter_args_t* args, int kind, tuple_t* d_out, uint64_t capacity,
                                      uint64_t* n_out, void* stream, hwbrj_stats_t* stats, double* ms) {
    if (const int rc = keys_rows_ok(d_Rkeys, nR, d_Skeys, nS)) return rc;
    if (const int rc = masks_ok(d_Rvalid, nR, d_Svalid, nS, args, true)) return rc;
    return join_semi(d_Rkeys, nR, d_Skeys, nS, args, kind, d_out, capacity, n_out, stream, stats, ms, SRC_KEYS,
                     KeyMasks{d_Rvalid, d_Svalid});
}

int hwbrj_join_keys_outer_nulls_device(const int32_t* d_Rkeys, const uint8_t* d_Rvalid, uint64_t nR,
                                       const int32_t* d_Skeys, const uint8_t* d_Svalid, uint64_t nS,
                                       const bloom_filter_args_t* args, int kind, tuple_t* d_out, uint64_t capacity,
                                       uint64_t* n_out, uint64_t* n_class, void* stream, hwbrj_stats_t* stats,
                                       double* ms) {
    if (const int rc = keys_rows_ok(d_Rkeys, nR, d_Skeys, nS)) return rc;
    if (const int rc = masks_ok(d_Rvalid, nR, d_Svalid, nS, args, true)) return rc;
    return join_outer(d_Rkeys, nR, d_Skeys, nS, args, kind, -1, d_out, capacity, n_out, n_class, stream, stats, ms,
                      SRC_KEYS, KeyMasks{d_Rvalid, d_Svalid});
}

// The group join: the materializing pipeline up to the join, then per-R-tuple accumulators instead of
// pairs (JOIN_GROUP); the global-bitmap mode runs the counting join (its filter and its
// "S-tuples after filter") and the group side pass. Both aggregate sets (agg: GroupAgg) share it:
// their rows are 16 bytes and every clause of the contract is the same.
// layout SRC_KEYS: d_R, d_S are int32 key columns, R's payload is its row index and the aggregated S
// payloads are the value column d_Svals (SRC_TUPLES: nullptr).
static int join_group(const void* d_R, uint64_t nR, const void* d_S, const void* d_Svals, uint64_t nS,
                      const bloom_filter_args_t* args, int kind, uint32_t agg, void* d_out, uint64_t capacity,
                      uint64_t* n_out, uint64_t* n_pairs, void* stream, hwbrj_stats_t* stats, double* ms,
                      int layout, const KeyMasks& masks = KeyMasks{}, const Build* b = nullptr) {
    static_assert(sizeof(hwbrj_group_row_t) == 16 && sizeof(hwbrj_group_minmax_row_t) == 16,
                  "a row is one 16-byte store");
    if (kind != HWBRJ_GROUP_MATCHED && kind != HWBRJ_GROUP_ALL) {  // (before any device call)
        set_last_error("unknown group join kind (HWBRJ_GROUP_MATCHED, HWBRJ_GROUP_ALL)");
        return 2;
    }
    if (capacity > 0 && !d_out) {
        set_last_error("d_out must hold capacity rows");
        return 2;
    }
    if (((uintptr_t) d_out & 15u) != 0) {
        set_last_error("d_out must be 16-byte aligned (a row is written as one 16-byte store)");
        return 2;
    }
    if (nS >= (1ull << 32)) {  // a count is 32 bits wide, and 2^32 payloads keep |sum| < 2^63
        set_last_error("group join: |S| must be below 2^32 rows (32-bit counts)");
        return 3;
    }
    JoinReq req = payload_req(JOIN_GROUP, d_out, capacity, layout, masks);
    req.all     = kind == HWBRJ_GROUP_ALL;
    req.agg     = agg;
    req.s_val   = d_Svals;
    return payload_join(JoinIn{d_R, nR, d_S, nS, args, (hipStream_t) stream}, req, "row", n_out, stats, ms, nullptr,
                        n_pairs, b);
}

int hwbrj_join_group_device(const tuple_t* d_R, uint64_t nR, const tuple_t* d_S, uint64_t nS,
                            const bloom_filter_args_t* args, int kind, hwbrj_group_row_t* d_out,
                            uint64_t capacity, uint64_t* n_out, uint64_t* n_pairs, void* stream,
                            hwbrj_stats_t* stats, double* ms) {
    return join_group(d_R, nR, d_S, nullptr, nS, args, kind, GRP_COUNT_SUM, d_out, capacity, n_out, n_pairs, stream,
                      stats, ms, SRC_TUPLES);
}

// The group join's MIN / MAX form: k_join_group's {count, min, max} accumulators ("Group
// joins: MIN/MAX").
int hwbrj_join_group_minmax_device(const tuple_t* d_R, uint64_t nR, const tuple_t* d_S, uint64_t nS,
                                   const bloom_filter_args_t* args, int kind, hwbrj_group_minmax_row_t* d_out,
                                   uint64_t capacity, uint64_t* n_out, uint64_t* n_pairs, void* stream,
                                   hwbrj_stats_t* stats, double* ms) {
    return join_group(d_R, nR, d_S, nullptr, nS, args, kind, GRP_COUNT_MINMAX, d_out, capacity, n_out, n_pairs, stream,
                      stats, ms, SRC_TUPLES);
}

// The group joins on key columns: the columns' alignment rule (the value column's as the key
// columns': its loads have the keys' shape), a value for every S key, and R rows that fit the int32
// row index. Checked before any device call; join_group then checks the rest (|S| < 2^32 among it).
static int keys_group_ok(const int32_t* d_Rkeys, uint64_t nR, const int32_t* d_Skeys, const int32_t* d_Svals,
                         uint64_t nS) {
    if (!keys_aligned(d_Rkeys, nR, d_Skeys, nS)) return 2;
    if (nS && !d_Svals) {
        set_last_error("d_Svals must hold a value for each of the nS keys of S");
        return 2;
    }
    if (nS && ((uintptr_t) d_Svals & 15u)) {
        set_last_error("value column S is not 16-byte aligned (shard a column at multiples of 4 values)");
        return 2;
    }
    if (nR >= (1ull << 31)) {
        set_last_error("key column R has 2^31 rows or more (row indices are int32)");
        return 3;
    }
    return 0;
}

int hwbrj_join_keys_group_device(const int32_t* d_Rkeys, uint64_t nR, const int32_t* d_Skeys,
                                 const int32_t* d_Svals, uint64_t nS, const bloom_filter_args_t* args, int kind,
                                 hwbrj_group_row_t* d_out, uint64_t capacity, uint64_t* n_out, uint64_t* n_pairs,
                                 void* stream, hwbrj_stats_t* stats, double* ms) {
    if (const int rc = keys_group_ok(d_Rkeys, nR, d_Skeys, d_Svals, nS)) return rc;
    return join_group(d_Rkeys, nR, d_Skeys, d_Svals, nS, args, kind, GRP_COUNT_SUM, d_out, capacity, n_out, n_pairs,
                      stream, stats, ms, SRC_KEYS);
}

int hwbrj_join_keys_group_minmax_device(const int32_t* d_Rkeys, uint64_t nR, const int32_t* d_Skeys,
                                        const int32_t* d_Svals, uint64_t nS, const bloom_filter_args_t* args,
                                        int kind, hwbrj_group_minmax_row_t* d_out, uint64_t capacity,
                                        uint64_t* n_out, uint64_t* n_pairs, void* stream, hwbrj_stats_t* stats,
                                        double* ms) {
    if (const int rc = keys_group_ok(d_Rkeys, nR, d_Skeys, d_Svals, nS)) return rc;
    return join_group(d_Rkeys, nR, d_Skeys, d_Svals, nS, args, kind, GRP_COUNT_MINMAX, d_out, capacity, n_out, n_pairs,
                      stream, stats, ms, SRC_KEYS);
}

// The group joins on key columns with validity bitmaps: the counterpart's rules, then the bitmaps'
// (masks_ok), then join_group's; all three bitmaps NULL: the counterpart's call.
static int join_keys_group_nulls(const int32_t* d_Rkeys, const uint8_t* d_Rvalid, uint64_t nR, const int32_t* d_Skeys,
                                 const uint8_t* d_Svalid, const int32_t* d_Svals, const uint8_t* d_Svals_valid,
                                 uint64_t nS, const bloom_filter_args_t* args, int kind, uint32_t agg, void* d_out,
                                 uint64_t capacity, uint64_t* n_out, uint64_t* n_pairs, void* stream,
                                 hwbrj_stats_t* stats, double* ms) {
    if (const int rc = keys_group_ok(d_Rkeys, nR, d_Skeys, d_Svals, nS)) return rc;
    if (const int rc = masks_ok(d_Rvalid, nR, d_Svalid, nS, args, true, d_Svals_valid)) return rc;
    return join_group(d_Rkeys, nR, d_Skeys, d_Svals, nS, args, kind, agg, d_out, capacity, n_out, n_pairs, stream,
                      stats, ms, SRC_KEYS, KeyMasks{d_Rvalid, d_Svalid, d_Svals_valid});
}

int hwbrj_join_keys_group_nulls_device(const int32_t* d_Rkeys, const uint8_t* d_Rvalid, uint64_t nR,
                                       const int32_t* d_Skeys, const uint8_t* d_Svalid, const int32_t* d_Svals,
                                       const uint8_t* d_Svals_valid, uint64_t nS, const bloom_filter_args_t* args,
                                       int kind, hwbrj_group_row_t* d_out, uint64_t capacity, uint64_t* n_out,
                                       uint64_t* n_pairs, void* stream, hwbrj_stats_t* stats, double* ms) {
    return join_keys_group_nulls(d_Rkeys, d_Rvalid, nR, d_Skeys, d_Svalid, d_Svals, d_Svals_valid, nS, args, kind,
                                 GRP_COUNT_SUM, d_out, capacity, n_out, n_pairs, stream, stats, ms);
}

int hwbrj_join_keys_group_minmax_nulls_device(const int32_t* d_Rkeys, const uint8_t* d_Rvalid, uint64_t nR,
                                              const int32_t* d_Skeys, const uint8_t* d_Svalid, const int32_t* d_Svals,
                                              const uint8_t* d_Svals_valid, uint64_t nS,
                                              const bloom_filter_args_t* args, int kind,
                                              hwbrj_group_minmax_row_t* d_out, uint64_t capacity, uint64_t* n_out,
                                              uint64_t* n_pairs, void* stream, hwbrj_stats_t* stats, double* ms) {
    return join_keys_group_nulls(d_Rkeys, d_Rvalid, nR, d_Skeys, d_Svalid, d_Svals, d_Svals_valid, nS, args, kind,
                                 GRP_COUNT_MINMAX, d_out, capacity, n_out, n_pairs, stream, stats, ms);
}

// ---- prepared builds (include/hwbrj.h "Prepared builds") ----
int hwbrj_build_keys_device(const int32_t* d_Rkeys, const uint8_t* d_Rvalid, uint64_t nR,
                            const bloom_filter_args_t* args, int purpose, void* stream, hwbrj_build_t** build,
                            double* ms) {
    // (all of these before any device call; *build is written on success only)
    if (purpose != HWBRJ_BUILD_COUNT && purpose != HWBRJ_BUILD_ROWS) {
        set_last_error("unknown build purpose (HWBRJ_BUILD_COUNT, HWBRJ_BUILD_ROWS)");
        return 2;
    }
    if (!build) {
        set_last_error("build must point to where the build's handle goes");
        return 2;
    }
    const bool rows = purpose == HWBRJ_BUILD_ROWS;
    if (!keys_aligned(d_Rkeys, nR, nullptr, 0)) return 2;
    if (d_Rvalid && nR && ((uintptr_t) d_Rvalid & 3u)) {
        set_last_error("validity bitmap of R is not 4-byte aligned (shard a masked column at multiples of 32 rows)");
        return 2;
    }
    if (rows && nR >= (1ull << 31)) {
        set_last_error("key column R has 2^31 rows or more (row indices are int32)");
        return 3;
    }
    Geometry    g;
    std::string err;
    if (!plan_geometry(args, nR, &g, &err, rows)) {
        set_last_error(err);
        return 2;
    }
    if (!masks_supported(g)) {
        set_last_error("a prepared build needs partition slices (blocked/sectorized, basic k = 1, or no filter)");
        return kRcMaskFilter;
    }
    Engine* e = engine_for_current_device();
    if (!e) return 10;
    hwbrj_build_t* b = new hwbrj_build_t();
    b->rows          = rows;
    const int rc     = e->build(d_Rkeys, d_Rvalid, nR, args, (hipStream_t) stream, b, ms);
    if (rc) {
        b->release();
        delete b;
        return rc;
    }
    *build = b;
    return 0;
}

// The current device's Engine when it is the build's, else why not
static Engine* build_engine(const Build* b, int* rc) {
    Engine* e = engine_for_current_device();
    *rc       = !e ? 10 : build_device_ok(b, e);
    return *rc ? nullptr : e;
}

int hwbrj_build_free(hwbrj_build_t* b) {
    if (!b) return 0;
    int rc = 0;
    if (!build_engine(b, &rc)) return rc;
    b->release();
    delete b;
    return 0;
}

int hwbrj_build_info(const hwbrj_build_t* b, uint64_t* out, int n) {
    if (!b) {
        set_last_error("build is NULL");
        return 2;
    }
    if (!out || n < HWBRJ_BI_COUNT) {
        set_last_error("out must hold HWBRJ_BI_COUNT words");
        return 7;
    }
    for (int i = 0; i < n; i++) out[i] = 0;
    out[HWBRJ_BI_NR]       = b->r.nR;
    out[HWBRJ_BI_PURPOSE]  = b->rows ? HWBRJ_BUILD_ROWS : HWBRJ_BUILD_COUNT;
    out[HWBRJ_BI_MODE]     = (uint64_t) b->r.g.mode;
    out[HWBRJ_BI_F]        = b->r.s.F;
    out[HWBRJ_BI_NSUB]     = b->r.s.NSUB;
    out[HWBRJ_BI_KEY_BITS] = b->r.kbits ? b->r.kbits : 32u;
    out[HWBRJ_BI_DEVICE]   = (uint64_t) b->device;
    out[HWBRJ_BI_BYTES]    = b->bytes();
    out[HWBRJ_BI_MASKED]   = b->r.r_masked ? 1u : 0u;
    return 0;
}

int hwbrj_build_export_filter(const hwbrj_build_t* b, uint8_t* host_out, uint64_t nbytes) {
    if (!b) {
        set_last_error("build is NULL");
        return 2;
    }
    int     rc = 0;
    Engine* e  = build_engine(b, &rc);
    return e ? e->export_build_filter(*b, host_out, nbytes) : rc;
}

// The build's filter applied to a key column (include/hwbrj.h): every refusal before any device call,
// in the header's order, with nothing written.
int hwbrj_build_filter_keys_device(const hwbrj_build_t* b, const int32_t* d_Skeys, const uint8_t* d_Svalid, uint64_t nS,
                                   uint8_t* d_out, uint64_t* n_pass, void* stream, double* ms) {
    if (!b) {
        set_last_error("build is NULL");
        return 2;
    }
    if (!b->has_args) {
        set_last_error("no filter has been built");
        return 5;
    }
    if (!keys_aligned(nullptr, 0, d_Skeys, nS)) return 2;
    if (d_Svalid && nS && ((uintptr_t) d_Svalid & 3u)) {
        set_last_error("validity bitmap of S is not 4-byte aligned (shard a masked column at multiples of 32 rows)");
        return 2;
    }
    if (nS && ((uintptr_t) d_out & 3u)) {
        set_last_error("d_out is not 4-byte aligned (the bitmap is written as dwords)");
        return 2;
    }
    if (nS && !d_out) {
        set_last_error("d_out must hold 4 * ceil(nS / 32) bytes");
        return 2;
    }
    if (nS >= (1ull << 32)) {
        set_last_error("nS must be below 2^32");
        return 3;
    }
    int     rc = 0;
    Engine* e  = build_engine(b, &rc);
    if (!e) return rc;
    if (nS == 0) {
        if (n_pass) *n_pass = 0;
        if (ms) *ms = 0;
        return 0;
    }
    return e->filter_keys(*b, d_Skeys, d_Svalid, nS, d_out, n_pass, (hipStream_t) stream, ms);
}

// What every probe checks first, before any device call: the build and its purpose
static int probe_build_ok(const hwbrj_build_t* b, bool rows) {
    if (!b) {
        set_last_error("build is NULL");
        return 2;
    }
    if (b->rows != rows) {
        set_last_error(rows ? "this probe needs a HWBRJ_BUILD_ROWS build" : "the counting probe needs a HWBRJ_BUILD_COUNT build");
        return 2;
    }
    return 0;
}
// the build's filter, and the bitmaps of a probe: R's is the build's own copy
static const bloom_filter_args_t* build_args(const Build* b) { return b->has_args ? &b->args : nullptr; }
static KeyMasks probe_masks(const Build* b, const uint8_t* d_Svalid, const uint8_t* d_Svv = nullptr) {
    return KeyMasks{b->r.rvalid.as<uint8_t>(), d_Svalid, d_Svv};
}

int hwbrj_probe_keys_device(const hwbrj_build_t* b, const int32_t* d_Skeys, const uint8_t* d_Svalid, uint64_t nS,
                            int algorithm, void* stream, hwbrj_stats_t* stats) {
    if (const int rc = probe_build_ok(b, false)) return rc;
    if (!keys_aligned(nullptr, 0, d_Skeys, nS)) return 2;
    if (const int rc = masks_ok(nullptr, b->r.nR, d_Svalid, nS, build_args(b), false)) return rc;
    int     rc = 0;
    Engine* e  = build_engine(b, &rc);
    if (!e) return rc;
    // (a counting build keeps no copy of R's bitmap: nothing after the R scatter reads it)
    return e->run(JoinIn{nullptr, b->r.nR, d_Skeys, nS, build_args(b), (hipStream_t) stream},
                  count_req(algorithm, SRC_KEYS, KeyMasks{nullptr, d_Svalid}), stats, nullptr, b);
}

int hwbrj_probe_keys_pairs_device(hwbrj_build_t* b, const int32_t* d_Skeys, const uint8_t* d_Svalid, uint64_t nS,
                                  tuple_t* d_out, uint64_t capacity, uint64_t* n_out, void* stream,
                                  hwbrj_stats_t* stats, double* ms) {
    if (const int rc = probe_build_ok(b, true)) return rc;
    if (const int rc = keys_rows_ok(nullptr, b->r.nR, d_Skeys, nS)) return rc;
    if (const int rc = masks_ok(nullptr, b->r.nR, d_Svalid, nS, build_args(b), true)) return rc;
    if (capacity > 0 && !d_out) {
        set_last_error("d_out must hold capacity rows");
        return 2;
    }
    return join_pairs(nullptr, b->r.nR, d_Skeys, nS, build_args(b), d_out, capacity, n_out, stream, stats, ms, SRC_KEYS,
                      probe_masks(b, d_Svalid), b);
}

int hwbrj_probe_keys_semi_device(hwbrj_build_t* b, const int32_t* d_Skeys, const uint8_t* d_Svalid, uint64_t nS,
                                 int kind, tuple_t* d_out, uint64_t capacity, uint64_t* n_out, void* stream,
                                 hwbrj_stats_t* stats, double* ms) {
    if (const int rc = probe_build_ok(b, true)) return rc;
    if (const int rc = keys_rows_ok(nullptr, b->r.nR, d_Skeys, nS)) return rc;
    if (const int rc = masks_ok(nullptr, b->r.nR, d_Svalid, nS, build_args(b), true)) return rc;
    return join_semi(nullptr, b->r.nR, d_Skeys, nS, build_args(b), kind, d_out, capacity, n_out, stream, stats, ms,
                     SRC_KEYS, probe_masks(b, d_Svalid), b);
}

int hwbrj_probe_keys_outer_device(hwbrj_build_t* b, const int32_t* d_Skeys, const uint8_t* d_Svalid, uint64_t nS,
                                  int kind, tuple_t* d_out, uint64_t capacity, uint64_t* n_out, uint64_t* n_class,
                                  void* stream, hwbrj_stats_t* stats, double* ms) {
    if (const int rc = probe_build_ok(b, true)) return rc;
    if (const int rc = keys_rows_ok(nullptr, b->r.nR, d_Skeys, nS)) return rc;
    if (const int rc = masks_ok(nullptr, b->r.nR, d_Svalid, nS, build_args(b), true)) return rc;
    return join_outer(nullptr, b->r.nR, d_Skeys, nS, build_args(b), kind, -1, d_out, capacity, n_out, n_class, stream,
                      stats, ms, SRC_KEYS, probe_masks(b, d_Svalid), b);
}

static int probe_keys_group(hwbrj_build_t* b, const int32_t* d_Skeys, const uint8_t* d_Svalid, const int32_t* d_Svals,
                            const uint8_t* d_Svals_valid, uint64_t nS, int kind, uint32_t agg, void* d_out,
                            uint64_t capacity, uint64_t* n_out, uint64_t* n_pairs, void* stream, hwbrj_stats_t* stats,
                            double* ms) {
    if (const int rc = probe_build_ok(b, true)) return rc;
    if (const int rc = keys_group_ok(nullptr, b->r.nR, d_Skeys, d_Svals, nS)) return rc;
    if (const int rc = masks_ok(nullptr, b->r.nR, d_Svalid, nS, build_args(b), true, d_Svals_valid)) return rc;
    return join_group(nullptr, b->r.nR, d_Skeys, d_Svals, nS, build_args(b), kind, agg, d_out, capacity, n_out, n_pairs,
                      stream, stats, ms, SRC_KEYS, probe_masks(b, d_Svalid, d_Svals_valid), b);
}

int hwbrj_probe_keys_group_device(hwbrj_build_t* b, const int32_t* d_Skeys, const uint8_t* d_Svalid,
                                  const int32_t* d_Svals, const uint8_t* d_Svals_valid, uint64_t nS, int kind,
                                  hwbrj_group_row_t* d_out, uint64_t capacity, uint64_t* n_out, uint64_t* n_pairs,
                                  void* stream, hwbrj_stats_t* stats, double* ms) {
    return probe_keys_group(b, d_Skeys, d_Svalid, d_Svals, d_Svals_valid, nS, kind, GRP_COUNT_SUM, d_out, capacity, n_out,
                            n_pairs, stream, stats, ms);
}

int hwbrj_probe_keys_group_minmax_device(hwbrj_build_t* b, const int32_t* d_Skeys, const uint8_t* d_Svalid,
                                         const int32_t* d_Svals, const uint8_t* d_Svals_valid, uint64_t nS, int kind,
                                         hwbrj_group_minmax_row_t* d_out, uint64_t capacity, uint64_t* n_out,
                                         uint64_t* n_pairs, void* stream, hwbrj_stats_t* stats, double* ms) {
    return probe_keys_group(b, d_Skeys, d_Svalid, d_Svals, d_Svals_valid, nS, kind, GRP_COUNT_MINMAX, d_out, capacity,
                            n_out, n_pairs, stream, stats, ms);
}

int hwbrj_build_unmatched_device(hwbrj_build_t* b, tuple_t* d_out, uint64_t capacity, uint64_t* n_out, void* stream,
                                 double* ms) {
    if (const int rc = probe_build_ok(b, true)) return rc;
    if (capacity > 0 && !d_out) {
        set_last_error("d_out must hold capacity rows");
        return 2;
    }
    int     rc = 0;
    Engine* e  = build_engine(b, &rc);
    if (!e) return rc;
    uint64_t n = 0;
    if ((rc = e->unmatched(b, (uint2*) d_out, capacity, &n, (hipStream_t) stream, ms))) return rc;
    if (n_out) *n_out = n;
    if (n > capacity) {
        set_last_error("output capacity below the row count (*n_out holds the count)");
        return 7;
    }
    return 0;
}

int hwbrj_build_reset_marks(hwbrj_build_t* b) {
    if (const int rc = probe_build_ok(b, true)) return rc;
    int rc = 0;
    if (!build_engine(b, &rc)) return rc;
    if (hipMemset(b->marks.p, 0, b->marks.bytes) != hipSuccess) {
        set_last_error("clearing the marks failed");
        return 1;
    }
    return 0;
}

// ---- group accumulators kept across batches (include/hwbrj.h, "group accumulators") ----
static_assert(HWBRJ_AGG_SUM == (int) GRP_COUNT_SUM && HWBRJ_AGG_MINMAX == (int) GRP_COUNT_MINMAX, "agg is GroupAgg");
static int agg_ok(int agg) {
    if (agg == HWBRJ_AGG_SUM || agg == HWBRJ_AGG_MINMAX) return 0;
    set_last_error("unknown aggregate form (HWBRJ_AGG_SUM, HWBRJ_AGG_MINMAX)");
    return 2;
}

// hwbrj_probe_keys_group_device's checks in its order, then the form's running total; the join is
// that probe's under HWBRJ_GROUP_MATCHED with the build's accumulators in place of an output.
int hwbrj_probe_keys_group_accum_device(hwbrj_build_t* b, const int32_t* d_Skeys, const uint8_t* d_Svalid,
                                        const int32_t* d_Svals, const uint8_t* d_Svals_valid, uint64_t nS, int agg,
                                        uint64_t* n_rows, uint64_t* n_pairs, void* stream, hwbrj_stats_t* stats,
                                        double* ms) {
    if (const int rc = probe_build_ok(b, true)) return rc;
    if (const int rc = keys_group_ok(nullptr, b->r.nR, d_Skeys, d_Svals, nS)) return rc;
    if (const int rc = masks_ok(nullptr, b->r.nR, d_Svalid, nS, build_args(b), true, d_Svals_valid)) return rc;
    if (const int rc = agg_ok(agg)) return rc;
    if (nS >= (1ull << 32)) {
        set_last_error("group join: |S| must be below 2^32 rows (32-bit counts)");
        return 3;
    }
    if (b->gacc_ns[agg] + nS >= (1ull << 32)) {  // (all before any device call)
        set_last_error("group accumulators: " + std::to_string(b->gacc_ns[agg]) + " S rows accumulated since the last reset, and " +
                       std::to_string(nS) + " more would reach 2^32 (32-bit counts, exact 64-bit sums); read the rows and reset");
        return 3;
    }
    int     rc = 0;
    Engine* e  = build_engine(b, &rc);
    if (!e) return rc;
    if (!b->gacc[agg].p && (rc = e->group_acc_reset(b, (uint32_t) agg))) return rc;
    JoinReq req = payload_req(JOIN_GROUP, nullptr, 0, SRC_KEYS, probe_masks(b, d_Svalid, d_Svals_valid));
    req.agg     = (uint32_t) agg;
    req.s_val   = d_Svals;
    req.gacc    = b->gacc[agg].as<uint4>();
    hwbrj_stats_t st;
    uint64_t      n = 0;
    JoinExtras    x;
    if ((rc = pipeline_or_side_pass(e, JoinIn{nullptr, b->r.nR, d_Skeys, nS, build_args(b), (hipStream_t) stream}, req, &st,
                                    &n, &x, ms, b)))
        return rc;
    b->gacc_ns[agg] += nS;
    if (n_rows) *n_rows = n;
    if (n_pairs) *n_pairs = x.pairs;
    if (stats) *stats = st;
    return 0;
}

int hwbrj_build_group_rows_device(hwbrj_build_t* b, int agg, int kind, void* d_out, uint64_t capacity, uint64_t* n_out,
                                  uint64_t* n_pairs, void* stream, double* ms) {
    if (const int rc = probe_build_ok(b, true)) return rc;
    if (const int rc = agg_ok(agg)) return rc;
    if (kind != HWBRJ_GROUP_MATCHED && kind != HWBRJ_GROUP_ALL) {
        set_last_error("unknown group join kind (HWBRJ_GROUP_MATCHED, HWBRJ_GROUP_ALL)");
        return 2;
    }
    if (capacity > 0 && !d_out) {
        set_last_error("d_out must hold capacity rows");
        return 2;
    }
    if (((uintptr_t) d_out & 15u) != 0) {
        set_last_error("d_out must be 16-byte aligned (a row is written as one 16-byte store)");
        return 2;
    }
    int     rc = 0;
    Engine* e  = build_engine(b, &rc);
    if (!e) return rc;
    uint64_t n = 0, pairs = 0;
    if ((rc = e->group_rows(b, (uint32_t) agg, kind == HWBRJ_GROUP_ALL, (uint4*) d_out, capacity, &n, &pairs,
                            (hipStream_t) stream, ms)))
        return rc;
    if (n_out) *n_out = n;
    if (n_pairs) *n_pairs = pairs;
    if (n > capacity) {
        set_last_error("output capacity below the row count (*n_out holds the count)");
        return 7;
    }
    return 0;
}

int hwbrj_build_group_reset(hwbrj_build_t* b, int agg) {
    if (const int rc = probe_build_ok(b, true)) return rc;
    if (const int rc = agg_ok(agg)) return rc;
    int     rc = 0;
    Engine* e  = build_engine(b, &rc);
    return e ? e->group_acc_reset(b, (uint32_t) agg) : rc;
}

static int g_materialize = -1;  // -1: from HWBRJ_MATERIALIZE
static int g_gpus        = 0;   // shards of a host BPRO/PRO (0: from HWBRJ_GPUS, default 1)
void hwbrj_set_materialize(int on) { g_materialize = on ? 1 : 0; }

int hwbrj_set_gpus(int g) {
    if (g < 0 || g > 4096) {
        set_last_error("gpus must be in [0, 4096]");
        return 2;
    }
    g_gpus = g;
    return 0;
}

int hwbrj_generate_device(tuple_t* d_out, uint64_t n, uint32_t nthreads, uint64_t maxid,
                          uint64_t threshold, double selectivity, uint64_t seed, void* stream) {
    Engine* e = engine_for_current_device();
    if (!e) return 10;  // (last error set by engine_for_current_device)
    return e->generate((uint2*) d_out, n, 0, n, nthreads, maxid, threshold, selectivity, seed,
                       (hipStream_t) stream);
}

int hwbrj_generate_device_range(tuple_t* d_out, uint64_t n, uint64_t offset, uint64_t count,
                                uint32_t nthreads, uint64_t maxid, uint64_t threshold,
                                double selectivity, uint64_t seed, void* stream) {
    Engine* e = engine_for_current_device();
    if (!e) return 10;  // (last error set by engine_for_current_device)
    return e->generate((uint2*) d_out, n, offset, count, nthreads, maxid, threshold, selectivity,
                       seed, (hipStream_t) stream);
}

int hwbrj_generate_host(tuple_t* out, uint64_t n, uint32_t nthreads, uint64_t maxid,
                        uint64_t threshold, double selectivity, uint64_t seed, int host_threads) {
    std::vector<GenPlan> plan(1);
    if (make_gen_plan(&plan[0], n, nthreads, maxid, threshold, selectivity)) {
        set_last_error("invalid generator parameters");
        return 2;
    }
    const Perm perm = make_perm(n, seed);
    int        T    = host_threads > 0 ? host_threads : (int) std::thread::hardware_concurrency();
    if (T < 1) T = 1;
    if ((uint64_t) T > n / 4096 + 1) T = (int) (n / 4096 + 1);
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) {
        th.emplace_back([&, t] {
            const uint64_t b = n * t / T, e = n * (t + 1) / T;
            for (uint64_t i = b; i < e; i++) {
                out[i].key     = gen_key_at(plan[0], perm_apply(perm, i));
                out[i].payload = (int32_t) i;
            }
        });
    }
    for (auto& x : th) x.join();
    return 0;
}

int hwbrj_export_filter(uint8_t* host_out, uint64_t nbytes) {
    Engine* e = engine_for_current_device();
    if (!e) return 10;  // (last error set by engine_for_current_device)
    return e->export_filter(host_out, nbytes);
}

int hwbrj_tables_info(uint64_t* out, int n) {
    Engine* e = engine_for_current_device();
    if (!e) return 10;  // (last error set by engine_for_current_device)
    return e->tables_info(out, n);
}

int hwbrj_tables_read(int which, void* host_out, uint64_t cap_bytes, uint64_t* bytes) {
    Engine* e = engine_for_current_device();
    if (!e) return 10;  // (last error set by engine_for_current_device)
    return e->tables_read(which, host_out, cap_bytes, bytes);
}

// src/bloom_filter.c:25-34 -- prints the reference's message and exits(1).
void assert_args(bloom_filter_args_t* args) {
    if ((args->m & (args->m - 1)) != 0) {
        printf("m must be a power of 2");
        exit(1);
    }
    if (args->variant != BASIC) {
        const uint64_t B = args->B;
        if (B == 0 || (B & (B - 1)) != 0) {
            printf("B must be a power 2");
            exit(1);
        }
        if (args->m % B != 0) {
            printf("m must be a multiple of B");
            exit(1);
        }
    }
}

}  // extern "C"

// ------------------------------------------------------------------ BPRO / PRO (host data)
static void fatal(const char* what) {
    printf("[ERROR] %s: %s\n", what, hwbrj_last_error());
    exit(EXIT_FAILURE);  // the reference's convention (src/parallel_radix_join_bloom.c:64-71)
}

// src/parallel_radix_join_bloom.c:1509-1547 print_timing, fed with device times.
static void print_timing(uint64_t total_cyc, uint64_t build_cyc, uint64_t part_cyc,
                         uint64_t numtuples, int64_t result, double total_usec,
                         double part_usec, double probe_usec, double join_usec) {
    const double nsec_per_tuple = total_usec * 1000.0 / (double) (numtuples ? numtuples : 1);
    fprintf(stdout, "RUNTIME TOTAL, BUILD, PART (cycles): \n");
    fprintf(stdout, "%llu \t %llu \t %llu ", (unsigned long long) total_cyc,
            (unsigned long long) build_cyc, (unsigned long long) part_cyc);
    fprintf(stdout, "\n");
    fprintf(stdout, "TOTAL-TIME-USECS, TOTAL-TUPLES, NSEC-PER-TUPLE: \n");
    fprintf(stdout, "%.4lf \t %llu \t ", total_usec, (unsigned long long) result);
    fprintf(stdout, "%.4lf ", nsec_per_tuple);
    fprintf(stdout, "\n");
    fprintf(stdout, "PARTITION-TIME-USECS, PROBE-TIME-USECS, JOIN-TIME-USECS: \n");
    fprintf(stdout, "%.4lf \t %.4lf\t %.4lf \n", part_usec, probe_usec, join_usec);
    fflush(stdout);
}

// src/tuple_buffer.h:27-126: the reference's chained result buffers. The newest buffer is the
// head (cb->buf, `writepos` tuples); older, full buffers of CHAINEDBUFF_NUMTUPLESPERBUF follow
// through `next`, so cb_begin / cb_read_next walk every pair.
namespace {
constexpr uint32_t kCbTuples = 1024 * 1024;  // CHAINEDBUFF_NUMTUPLESPERBUF
struct TupleBuffer {
    tuple_t*     tuples;
    TupleBuffer* next;
};
struct ChainedTupleBuffer {
    TupleBuffer* buf;
    TupleBuffer* readcursor;
    TupleBuffer* writecursor;
    uint32_t     writepos, readpos, readlen, numbufs;
};

ChainedTupleBuffer* chained_from(const tuple_t* pairs, uint64_t n) {
    ChainedTupleBuffer* cb   = (ChainedTupleBuffer*) calloc(1, sizeof(ChainedTupleBuffer));
    TupleBuffer*        head = nullptr;
    uint64_t            off  = 0;
    do {
        const uint64_t c = n - off < kCbTuples ? n - off : kCbTuples;
        TupleBuffer*   b = (TupleBuffer*) malloc(sizeof(TupleBuffer));
        if (posix_memalign((void**) &b->tuples, 64, sizeof(tuple_t) * kCbTuples)) b->tuples = nullptr;
        if (!b->tuples) {
            set_last_error("out of host memory (result buffers)");
            return nullptr;
        }
        if (c) memcpy(b->tuples, pairs + off, c * sizeof(tuple_t));
        b->next      = head;
        head         = b;
        cb->writepos = (uint32_t) c;
        cb->numbufs++;
        off += c;
    } while (off < n);
    cb->buf = cb->readcursor = cb->writecursor = head;
    return cb;
}
}  // namespace

// JOIN_RESULT_MATERIALIZE (src/parallel_radix_join_bloom.c:1450-1472): resultlist[t] of every
// worker; here all pairs are thread 0's, the others hold empty buffers.
static threadresult_t* materialize_to_host(const tuple_t* dR, uint64_t nR, const tuple_t* dS,
                                           uint64_t nS, const bloom_filter_args_t* args,
                                           uint64_t matches, int nthreads) {
    tuple_t* dout = nullptr;
    if (hipMalloc((void**) &dout, (matches ? matches : 1) * sizeof(tuple_t)) != hipSuccess) {
        set_last_error("hipMalloc of the result pairs failed");
        fatal("BPRO");
    }
    Engine*       e = engine_for_current_device();
    uint64_t      n = 0;
    hwbrj_stats_t st;
    if (!e || pipeline_or_side_pass(e, JoinIn{dR, nR, dS, nS, args, nullptr},
                                    payload_req(JOIN_PAIRS, dout, matches, SRC_TUPLES, KeyMasks{}), &st, &n, nullptr,
                                    nullptr) != 0 ||
        n != matches)
        fatal("BPRO (materialize)");
    std::vector<tuple_t> host(matches ? matches : 1);
    if (matches && hipMemcpy(host.data(), dout, matches * sizeof(tuple_t), hipMemcpyDeviceToHost) != hipSuccess) {
        set_last_error("D2H of the result pairs failed");
        fatal("BPRO");
    }
    (void) hipFree(dout);
    const int       T    = nthreads > 0 ? nthreads : 1;
    threadresult_t* tres = (threadresult_t*) calloc(T, sizeof(threadresult_t));
    for (int t = 0; t < T; t++) {
        tres[t].threadid = (uint32_t) t;
        tres[t].nresults = t == 0 ? (int64_t) matches : 0;
        tres[t].results  = chained_from(host.data(), t == 0 ? matches : 0);
        if (!tres[t].results) fatal("BPRO");
    }
    return tres;
}

static int host_shards() {
    if (g_gpus > 0) return g_gpus;
    const char* e = getenv("HWBRJ_GPUS");
    const int   v = e ? atoi(e) : 1;
    return v > 0 ? v : 1;
}

// One shard of a host join: R replicated, S rows [s0, s1) (the reference's per-thread chunking of
// S, src/parallel_radix_join_bloom.c:1646-1670, with a GPU per chunk).
struct Shard {
    uint64_t      s0 = 0, s1 = 0;
    hwbrj_stats_t st{};
    double        h2d_usec = 0;
    tuple_t*      dS = nullptr;  // this shard's S rows in HBM (staged before the timed region)
};

// The device copies of one device's shards (first, first + step, ...): R once, every shard's S.
struct DeviceStage {
    int      dev = 0;
    tuple_t* dR  = nullptr;
};

static void free_stage(DeviceStage& ds, std::vector<Shard>& shards, int first, int step) {
    (void) hipSetDevice(ds.dev);
    (void) hipFree(ds.dR);
    ds.dR = nullptr;
    for (size_t g = first; g < shards.size(); g += step) {
        (void) hipFree(shards[g].dS);
        shards[g].dS = nullptr;
    }
}

// Everything the reference does before its timer starts (src/parallel_radix_join_bloom.c:1560-1640:
// allocations, the zeroed bitmap and tmp buffers): device allocations, the H2D copies of R and of
// every shard's S rows, and the join's scratch (Engine::reserve). Returns 0 or an error code.
static int stage_device_shards(DeviceStage& ds, int first, int step, const relation_t* relR,
                               const relation_t* relS, const bloom_filter_args_t* args,
                               std::vector<Shard>& shards, int algo) {
    if (hipSetDevice(ds.dev) != hipSuccess) {
        set_last_error("hipSetDevice failed");
        return 11;
    }
    const uint64_t nR = relR->num_tuples;
    if (hipMalloc((void**) &ds.dR, (nR ? nR : 1) * sizeof(tuple_t)) != hipSuccess) {
        set_last_error("hipMalloc of the input relations failed");
        return 12;
    }
    const auto h0 = std::chrono::steady_clock::now();
    if (nR && hipMemcpy(ds.dR, relR->tuples, nR * sizeof(tuple_t), hipMemcpyHostToDevice) != hipSuccess) {
        set_last_error("H2D copy failed");
        return 13;
    }
    double h2d_r = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h0).count();
    for (size_t g = first; g < shards.size(); g += step) {
        Shard&         sh = shards[g];
        const uint64_t n  = sh.s1 - sh.s0;
        if (hipMalloc((void**) &sh.dS, (n ? n : 1) * sizeof(tuple_t)) != hipSuccess) {
            set_last_error("hipMalloc of the input relations failed");
            return 12;
        }
        const auto h1 = std::chrono::steady_clock::now();
        if (n && hipMemcpy(sh.dS, relS->tuples + sh.s0, n * sizeof(tuple_t), hipMemcpyHostToDevice) != hipSuccess) {
            set_last_error("H2D copy failed");
            return 13;
        }
        sh.h2d_usec = h2d_r + std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h1).count();
        h2d_r       = 0;
    }
    Engine* e = engine_for_current_device();
    if (!e) return 10;
    for (size_t g = first; g < shards.size(); g += step) {  // grow-only: the largest shard decides
        const int rc = e->reserve((const uint2*) ds.dR, nR, (const uint2*) shards[g].dS,
                                  shards[g].s1 - shards[g].s0, args, algo);
        if (rc) return rc;
    }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 14;
}

// The timed part: the device's shards joined one after the other on its Engine.
static int join_device_shards(const DeviceStage& ds, int first, int step, uint64_t nR,
                              const bloom_filter_args_t* args, std::vector<Shard>& shards, int algo) {
    if (hipSetDevice(ds.dev) != hipSuccess) {
        set_last_error("hipSetDevice failed");
        return 11;
    }
    for (size_t g = first; g < shards.size(); g += step) {
        Shard&    sh = shards[g];
        const int rc = hwbrj_join_device_algo(ds.dR, nR, sh.dS, sh.s1 - sh.s0, args, algo, nullptr, &sh.st);
        if (rc) return rc;
    }
    return 0;
}

// algo: the per-partition join (HWBRJ_ALGO_PRO / PRH / PRHO, the reference's join_init_run
// JoinFunction: bucket_chaining_join / histogram_join / histogram_optimized_join)
static result_t* run_host_join(relation_t* relR, relation_t* relS, int nthreads,
                               bloom_filter_args_t* args, bool print_filtered = true, int algo = 0) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        set_last_error("no MI355X device visible");
        fatal("BPRO");
    }
    int cur = 0;
    (void) hipGetDevice(&cur);
    const uint64_t nR = relR->num_tuples, nS = relS->num_tuples;
    // G shards of S over the visible devices (shard g on device g mod ndev; G > ndev runs several
    // shards per device one after the other, e.g. to rehearse G = 8 on one GPU)
    const int          G    = host_shards();
    const int          nuse = std::min(G, ndev);
    std::vector<Shard> shards(G);
    for (int g = 0; g < G; g++) {
        shards[g].s0 = nS * (uint64_t) g / (uint64_t) G;
        shards[g].s1 = nS * (uint64_t) (g + 1) / (uint64_t) G;
    }
    std::vector<int> rcs(nuse, 0);
    std::vector<std::string> errs(nuse);
    std::vector<DeviceStage> stage(nuse);
    for (int d = 0; d < nuse; d++) stage[d].dev = nuse == 1 ? cur : d;
    // one host thread per device (the reference's nthreads workers, one per GPU); phase 0 stages
    // the inputs and scratch, phase 1 is the timed join
    auto each_device = [&](int phase) {
        auto work = [&](int d) {
            rcs[d] = phase == 0 ? stage_device_shards(stage[d], d, nuse, relR, relS, args, shards, algo)
                                : join_device_shards(stage[d], d, nuse, nR, args, shards, algo);
            errs[d] = hwbrj_last_error();
        };
        if (nuse == 1) {
            work(0);
        } else {
            std::vector<std::thread> th;
            for (int d = 0; d < nuse; d++) th.emplace_back(work, d);
            for (auto& t : th) t.join();
        }
        for (int d = 0; d < nuse; d++)
            if (rcs[d]) {
                for (int d2 = 0; d2 < nuse; d2++) free_stage(stage[d2], shards, d2, nuse);
                (void) hipSetDevice(cur);
                set_last_error(errs[d]);
                fatal("BPRO");
            }
    };
    each_device(0);
    // The timed region (src/parallel_radix_join_bloom.c:1107-1131 to :1477-1484): the joins only,
    // so RUNTIME TOTAL (cycles) and TOTAL-TIME-USECS cover the same work.
    const uint64_t c0 = __rdtsc();
    each_device(1);
    const uint64_t c1 = __rdtsc();
    for (int d = 0; d < nuse; d++) free_stage(stage[d], shards, d, nuse);
    (void) hipSetDevice(cur);
    // counts summed over shards; device times: the slowest device (its shards back to back)
    hwbrj_stats_t st{};
    std::vector<double> dev_ms(nuse, 0.0), dev_join(nuse, 0.0), dev_probe(nuse, 0.0);
    double h2d_usec = 0;
    for (int g = 0; g < G; g++) {
        const hwbrj_stats_t& s = shards[g].st;
        st.filtered += s.filtered;
        st.matches += s.matches;
        st.mode = s.mode, st.format = s.format, st.partitions = s.partitions;
        st.subparts = s.subparts, st.slice_segments = s.slice_segments;
        dev_ms[g % nuse] += s.ms_total;
        dev_join[g % nuse] += s.ms_join;
        dev_probe[g % nuse] += s.ms_join_probe;
        h2d_usec = std::max(h2d_usec, shards[g].h2d_usec);
        st.ms_r_scatter += s.ms_r_scatter, st.ms_r_index += s.ms_r_index, st.ms_build += s.ms_build;
        st.ms_s_scatter += s.ms_s_scatter, st.ms_s_index += s.ms_s_index, st.ms_probe += s.ms_probe;
        st.ms_surv += s.ms_surv;
    }
    const int slow = (int) (std::max_element(dev_ms.begin(), dev_ms.end()) - dev_ms.begin());
    st.ms_total      = dev_ms[slow];
    st.ms_join       = dev_join[slow];
    st.ms_join_probe = dev_probe[slow];
    // materialization (JOIN_RESULT_MATERIALIZE) runs on one device over the whole relations
    const bool mat = g_materialize == 1 || (g_materialize < 0 && getenv("HWBRJ_MATERIALIZE"));
    threadresult_t* tres = nullptr;
    if (mat) {
        tuple_t *dR = nullptr, *dS = nullptr;
        if (hipMalloc((void**) &dR, (nR ? nR : 1) * sizeof(tuple_t)) != hipSuccess ||
            hipMalloc((void**) &dS, (nS ? nS : 1) * sizeof(tuple_t)) != hipSuccess ||
            (nR && hipMemcpy(dR, relR->tuples, nR * sizeof(tuple_t), hipMemcpyHostToDevice) != hipSuccess) ||
            (nS && hipMemcpy(dS, relS->tuples, nS * sizeof(tuple_t), hipMemcpyHostToDevice) != hipSuccess)) {
            set_last_error("device copies of the relations for materialization failed");
            fatal("BPRO");
        }
        hwbrj_stats_t one;
        if (G > 1 && hwbrj_join_device_algo(dR, nR, dS, nS, args, algo, nullptr, &one) != 0) fatal("BPRO");
        tres = materialize_to_host(dR, nR, dS, nS, args, (uint64_t) st.matches, nthreads);
        (void) hipFree(dR);
        (void) hipFree(dS);
    }
    // "S-tuples after filter" is printed by BPRO/BPRH/BPRHO's thread 0 (:1253); BRJ has no such line
    if (args && print_filtered) fprintf(stdout, "S-tuples after filter: %d\n", (int) st.filtered);
    // print_timing (:1730-1742): PARTITION = start -> partitioned (both partition passes, filter
    // build and probe), JOIN = partitioned -> end, PROBE = the probe share of the join (the
    // reference's per-thread probe timers, bucket_chaining_join :289-321), cycles likewise
    const double total_cyc = (double) (c1 - c0);
    const double part_ms   = st.ms_total - st.ms_join;
    const double frac_part = st.ms_total > 0 ? part_ms / st.ms_total : 0.0;
    const double frac_prob = st.ms_total > 0 ? st.ms_join_probe / st.ms_total : 0.0;
    const uint64_t part_cyc  = (uint64_t) (total_cyc * frac_part);
    const uint64_t probe_cyc = (uint64_t) (total_cyc * frac_prob);
    print_timing((uint64_t) total_cyc, (uint64_t) total_cyc - part_cyc - probe_cyc, part_cyc, nS,
                 st.matches, st.ms_total * 1e3, part_ms * 1e3, st.ms_join_probe * 1e3, st.ms_join * 1e3);
    if (getenv("HWBRJ_VERBOSE"))
        fprintf(stderr,
                "[hwbrj] shards=%d devices=%d mode=%d format=%d F=%u NSUB=%u nseg=%u h2d_usec=%.1f | "
                "ms (summed over shards): r_scatter %.3f r_index %.3f build %.3f s_scatter %.3f "
                "s_index %.3f probe %.3f surv %.3f | join (slowest device) %.3f\n",
                G, nuse, st.mode, st.format, st.partitions, st.subparts, st.slice_segments, h2d_usec,
                st.ms_r_scatter, st.ms_r_index, st.ms_build, st.ms_s_scatter, st.ms_s_index,
                st.ms_probe, st.ms_surv, st.ms_join);
    result_t* res = (result_t*) malloc(sizeof(result_t));
    if (!res) {
        set_last_error("malloc");
        fatal("BPRO");
    }
    res->totalresults = st.matches;
    res->resultlist   = tres;
    res->nthreads     = nthreads;
    return res;
}

extern "C" {

// src/parallel_radix_join_bloom.h:34-36
result_t* BPRO(relation_t* relR, relation_t* relS, int nthreads,
               bloom_filter_args_t* bloom_filter_args) {
    return run_host_join(relR, relS, nthreads, bloom_filter_args);
}

// src/parallel_radix_join.h:33-34
result_t* PRO(relation_t* relR, relation_t* relS, int nthreads) {
    return run_host_join(relR, relS, nthreads, nullptr);
}

// The other entries of the reference's algorithm table (src/main.c:331-339). BPRH / BPRHO plug a
// different per-partition join function into the same join_init_run
// (src/parallel_radix_join_bloom.c:1789-1804): the histogram join of Kim et al. (histogram_join,
// :350-419) and its SIMD + prefetch form (histogram_optimized_join, :441-555); here k_join runs
// them (JoinParams::jkind 1 / 2) instead of its bitmap / hash table. BRJ is the single-threaded
// form of BPRO (:1806-1930) with bucket chaining: the same operator on the MI355X.
result_t* BPRH(relation_t* relR, relation_t* relS, int nthreads, bloom_filter_args_t* a) {
    return run_host_join(relR, relS, nthreads, a, true, 1);
}
result_t* BPRHO(relation_t* relR, relation_t* relS, int nthreads, bloom_filter_args_t* a) {
    return run_host_join(relR, relS, nthreads, a, true, 2);
}
result_t* BRJ(relation_t* relR, relation_t* relS, int nthreads, bloom_filter_args_t* a) {
    return run_host_join(relR, relS, nthreads, a, false);
}
result_t* PRH(relation_t* relR, relation_t* relS, int nthreads) {
    return run_host_join(relR, relS, nthreads, nullptr, true, 1);
}
result_t* PRHO(relation_t* relR, relation_t* relS, int nthreads) {
    return run_host_join(relR, relS, nthreads, nullptr, true, 2);
}
result_t* RJ(relation_t* relR, relation_t* relS, int nthreads) {
    return run_host_join(relR, relS, nthreads, nullptr);
}

result_t* hwbrj_BPRO(relation_t* relR, relation_t* relS, int nthreads,
                     bloom_filter_args_t* bloom_filter_args) {
    return run_host_join(relR, relS, nthreads, bloom_filter_args);
}

result_t* hwbrj_PRO(relation_t* relR, relation_t* relS, int nthreads) {
    return run_host_join(relR, relS, nthreads, nullptr);
}

}  // extern "C"
