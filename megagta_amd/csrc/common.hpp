// common.hpp — shared host-side plumbing of libmegagta_hip.so (context, error reporting, device buffers).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "../../include/megagta_hip.h"

namespace mgta {

void set_error(const char *fmt, ...);

struct HipError {
    int code;
};

#define MGTA_HIP_CHECK(expr)                                                                        \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            ::mgta::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            throw ::mgta::HipError{e_ == hipErrorOutOfMemory ? MGTA_ENOMEM : MGTA_EHIP};           \
        }                                                                                           \
    } while (0)

// RAII device allocation; tracks the context's running / peak byte count.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    uint64_t *live = nullptr, *peak = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; live = o.live; peak = o.peak; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void alloc(size_t n, uint64_t *live_ = nullptr, uint64_t *peak_ = nullptr) {
        release();
        if (n == 0) n = 16;
        MGTA_HIP_CHECK(hipMalloc(&p, n));
        bytes = n; live = live_; peak = peak_;
        if (live) { *live += n; if (peak && *live > *peak) *peak = *live; }
    }
    void release() {
        if (p) { (void)hipFree(p); if (live) *live -= bytes; }
        p = nullptr; bytes = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// no exception crosses the C boundary: a device error or a host allocation that fails inside is an error code like any other
template <class F> int guarded(const char *who, F &&f) {
    try { return f(); }
    catch (const HipError &e) { return e.code; }
    catch (const std::bad_alloc &) { set_error("%s: out of host memory", who); return MGTA_ENOMEM; }
    catch (const std::exception &e) { set_error("%s: %s", who, e.what()); return MGTA_EHIP; }
}

struct Timer {                   // owns its two events
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st;
    explicit Timer(hipStream_t s) : st(s) { MGTA_HIP_CHECK(hipEventCreate(&a)); MGTA_HIP_CHECK(hipEventCreate(&b)); }
    Timer(Timer &&o) noexcept : a(o.a), b(o.b), st(o.st) { o.a = o.b = nullptr; }
    ~Timer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    void start() { MGTA_HIP_CHECK(hipEventRecord(a, st)); }
    void end() { MGTA_HIP_CHECK(hipEventRecord(b, st)); }        // without waiting: ms() once the stream is past it
    float ms() const { float t = 0; MGTA_HIP_CHECK(hipEventElapsedTime(&t, a, b)); return t; }
    double stop() {   // milliseconds, synchronises; a launch the runtime rejected inside the phase (grid or LDS limits) surfaces here
        MGTA_HIP_CHECK(hipGetLastError());
        end();
        MGTA_HIP_CHECK(hipEventSynchronize(b));
        MGTA_HIP_CHECK(hipGetLastError());
        return ms();
    }
};

// slots of mgta_ctx::pool, the graph build's grow-only device buffers; between builds others may borrow its key buffers S_KEYS_A / S_KEYS_B.
// S_FUSED_HIST (sdbg_build.hip, Build::count_pass): per-workgroup counts of the first sort digit of the ranges counted ahead -- gigabytes
// at 10^8 reads, so unlike the other slots it is part of a pass's memory need, and Build::admit_pass lets it go where a pass only
// fits without it
enum Slot { S_BLOCK_COUNT, S_BLOCK_BASE, S_SCAN_TMP, S_SMALL, S_KEYS_A, S_KEYS_B, S_HIST, S_TILE_HEADS, S_TILE_BASE, S_CNT, S_BASE,
            S_FIRST, S_OUT_REC, S_OUT_LARGE, S_OUT_TIPS, S_PLAN, S_BIG, S_LSD, S_MULTI_COUNT, S_POS2ID, S_SOLID, S_MERCY, S_EDGE_COUNT, S_SIDE, S_FUSED_HIST,
            S_DIGIT_TOTALS /* keys per digit value of the global sort pass about to run: up to 1024 values */,
            S_SPLIT /* range lists of the oversized segments of a sort (sdbg_build.hip, split_oversized): part of a pass's memory need */, S_NUM };

}  // namespace mgta

namespace mgta {
struct AstarArenas {           // A* work memory kept between mgta_astar_batch calls: the chunk pool (base arenas of the search slots +
    DevBuf pool, meta;         // the region the searches grow into) and the allocator's bookkeeping
};
}  // namespace mgta

struct mgta_ctx {
    int refs = 1;                 // the handle itself + every reads / graph / hmm object created from it
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t mem_limit = 0;       // 0 = auto
    int force_full_lsd = 0;
    int lsd_skip_left = 0;       // sorts left that go straight to LSD passes in LDS (the last look found mostly long runs)
    int64_t emit_fused_passes = 0;   // passes of the current build whose emitter took the sort's info bytes (mgta_sdbg_last_emit_fused)
    int split_levels = 0;        // most split levels a sort of the current build ran on its oversized segments (mgta_build_stats::n_split_levels)
    int astar_log_b0 = 0;        // base arena of a search slot = 1 << astar_log_b0 nodes (0 = default 12); searches grow beyond it in place
    uint64_t astar_pool_bytes = 0;   // device memory the searches may grow into (0 = auto)
    int search_page_limit = 0;   // pages one array of a search may hold (mgta_ctx_set_search_page_limit; 0 = kMaxPages)
    int search_share_num = 1, search_share_den = 1;   // share of the CUs a search batch of this context takes (mgta_ctx_set_search_share)
    int search_cost_rate = 0;    // shared-cache searches: a path found with c expansions becomes visible c / rate seeds later (0 = no cost term)
    uint64_t search_cost_knee = 0;   // ... up to this many expansions, and 1 / search_cost_rate2 seeds per expansion beyond (0 = one rate)
    int search_cost_rate2 = 0;
    int force_lsd_tiles = 0;     // segment-local sort: LSD passes over every digit, no finish by comparison
    uint64_t live_bytes = 0, peak_bytes = 0;
    int num_cus = 256;
    hipDeviceProp_t prop;
    std::vector<mgta::DevBuf> pool;   // grow-only scratch kept between calls
    mgta::AstarArenas astar;
    std::vector<int64_t> edge_counting;   // (k+1)-mer multiplicity histogram of the last stage-1 run (.counting)
    const void *last_rec = nullptr;   // records of the last build pass, still resident in the pool
    uint64_t last_n_rec = 0;
    uint32_t last_bucket_lo = 0, last_bucket_hi = 0;
    const void *last_tips = nullptr;  // tip labels of that pass (words_per_tip words each), and where every bucket starts ([nb][3], -1 = empty)
    const void *last_first = nullptr;
    uint64_t last_n_tips = 0;
    int last_k = 0, last_words_per_tip = 0;
    // mgta_ctx_keep_stream: a build of several memory-bound passes also leaves its WHOLE edge stream on the device (records and tip
    // labels of every pass appended here, records per bucket on the host), so that mgta_sdbg_load_resident works at any size
    int keep_stream = 0;
    bool acc_valid = false;
    mgta::DevBuf acc_rec, acc_tips;
    uint64_t acc_n_rec = 0, acc_n_tips = 0;
    std::vector<int64_t> acc_items;
    // mgta_ctx_keep_multiplicity: loads keep the full edge multiplicities.  The large words (records stored as 255) of the last pass
    // are in the pool; a kept multi-pass stream accumulates them here when the build ran with the switch on (acc_has_large)
    int keep_multiplicity = 0;
    uint64_t coverage_batch_windows = 0;   // mgta_ctx_set_coverage_batch (0 = the library's default)
    uint64_t align_batch_cells = 0;        // mgta_ctx_set_align_batch: cells (L * M) of one batch of mgta_seqs_align (0 = by free memory)
    uint64_t posterior_batch_cells = 0;    // mgta_ctx_set_posterior_batch: cells (L * M) of one batch of mgta_seqs_posterior (0 = by free memory)
    uint64_t nearest_batch_cells = 0;      // mgta_ctx_set_nearest_batch: cells (L * R) of one trace batch of mgta_seqs_nearest (0 = by free memory)
    uint64_t chimera_segment_cols = 0;     // mgta_ctx_set_chimera_segment: reference columns of one segment of mgta_seqs_chimera (0 = the library's default)
    uint64_t chimera_groups = 0;           // mgta_ctx_set_chimera_groups: groups of segments per (contig, direction) of mgta_seqs_chimera (0 = by the number of contigs)
    uint64_t cluster_tile_rows = 0;        // mgta_ctx_set_cluster_tile: rows of one row block of mgta_rows_pairs (0 = the library's default)
    int derep_hash_bits = 64;    // mgta_ctx_set_derep_hash_bits: bits of both hashes mgta_seqs_derep keeps (fewer = more collisions, same answers)
    int share_hash_bits = 64;    // mgta_ctx_set_share_hash_bits: bits of the hash the count table of mgta_contig_share_coverage keeps (fewer = more collisions, same answers)
    uint32_t pileup_chunk = 0;   // mgta_ctx_set_pileup_chunk: reads a group takes per visit to the queue head of mgta_reads_pileup (0 = the library's choice)
    uint32_t phase_chunk = 0;    // mgta_ctx_set_phase_chunk: fragment slots a group takes per visit to the queue head of mgta_reads_phase (0 = the library's choice)
    uint32_t recruit_chunk = 0;  // mgta_ctx_set_recruit_chunk: reads a wave takes per visit to the queue head of mgta_reads_recruit (0 = the library's choice)
    const void *last_large = nullptr;
    uint64_t last_n_large = 0;
    mgta::DevBuf acc_large;
    uint64_t acc_n_large = 0;
    bool acc_has_large = false;
};

namespace mgta {
inline void ctx_retain(mgta_ctx *c) { __atomic_add_fetch(&c->refs, 1, __ATOMIC_RELAXED); }
void ctx_release(mgta_ctx *c);    // frees the context when the last reference goes (ctx.hip)
// the context no longer names the output of its last build (its buffers went, or now belong to something else)
inline void forget_last_build(mgta_ctx *c) {
    c->last_rec = nullptr; c->last_tips = nullptr; c->last_first = nullptr; c->last_n_rec = 0; c->last_n_tips = 0; c->last_k = 0;
    c->last_large = nullptr; c->last_n_large = 0;
}
}  // namespace mgta

struct mgta_hmm {
    mgta_ctx *ctx = nullptr;
    int M = 0, A = 0;
    mgta::DevBuf tab;            // [msc (M+1)*A][tsc 7*(M+1)][maxm (M+1)][h 3*(M+1)]
    int8_t col[2][64];           // codon (c1*16+c2*4+c3) -> emission column; [0] codonTable, [1] rc_codonTable; -1 = stop
    mgta::DevBuf d_col;          // the same 128 bytes on the device
    int8_t alpha[128];           // residue letter -> emission column, -1 = unknown (and [127])
    mgta::DevBuf d_alpha;        // the same 128 bytes on the device
    size_t n_doubles = 0;
};

struct mgta_reads {
    mgta_ctx *ctx = nullptr;
    const uint32_t *d_packed = nullptr;   // padded with >= 16 zero words past n_words
    const uint64_t *d_start = nullptr;    // [n_reads+1]
    uint64_t n_words = 0, n_reads = 0;
    mgta::DevBuf own_packed, own_start;   // empty when adopted
};
