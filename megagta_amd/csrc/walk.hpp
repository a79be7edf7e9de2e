// walk.hpp -- the walk along the resident graph, k + 1 letters at a time, and what the kernels that walk share.
//
// Device.  A group of 8 lanes owns a sequence.  walk_next is the step-or-search of one window: a forward step (cov_step) from the
// edge of the window before, an index search (g_index_edge, graph.hpp) where that window had none.  On it stands walk_contig, the
// walk over symbols 0..4 (0 = no base: the walk starts again behind it), which hands every window's edge (-1 = none) to a sink;
// cov_walk_kernel and match_mark_kernel (coverage.hip) call it.
// Four kernels keep the loop written out, because each was measurably slower on a walker (profiles/walk/README.md):
// share_walk_kernel here for the contig walk; match_walk_kernel, sample_scan_kernel (coverage.hip) and pile_scan_kernel (pileup.hip)
// for the read walk, which therefore has no walker.  A change of the walk is made in five places: walk_next and these four.
// tests/test_walk_edges_gpu.py pins all five copies edge by edge: on graphs whose edge i has multiplicity i + 1 the two contig walks
// must report the id of every window's edge, and the three read walks the same edges up to strand, at k = 20 .. 127, over every
// branch of cov_step (the census in tests/test_walk_edges_host.py), before and after `denovo` has consumed the validity bits.
// They share the small pieces: the queue dequeue of a group (grp_next_chunk; phase.hip's slot queue too, pile_scan_kernel not:
// its all-lanes form measured faster), the decode of a
// packed base (packed_symbol) and the mark bits (edge_marked, mark_edge); walk_contig's callers also the counts of a walk and their
// flush (WalkCounts).  Further down: the edge-keyed table of a call's contig windows on both strands (SampleTable with its add,
// find, count and numbering kernels) and the symbol kernels.
// Host (needs HIP; the plain part -- CovJob, the offsets check, the batch cutter -- is contig_jobs.hpp): marks_reset, table_slots
// and sample_table_alloc, stage_symbols, queue_per_cu and queue_launch, window_scratch.
// coverage.hip, pileup.hip and phase.hip include this file; every kernel has internal linkage, so each compiles its own copy.
#pragma once
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "contig_jobs.hpp"
#include "device_utils.hpp"
#include "graph.hpp"

namespace mgta {
namespace {

constexpr int kCovThreads = 256;          // 4 waves = 32 groups of 8 lanes
constexpr int kCovGroups = kCovThreads / 8;

// letters -> symbols 1..4 (A C G T in either case), 0 for anything else (an N is NOT folded to G: it was never counted); in place
__global__ __launch_bounds__(256) void cov_symbols_kernel(uint8_t *s, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint32_t c = s[i] & 0xDFu;
        s[i] = (uint8_t)(c == 'A' ? 1 : c == 'C' ? 2 : c == 'G' ? 3 : c == 'T' ? 4 : 0);
    }
}

// A group of 8 lanes fetches line li with one request, 16 bytes per lane, and hands every lane the whole line (sub = lane & 7).
// All 8 lanes of a group run the same control flow on the same values, so the shuffles always find their source lane active.
__device__ __forceinline__ LineR grp_load_line(const GraphDev &g, uint64_t li, int sub) {
    const uint4 v = reinterpret_cast<const uint4 *>(g.lines + li)[sub];
    const uint64_t lo = (uint64_t)v.x | ((uint64_t)v.y << 32), hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
    LineR L;
    L.w0 = __shfl(lo, 0, 8); L.w1 = __shfl(hi, 0, 8); L.w2 = __shfl(lo, 1, 8); L.w3 = __shfl(hi, 1, 8);
    L.last = __shfl(lo, 2, 8); L.tip = __shfl(hi, 2, 8); L.invalid = __shfl(lo, 3, 8); L.multi1 = 0;
    L.rank_last = __shfl(lo, 4, 8);
    L.rw0 = __shfl(lo, 5, 8); L.rw1 = __shfl(hi, 5, 8); L.rw2 = __shfl(lo, 6, 8); L.rw3 = __shfl(hi, 6, 8);
    L.h01 = __shfl(lo, 7, 8); L.h23 = __shfl(hi, 7, 8);
    return L;
}

// One forward step of the walk.  In: e = the edge of the window before, L = its line (e >> 6), c = the next base (1..4).
// Out: the edge of the next window, i.e. the edge of the node Forward(e) points to (succinct_dbg.h:155-164) whose label is c or c + 4,
// with L = its line; -1 when that node has no such edge.
//
// This is NOT g_outgoing / g_out_all_fd: those answer -1 for a start edge whose `invalid` bit is set and skip invalid target edges
// (tips and $ edges after a load, everything `denovo` removed), while IndexBinarySearchEdge -- the contract of a window -- does not look
// at that bit, and such an edge has a multiplicity in the stream like any other.  So the step forwards from any edge and scans the
// target node exactly as IndexBinarySearchEdge scans the node it found: from the node's `last` edge downwards to the next last | tip bit.
__device__ __forceinline__ int64_t cov_step(const GraphDev &g, LineR &L, int64_t e, int c, int sub) {
    int a = l_W(L, e);
    if (a > 4) a -= 4;
    if (a == 0) return -1;
    int64_t cnt;                                                          // Rank(a, e) from the registers (rank_and_select.h:153)
    if (e >= g.size - 1) cnt = a == 1 ? g.total_w[1] : a == 2 ? g.total_w[2] : a == 3 ? g.total_w[3] : g.total_w[4];
    else {
        const int j = (int)(e & 63), fw = j >> 4;
        const int nb = (j & 15) + 1;
        const uint64_t m = nb == 16 ? ~0ull : ((1ull << (4 * nb)) - 1);
        cnt = (int64_t)sel4(L.rw0, L.rw1, L.rw2, L.rw3, a - 1);
        const uint64_t e0 = nib_eq(L.w0, a), e1 = nib_eq(L.w1, a), e2 = nib_eq(L.w2, a), e3 = nib_eq(L.w3, a);
        cnt += __popcll(fw > 0 ? e0 : (e0 & m));
        if (fw >= 1) cnt += __popcll(fw > 1 ? e1 : (e1 & m));
        if (fw >= 2) cnt += __popcll(fw > 2 ? e2 : (e2 & m));
        if (fw >= 3) cnt += __popcll(e3 & m);
    }
    const int64_t rf = a == 1 ? g.rank_f[1] : a == 2 ? g.rank_f[2] : a == 3 ? g.rank_f[3] : g.rank_f[4];
    const int64_t r = rf + cnt - 1;
    if (r >= g.total_last || r < 0) return -1;
    const uint64_t hh = (a <= 2) ? L.h01 : L.h23;
    uint64_t li = (a & 1) ? (hh & 0xFFFFFFFFull) : (hh >> 32);           // fwd_hint[a - 1]
    LineR A = grp_load_line(g, li, sub);                                  // the one dependent line of this window
    uint64_t next_rank = A.rank_last + (uint64_t)__popcll(A.last);
    while (li + 1 < g.n_lines && (int64_t)next_rank <= r) {               // rare: the target is a line further
        ++li;
        A = grp_load_line(g, li, sub);
        next_rank = A.rank_last + (uint64_t)__popcll(A.last);
    }
    int64_t x = (int64_t)(li << 6) + select64(A.last, (int)(r - (int64_t)A.rank_last));
    do {                                                                  // succinct_dbg.cpp:540-548
        const bool in = (uint64_t)(x >> 6) == li;                         // almost always: the node's edges sit in the target line
        const int lab = in ? l_W(A, x) : g_W(g, x);
        if (lab == c || lab - 4 == c) {
            L = in ? A : grp_load_line(g, (uint64_t)x >> 6, sub);
            return x;
        }
        --x;
    } while (x >= 0 && !(((uint64_t)(x >> 6) == li) ? g_bit(A.last | A.tip, x) : (int)g_last_or_tip(g, x)));
    return -1;
}

struct WalkCounts {                       // of one lane's walks; all 8 lanes of a group hold the same numbers
    uint32_t walked = 0, searched = 0;    // windows found by a step; index searches
};

// the groups' counts -> *walked and *searched: the sum over the group leaders of a wave, one atomic per wave and counter
__device__ __forceinline__ void walk_counts_flush(const WalkCounts &n, int sub, unsigned long long *walked, unsigned long long *searched) {
    const uint32_t w = wave_sum(sub == 0 ? n.walked : 0u), sc = wave_sum(sub == 0 ? n.searched : 0u);
    if (lane_id() == 0) {
        if (w) atomicAdd(walked, (unsigned long long)w);
        if (sc) atomicAdd(searched, (unsigned long long)sc);
    }
}

// A group takes the next `chunk` items of a queue: its first lane moves the head, and the shuffle that hands the old value round sits
// behind the branch, where the 8 lanes are together again.
__device__ __forceinline__ unsigned long long grp_next_chunk(unsigned long long *head, uint32_t chunk, int sub) {
    unsigned long long first = 0;
    if (sub == 0) first = atomicAdd(head, (unsigned long long)chunk);
    return __shfl(first, 0, 8);
}

// one mark bit per edge (mgta_sdbg::marks)
__device__ __forceinline__ bool edge_marked(const uint32_t *marks, int64_t e) { return (marks[e >> 5] >> (e & 31)) & 1u; }

// turns the bit of edge e on; true in the one lane that found it off
__device__ __forceinline__ bool mark_edge(uint32_t *marks, int64_t e) {
    const uint32_t bit = 1u << (e & 31);
    return !(atomicOr(&marks[e >> 5], bit) & bit);
}

// The edge of the next window.  In: e = the edge of the window before (L = its line), -1 = the walk has to start again; c = the
// window's last symbol; window() = its k + 1 symbols, asked for only when it has to be searched.
template <class Window>
__device__ __forceinline__ int64_t walk_next(const GraphDev &g, LineR &L, int64_t e, int c, int sub, WalkCounts &n, Window &&window) {
    if (e >= 0) {
        e = cov_step(g, L, e, c, sub);
        if (e >= 0) ++n.walked;
    } else {
        e = g_index_edge(g, window());
        ++n.searched;
        if (e >= 0) L = grp_load_line(g, (uint64_t)e >> 6, sub);
    }
    return e;
}

// The walk along the len symbols at s (1..4, 0 = no base): sink(p, e) once per window p, e = its edge, -1 for none.  A window with a
// 0 in it has no edge, and the walk starts again with the first window behind it.
template <class Sink>
__device__ __forceinline__ void walk_contig(const GraphDev &g, const uint8_t *s, uint32_t len, int sub, WalkCounts &n, Sink &&sink) {
    const int k = g.k;
    const uint32_t n_win = len > (uint32_t)k ? len - (uint32_t)k : 0;
    int run = 0;                                                          // A C G T letters in a row, up to the window's last letter
    for (int i = 0; i < k && (uint32_t)i < len; ++i) run = s[i] ? run + 1 : 0;
    int64_t e = -1;
    LineR L{};
    for (uint32_t p = 0; p < n_win; ++p) {
        const int c = s[p + k];
        run = c ? run + 1 : 0;
        e = run > k ? walk_next(g, L, e, c, sub, n, [&]() { return s + p; }) : -1;
        sink(p, e);
    }
}

// base q of the packed reads (2 bits per base, base j of a word at bits 30 - 2j) out of its word w = packed[q >> 4], as a symbol
// 1..4; flip = 3 gives the complement
__device__ __forceinline__ uint32_t packed_symbol(uint32_t w, uint64_t q, uint32_t flip) { return (((w >> (30 - 2 * (int)(q & 15))) & 3u) ^ flip) + 1; }

constexpr int kMatchMaxWindow = 128;      // k + 1 symbols of an index search, staged in LDS per group (32 groups: 4 KB per workgroup)

// the reverse complement of all n symbols behind them: s[n + i] = complement of s[n - 1 - i] (0 stays 0), so the reverse complement
// of the contig at [a, b) lies at [2n - b, 2n - a)
__global__ __launch_bounds__(256) void match_rc_symbols_kernel(uint8_t *s, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint32_t c = s[n - 1 - i];
        s[n + i] = (uint8_t)(c ? 5u - c : 0u);
    }
}

constexpr unsigned long long kShareEmpty = ~0ull;                         // (an edge id is < 2^63)

// The edge id of every window of the jobs (8 bytes, -1 = none), where cov_walk_kernel leaves the multiplicity.  The loop is
// walk_contig's, written out: on walk_contig this kernel compiled to the same registers and loads, yet took 2.7 % longer where
// every window is an index search (profiles/walk/README.md).
// counters: [0] queue head, [1] windows found by a step, [2] index searches ([3] .. [6] belong to the count and numbering kernels)
__global__ __launch_bounds__(kCovThreads) void share_walk_kernel(GraphDev g, const uint8_t *sym, const CovJob *jobs, uint32_t n_jobs, uint32_t chunk, int64_t *ids,
                                                                 unsigned long long *counters) {
    const int sub = threadIdx.x & 7;
    const int k = g.k;
    uint32_t walked = 0, searched = 0;
    for (;;) {
        const unsigned long long first = grp_next_chunk(&counters[0], chunk, sub);
        if (first >= n_jobs) break;
        const uint32_t j_end = (uint32_t)min((unsigned long long)n_jobs, first + chunk);
        for (uint32_t j = (uint32_t)first; j < j_end; ++j) {
            const CovJob job = jobs[j];
            const uint8_t *s = sym + job.off;
            const uint32_t n_win = job.len > (uint32_t)k ? job.len - (uint32_t)k : 0;
            int64_t *out = ids + job.win_base;
            int run = 0;                                                  // A C G T letters in a row, up to the window's last letter
            for (int i = 0; i < k && (uint32_t)i < job.len; ++i) run = s[i] ? run + 1 : 0;
            int64_t e = -1;                                               // the edge of the window before, -1 = the walk has to start again
            LineR L{};
            int64_t mine = -1;
            for (uint32_t p = 0; p < n_win; ++p) {
                const int c = s[p + k];
                run = c ? run + 1 : 0;
                if (run > k) {
                    if (e >= 0) {
                        e = cov_step(g, L, e, c, sub);
                        if (e >= 0) ++walked;
                    } else {
                        e = g_index_edge(g, s + p);
                        ++searched;
                        if (e >= 0) L = grp_load_line(g, (uint64_t)e >> 6, sub);
                    }
                } else e = -1;
                // eight windows leave as one 64-byte store of the group
                if ((int)(p & 7) == sub) mine = e;
                if ((p & 7) == 7 || p + 1 == n_win) {
                    const uint32_t q = (p & ~7u) + (uint32_t)sub;
                    if (q <= p) out[q] = mine;
                }
            }
        }
    }
    const uint32_t w = wave_sum(sub == 0 ? walked : 0u), sc = wave_sum(sub == 0 ? searched : 0u);
    if (lane_id() == 0) {
        if (w) atomicAdd(&counters[1], (unsigned long long)w);
        if (sc) atomicAdd(&counters[2], (unsigned long long)sc);
    }
}

// the value lane `src` (the same in every lane) holds
__device__ __forceinline__ int64_t wave_read64(int64_t v, int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), src);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ uint64_t mix64_share(uint64_t x) {             // the finaliser of splitmix64, as in derep.hip
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

struct SampleTable {
    unsigned long long *keys;
    uint32_t *share, *dense;
    uint64_t n_slots, hmask;
};

// `times` as-given occurrences of edge e (0 for a reverse-complement window) -> its slot; 0 and *full = 1 when the table has no room
__device__ __forceinline__ uint32_t sample_table_add(const SampleTable &t, int64_t e, uint32_t times, uint32_t *marks, uint32_t &n_new, unsigned long long *full) {
    uint64_t slot = mix64_share((uint64_t)e) & t.hmask & (t.n_slots - 1);
    if (slot == 0) slot = 1;
    for (uint64_t tries = 0; tries < t.n_slots; ++tries) {
        unsigned long long key = __hip_atomic_load(&t.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (key == kShareEmpty) {
            key = atomicCAS(&t.keys[slot], kShareEmpty, (unsigned long long)e);
            if (key == kShareEmpty) {                                     // this lane made the key: the read scan looks at marked edges only
                mark_edge(marks, e);
                ++n_new;
                key = (unsigned long long)e;
            }
        }
        if (key == (unsigned long long)e) {
            if (times) atomicAdd(&t.share[slot], times);
            return (uint32_t)slot;
        }
        slot = (slot + 1) & (t.n_slots - 1);
        if (slot == 0) slot = 1;
    }
    atomicExch(full, 1ull);
    return 0;
}

// the slot of edge e, 0 when it is no key (the table is final and at most half full: an empty slot ends every probe)
__device__ __forceinline__ uint32_t sample_table_find(const SampleTable &t, int64_t e) {
    uint64_t slot = mix64_share((uint64_t)e) & t.hmask & (t.n_slots - 1);
    if (slot == 0) slot = 1;
    for (uint64_t tries = 0; tries < t.n_slots; ++tries) {
        const unsigned long long key = t.keys[slot];
        if (key == (unsigned long long)e) return (uint32_t)slot;
        if (key == kShareEmpty) return 0;
        slot = (slot + 1) & (t.n_slots - 1);
        if (slot == 0) slot = 1;
    }
    return 0;
}

// share_count_kernel's shape over the jobs of both strands (job.idx = 2 * contig + strand; the ids of a reverse-complement job lie
// n_win_batch behind those of its contig, its window p is window n_win - 1 - p of the contig).
// counters: [3] keys made, [5] set when the table ran full
__global__ __launch_bounds__(256) void sample_count_kernel(SampleTable t, const CovJob *jobs, uint32_t n_jobs, int k, const int64_t *ids, uint64_t n_win_batch,
                                                           uint64_t win_done, uint32_t *slots_own, uint32_t *slots_rc, uint32_t *marks, unsigned long long *counters) {
    const int lane = lane_id();
    const uint32_t j = blockIdx.x * 64 + (uint32_t)lane;
    uint32_t n_win = 0;
    uint64_t base = 0;
    bool rc = false;
    if (j < n_jobs) {
        const CovJob job = jobs[j];
        n_win = job.len > (uint32_t)k ? job.len - (uint32_t)k : 0;
        base = job.win_base;
        rc = job.idx & 1u;
    }
    const uint64_t longest = wave_max(n_win);
    const uint64_t given = __ballot(!rc);
    uint32_t n_new = 0;
    for (uint64_t p0 = ((uint64_t)blockIdx.y * 4 + (uint64_t)wave_id()) * 64; p0 < longest; p0 += (uint64_t)gridDim.y * 256) {
        const uint64_t p1 = min(longest, p0 + 64);
        for (uint64_t p = p0; p < p1; ++p) {
            const bool in = p < n_win;
            const int64_t e = in ? ids[base + p] : -1;
            int leader = lane;
            uint32_t times = rc ? 0u : 1u;
            uint64_t todo = __ballot(e >= 0);
            while (todo) {                                                // one turn per distinct id among the 64
                const int src = __ffsll((long long)todo) - 1;
                const int64_t e0 = wave_read64(e, src);
                const uint64_t same = __ballot(e == e0);
                if (e == e0) { leader = src; times = (uint32_t)__popcll(same & given); }
                todo &= ~same;
            }
            uint32_t slot = 0;
            if (e >= 0 && leader == lane) slot = sample_table_add(t, e, times, marks, n_new, &counters[5]);
            slot = __shfl(slot, leader, 64);
            if (in) {
                if (rc) slots_rc[win_done + (base - n_win_batch) + ((uint64_t)n_win - 1 - p)] = slot;
                else slots_own[win_done + base + p] = slot;
            }
        }
    }
    n_new = wave_sum(n_new);
    if (lane == 0 && n_new) atomicAdd(&counters[3], (unsigned long long)n_new);
}

// the keys get the numbers 1 .. n_keys (the order is the table's, which no output depends on); n_slots is a multiple of 1024
// counters: [6] keys numbered so far
__global__ __launch_bounds__(256) void sample_dense_kernel(SampleTable t, unsigned long long *counters) {
    const int lane = lane_id();
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < t.n_slots; i += stride) {
        const bool used = t.keys[i] != kShareEmpty;
        const uint64_t m = __ballot(used);
        unsigned long long first = 0;
        if (lane == 0 && m) first = atomicAdd(&counters[6], (unsigned long long)__popcll(m));
        first = wave_uniform((uint64_t)first);
        t.dense[i] = used ? (uint32_t)(first + (uint64_t)__popcll(m & lanemask_lt()) + 1) : 0u;
    }
}

// ---- the packed reads, as the scans of pileup.hip and phase.hip read them

// the longest of the reads [0, n_reads) (atomicMax into *out, zeroed by the caller)
__global__ __launch_bounds__(256) void pile_maxlen_kernel(const uint64_t *start, uint64_t n_reads, unsigned long long *out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    unsigned long long mx = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_reads; r += stride) mx = max(mx, (unsigned long long)(start[r + 1] - start[r]));
    if (mx) atomicMax(out, mx);
}

// base j of the read in orientation o as a symbol 1..4.  same = (o == the orientation the stored order walks), comp = 3 for o = 1
__device__ __forceinline__ uint32_t pile_base(const uint32_t *packed, uint64_t s0, uint32_t len, int same, uint32_t comp, uint32_t j) {
    const uint64_t q = s0 + (same ? j : len - 1 - j);
    return packed_symbol(packed[q >> 4], q, comp);
}

// ---- the host side the calls share (the part that needs no HIP is contig_jobs.hpp)

// the per-window scratch: a key buffer of the build pool when it is large enough (it sits idle between the steps), grown otherwise
uint16_t *window_scratch(mgta_ctx *ctx, uint64_t bytes) {
    if ((int)ctx->pool.size() < S_NUM) ctx->pool.resize(S_NUM);
    DevBuf &b = ctx->pool[S_KEYS_A];
    if (!b.p || b.bytes < bytes) {
        b.release();
        b.alloc(bytes, &ctx->live_bytes, &ctx->peak_bytes);
    }
    return b.as<uint16_t>();
}

// one mark bit per edge, the graph's own, grown where needed and zeroed per call = per set of contigs
uint32_t *marks_reset(mgta_sdbg *g, hipStream_t st) {
    const size_t mark_b = ((size_t)std::max<int64_t>(g->dev.size, 0) / 32 + 2) * 4;
    if (g->marks.bytes < mark_b) g->marks.alloc(mark_b, &g->ctx->live_bytes, &g->ctx->peak_bytes);
    MGTA_HIP_CHECK(hipMemsetAsync(g->marks.p, 0, mark_b, st));
    return g->marks.as<uint32_t>();
}

// the slots of an edge-keyed table of at most most_keys keys: at most half full, a power of two, never more than 2^32 (a slot number is
// 32 bits; slot 0 is "no edge"); and the bits of the hash the context lets it keep
uint64_t table_slots(uint64_t most_keys) {
    uint64_t n_slots = 1024;
    while (n_slots < 2 * most_keys + 2 && n_slots < (1ull << 32)) n_slots <<= 1;
    return n_slots;
}
uint64_t table_hmask(const mgta_ctx *ctx) { return ctx->share_hash_bits >= 64 ? ~0ull : (1ull << ctx->share_hash_bits) - 1; }

struct SampleTableMem {
    DevBuf keys, share, dense;
    SampleTable t;
};

// an empty SampleTable for most_keys keys (the caller has checked that its slots fit); the bytes are counted in *live and *peak
void sample_table_alloc(mgta_ctx *ctx, hipStream_t st, uint64_t most_keys, uint64_t *live, uint64_t *peak, SampleTableMem &m) {
    const uint64_t n_slots = table_slots(most_keys);
    m.keys.alloc(n_slots * 8, live, peak);
    m.share.alloc(n_slots * 4, live, peak);
    m.dense.alloc(n_slots * 4, live, peak);
    m.t = SampleTable{m.keys.as<unsigned long long>(), m.share.as<uint32_t>(), m.dense.as<uint32_t>(), n_slots, table_hmask(ctx)};
    MGTA_HIP_CHECK(hipMemsetAsync(m.keys.p, 0xFF, n_slots * 8, st));
    MGTA_HIP_CHECK(hipMemsetAsync(m.share.p, 0, n_slots * 4, st));
}

// n_bytes letters -> symbols in d_sym (which holds n_bytes, or 2 n_bytes with both_strands: the reverse complement of all of them
// behind).  timed, where given, is started behind the upload: it measures the symbol kernels and what the caller launches next.
void stage_symbols(mgta_ctx *ctx, hipStream_t st, DevBuf &d_sym, const char *seqs, uint64_t n_bytes, bool both_strands, Timer *timed = nullptr) {
    if (n_bytes) MGTA_HIP_CHECK(hipMemcpyAsync(d_sym.p, seqs, n_bytes, hipMemcpyHostToDevice, st));
    if (timed) timed->start();
    if (!n_bytes) return;
    const unsigned blocks = (unsigned)std::min<uint64_t>((n_bytes + 255) / 256, (uint64_t)ctx->num_cus * 16);
    hipLaunchKernelGGL(cov_symbols_kernel, dim3(blocks), dim3(256), 0, st, d_sym.as<uint8_t>(), n_bytes);
    if (both_strands) hipLaunchKernelGGL(match_rc_symbols_kernel, dim3(blocks), dim3(256), 0, st, d_sym.as<uint8_t>(), n_bytes);
}

// The launch of a kernel whose groups of 8 lanes take their items from one atomic head.  per_cu = the workgroups a CU holds at once:
// what the kernel's registers allow, asked of the runtime once per call (queue_per_cu; never assumed).  A group takes `chunk` items
// per visit to the head (one word saturates near 88 dequeues per microsecond): big_chunk where every group in flight has at least
// `threshold` items, else 1; 64 and 4 for contigs, 256 and 16 for reads.  chunk_override != 0 is the caller's own chunk.
struct QueueLaunch {
    int per_cu;
    uint32_t chunk;
    unsigned blocks;
    int64_t groups_per_cu() const { return (int64_t)per_cu * kCovGroups; }
};

template <class K>
int queue_per_cu(K kernel) {
    int per_cu = 0;
    MGTA_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kCovThreads, 0));
    return std::max(1, per_cu);
}

QueueLaunch queue_launch(const mgta_ctx *ctx, int per_cu, uint64_t n_items, uint64_t threshold, uint32_t big_chunk, uint32_t chunk_override = 0) {
    QueueLaunch q{per_cu, 1, 1};
    const uint64_t resident = (uint64_t)ctx->num_cus * (uint64_t)per_cu;
    q.chunk = chunk_override ? chunk_override : (n_items >= resident * kCovGroups * threshold ? big_chunk : 1u);
    const uint64_t per_block = (uint64_t)kCovGroups * q.chunk;
    q.blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(resident, (n_items + per_block - 1) / per_block));
    return q;
}
}  // namespace
}  // namespace mgta
