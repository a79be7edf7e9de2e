// coverage.hip — per-contig k-mer coverage and abundance from the resident graph, the batched EdgeMultiplicity query, and read
// recruitment (the reads that share a (k+1)-mer with a set of contigs: the same walk, over reads; further down), and the
// window-shared coverage (every edge's multiplicity split among the windows of the call that land on it: the same walk, once, then
// a count per distinct edge), and the per-library coverage (the read windows of every library on the windows of a set of contigs: the
// read walk again, with a count per key and library; at the end).
//
// The reference's last post-processing step (`kmer_coverage`, bin/post_proc.sh:113-118) counts the (k+1)-mers of the contigs in a
// second pass over all reads.  That count is the multiplicity the edge stream already carries (sdbg_multi_io.h:83-112) and a graph
// loaded under mgta_ctx_keep_multiplicity still holds (SuccinctDBG::EdgeMultiplicity, succinct_dbg.h:133-147): the coverage of a
// contig is one walk along it.
//
// A window's edge is what IndexBinarySearchEdge (succinct_dbg.cpp:530-549) finds for its k + 1 letters.  Only the first window of a
// contig is found that way; the edge of the next window is the edge of the node Forward(e) points to whose label is the next base:
// ONE dependent graph line per window.  That is a pointer chase (0.5-0.65 us per dependent line), so the parallelism is
// across contigs: a group of 8 lanes owns a contig and reads a line with one request (16 bytes per lane, the shape of probe.hip),
// 32 groups per workgroup, as many workgroups per CU as the kernel's registers allow (asked of the runtime at the launch and
// reported in mgta_coverage_stats.groups_per_cu).  As compiled for gfx950 the walk takes 111 VGPRs = 4 waves per SIMD = 4 workgroups
// = 128 groups = 128 independent lines in flight per CU, half of the 256 DESIGN 5 names for the full random-line rate: asking the
// compiler for 8 waves per SIMD (64 VGPRs) spills 72 VGPRs to scratch memory (its resource report), so it is not asked.  Contigs are
// handed out longest first from one atomic head, a few at a time.
//
// What the walks share is in walk.hpp: the step-or-search of a window (walk_next), the contig walker walk_contig, the queue dequeue
// (grp_next_chunk), the decode of a packed base (packed_symbol), the mark bits and the counts of a walk.  cov_walk_kernel
// (multiplicity, abundance) and match_mark_kernel (marking) are a prologue, a call of walk_contig with what they do with a window's
// edge, and an epilogue.  match_walk_kernel and sample_scan_kernel keep the read walk written out, as share_walk_kernel in walk.hpp
// keeps the contig walk: on a walker they were measurably slower (profiles/walk/README.md).  SampleTable and the symbol kernels,
// which pileup.hip uses too, are in walk.hpp as well.  The host side of the entry points stands on contig_jobs.hpp (the offsets
// check, the batch cutter, the job list of one strand or both, the window offsets) and on walk.hpp's marks_reset,
// sample_table_alloc, stage_symbols and queue_launch.
#include <algorithm>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "device_utils.hpp"
#include "graph.hpp"
#include "walk.hpp"

namespace mgta {
namespace {

constexpr int kCovLowBins = 256;          // abundance bins counted in LDS per workgroup (where nearly all edges are); the rest go straight to device memory

// walk_contig with the multiplicity of every window's edge (0 = none) as the per-window value, and the abundance of the call's edges
// counters: [0] queue head, [1] windows found by a step, [2] index searches
__global__ __launch_bounds__(kCovThreads) void cov_walk_kernel(GraphDev g, MultDev m, const uint8_t *sym, const CovJob *jobs, uint32_t n_jobs, uint32_t chunk,
                                                               uint16_t *pw, uint32_t *marks, unsigned long long *abund, unsigned long long *counters) {
    __shared__ uint32_t s_hist[kCovLowBins];
    for (int i = threadIdx.x; i < kCovLowBins; i += kCovThreads) s_hist[i] = 0;
    __syncthreads();
    const int sub = threadIdx.x & 7;
    WalkCounts n;
    for (;;) {
        const unsigned long long first = grp_next_chunk(&counters[0], chunk, sub);
        if (first >= n_jobs) break;
        const uint32_t j_end = (uint32_t)min((unsigned long long)n_jobs, first + chunk);
        for (uint32_t j = (uint32_t)first; j < j_end; ++j) {
            const CovJob job = jobs[j];
            const uint32_t n_win = job.len > (uint32_t)g.k ? job.len - (uint32_t)g.k : 0;
            uint16_t *out = pw + job.win_base;
            uint32_t mine = 0;
            walk_contig(g, sym + job.off, job.len, sub, n, [&](uint32_t p, int64_t e) {
                uint32_t cov = 0;
                if (e >= 0) {
                    cov = g_edge_mult(m, e);
                    if (marks && sub == 0 && mark_edge(marks, e)) {       // abundance: the lane that turns the edge's bit on counts the edge
                        if (cov < (uint32_t)kCovLowBins) atomicAdd(&s_hist[cov], 1u);
                        else atomicAdd(&abund[cov], 1ull);
                    }
                }
                // eight windows leave as one 16-byte store of the group
                if ((int)(p & 7) == sub) mine = cov;
                if ((p & 7) == 7 || p + 1 == n_win) {
                    const uint32_t q = (p & ~7u) + (uint32_t)sub;
                    if (q <= p) out[q] = (uint16_t)mine;
                }
            });
        }
    }
    __syncthreads();
    if (marks)
        for (int i = threadIdx.x; i < kCovLowBins; i += kCovThreads)
            if (s_hist[i]) atomicAdd(&abund[i], (unsigned long long)s_hist[i]);
    walk_counts_flush(n, sub, &counters[1], &counters[2]);
}

// the bin of `h` (256 bins, 4 per lane) that holds the r-th element (0-based) of what was counted; rem = its rank inside the bin
__device__ __forceinline__ uint32_t cov_select_bin(const uint32_t *h, uint32_t r, uint32_t &rem) {
    const int lane = lane_id();
    const uint32_t c0 = h[lane * 4], c1 = h[lane * 4 + 1], c2 = h[lane * 4 + 2], c3 = h[lane * 4 + 3];
    const uint32_t tot = c0 + c1 + c2 + c3, incl = wave_incl_scan(tot), excl = incl - tot;
    const bool here = excl <= r && r < incl;
    uint32_t bin = 0, left = 0;
    if (here) {
        uint32_t q = r - excl;
        if (q < c0) bin = lane * 4;
        else if ((q -= c0) < c1) bin = lane * 4 + 1;
        else if ((q -= c1) < c2) bin = lane * 4 + 2;
        else { q -= c2; bin = lane * 4 + 3; }
        left = q;
    }
    const uint64_t who = __ballot(here);
    const int src = who ? __ffsll((long long)who) - 1 : 0;
    rem = __shfl(left, src, 64);
    return __shfl(bin, src, 64);
}

// One wave per contig over its per-window slice.  The median (lower median, zeros included) by a counting select over the 16-bit
// value range: the high byte, then the low byte among the values of that high byte -- no sort.
__global__ __launch_bounds__(256) void cov_stats_kernel(const CovJob *jobs, uint32_t n_jobs, int k, const uint16_t *pw, mgta_contig_cov *out) {
    __shared__ uint32_t s_h[4][256];
    const int w = wave_id(), lane = lane_id();
    const uint32_t j = blockIdx.x * 4 + (uint32_t)w;
    if (j >= n_jobs) return;                                              // (whole waves leave; the rest use wave-level ordering only)
    const CovJob job = jobs[j];
    const uint32_t n_win = job.len > (uint32_t)k ? job.len - (uint32_t)k : 0;
    const uint16_t *v = pw + job.win_base;
    mgta_contig_cov res;
    res.sum = 0; res.len = job.len; res.n_windows = n_win; res.n_covered = 0; res.min = 0; res.max = 0; res.median = 0;
    if (n_win) {
        uint64_t sum = 0;
        uint32_t mn = 0xFFFFFFFFu, mx = 0, nc = 0;
        uint32_t *h = s_h[w];
        for (int i = 0; i < 4; ++i) h[lane * 4 + i] = 0;
        wave_lds_fence();
        for (uint32_t i = lane; i < n_win; i += 64) {
            const uint32_t x = v[i];
            sum += x; mn = min(mn, x); mx = max(mx, x); nc += x != 0;
            atomicAdd(&h[x >> 8], 1u);
        }
        wave_lds_fence();
        uint32_t rem = 0;
        const uint32_t hi = cov_select_bin(h, (n_win - 1) / 2, rem);
        wave_lds_fence();
        for (int i = 0; i < 4; ++i) h[lane * 4 + i] = 0;
        wave_lds_fence();
        for (uint32_t i = lane; i < n_win; i += 64) {
            const uint32_t x = v[i];
            if ((x >> 8) == hi) atomicAdd(&h[x & 255u], 1u);
        }
        wave_lds_fence();
        uint32_t rem2 = 0;
        const uint32_t lo = cov_select_bin(h, rem, rem2);
        res.sum = wave_sum64(sum); res.min = wave_min(mn); res.max = wave_max(mx); res.n_covered = wave_sum(nc);
        res.median = (hi << 8) | lo;
    }
    if (lane == 0) out[job.idx] = res;
}

__global__ __launch_bounds__(256) void edge_mult_kernel(MultDev m, const int64_t *ids, int64_t n, uint16_t *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (uint16_t)g_edge_mult(m, ids[i]);
}

// ---- read recruitment (mgta_reads_match_contigs): which reads share a (k+1)-mer with a set of contigs ------------------------------
// The contigs turn on the mark bit of every edge their windows find, as given and reverse-complemented; a read matches when the edge
// of one of its windows is marked.  Both passes are the walk above -- one index search, then one dependent line per window -- without
// multiplicities and without the per-window scratch.

// walk_contig over both strands of every contig (the jobs of cut_batch), marking
// counters: [0] queue head, [1] edges whose bit this launch turned on
__global__ __launch_bounds__(kCovThreads) void match_mark_kernel(GraphDev g, const uint8_t *sym, const CovJob *jobs, uint32_t n_jobs, uint32_t chunk, uint32_t *marks,
                                                                 unsigned long long *counters) {
    const int sub = threadIdx.x & 7;
    WalkCounts n;                                                         // (not reported)
    uint32_t marked = 0;
    for (;;) {
        const unsigned long long first = grp_next_chunk(&counters[0], chunk, sub);
        if (first >= n_jobs) break;
        const uint32_t j_end = (uint32_t)min((unsigned long long)n_jobs, first + chunk);
        for (uint32_t j = (uint32_t)first; j < j_end; ++j) {
            const CovJob job = jobs[j];
            walk_contig(g, sym + job.off, job.len, sub, n, [&](uint32_t, int64_t e) {
                if (e >= 0 && sub == 0 && mark_edge(marks, e)) ++marked;  // the lane that turns the edge's bit on counts the edge
            });
        }
    }
    const uint32_t m = wave_sum(marked);
    if (lane_id() == 0 && m) atomicAdd(&counters[1], (unsigned long long)m);
}

// The read walk, written out (walk.hpp says why), over the reads [0, n_reads): a group of 8 lanes owns a read and walks it in
// STORED order, words ascending -- as it is when stored as sequenced, with complemented bases, i.e. along its reverse complement,
// when stored reversed.  A read matches when the edge of one of its windows is marked: the marks hold both strands of every contig
// window, so that walk hits exactly when the read does, window for window.  count_all = 0: the walk of a read ends at its first hit.
// counters: [0] queue head, [1] windows found by a step, [2] index searches, [3] matched reads, [4] read windows
__global__ __launch_bounds__(kCovThreads) void match_walk_kernel(GraphDev g, const uint32_t *packed, const uint64_t *start, uint64_t n_reads, int reversed, uint32_t chunk,
                                                                 const uint32_t *marks, uint32_t *bits, uint32_t *hit_windows, int count_all,
                                                                 unsigned long long *counters) {
    __shared__ uint8_t s_seq[kCovGroups][kMatchMaxWindow];
    const int sub = threadIdx.x & 7;
    const int k = g.k;
    uint8_t *seq = s_seq[threadIdx.x >> 3];
    const uint32_t flip = reversed ? 3u : 0u;                             // base b -> symbol (b ^ flip) + 1: the complement when stored reversed
    uint32_t walked = 0, searched = 0, matched = 0;
    unsigned long long windows = 0;
    for (;;) {
        const unsigned long long first = grp_next_chunk(&counters[0], chunk, sub);
        if (first >= n_reads) break;
        const uint64_t r_end = min((unsigned long long)n_reads, first + chunk);
        for (uint64_t r = first; r < r_end; ++r) {
            const uint64_t s0 = start[r], len = start[r + 1] - s0;
            const uint64_t n_win = len > (uint64_t)k ? len - (uint64_t)k : 0;
            windows += n_win;
            int64_t e = -1;                                               // the edge of the window before, -1 = the walk has to start again
            LineR L{};
            uint32_t hits = 0, w = 0;
            for (uint64_t p = 0; p < n_win; ++p) {
                const uint64_t q = s0 + p + (uint64_t)k;                  // the window's last base
                if (p == 0 || (q & 15) == 0) w = packed[q >> 4];
                const int c = (int)packed_symbol(w, q, flip);
                if (e >= 0) {
                    e = cov_step(g, L, e, c, sub);
                    if (e >= 0) ++walked;
                } else {
                    // every lane writes all k + 1 symbols itself and reads back only what it wrote (the same values in every lane of the group)
                    for (int i = 0; i <= k; ++i) {
                        const uint64_t qi = s0 + p + (uint64_t)i;
                        seq[i] = (uint8_t)packed_symbol(packed[qi >> 4], qi, flip);
                    }
                    e = g_index_edge(g, seq);
                    ++searched;
                    if (e >= 0) L = grp_load_line(g, (uint64_t)e >> 6, sub);
                }
                if (e >= 0 && edge_marked(marks, e)) {
                    ++hits;
                    if (!count_all) break;
                }
            }
            if (sub == 0) {
                if (count_all) hit_windows[r] = hits;
                if (hits) {
                    atomicOr(&bits[r >> 5], 1u << (r & 31));
                    ++matched;
                }
            }
        }
    }
    const uint32_t wk = wave_sum(sub == 0 ? walked : 0u), sc = wave_sum(sub == 0 ? searched : 0u), mt = wave_sum(matched);
    const uint64_t wn = wave_sum64(sub == 0 ? windows : 0ull);
    if (lane_id() == 0) {
        if (wk) atomicAdd(&counters[1], (unsigned long long)wk);
        if (sc) atomicAdd(&counters[2], (unsigned long long)sc);
        if (mt) atomicAdd(&counters[3], (unsigned long long)mt);
        if (wn) atomicAdd(&counters[4], (unsigned long long)wn);
    }
}

// ---- window-shared coverage (mgta_contig_share_coverage): every edge's multiplicity split among the windows of the call on it -------
// Three phases.  (1) The walk above, once, leaving the edge id of every window of a batch (8 bytes, -1 = none) where the coverage
// call leaves the multiplicity.  (2) The ids of the batch go into an open-addressing table keyed by the edge id (linear probing, 64-bit
// compare-and-swap for the key, one 64-bit atomic add for the value: occurrences in the low word, the multiplicity -- added once, by the
// lane that created the key -- in the high word) and every window keeps its slot number, 4 bytes, for the whole call.  (3) When all
// batches are counted, one pass over the slot numbers: one 8-byte gather and one 32-bit division per window, one wave per contig.
// Slot 0 is never used by a key and stands for "no edge": its value stays 0.
//
// Redundant contigs put thousands of windows on one edge, all on one address.  So equal ids are added up inside a wave before the
// atomic: a wave of the count kernel owns 64 contigs that follow each other in the batch's job order (longest first, ties by number:
// copies and contigs of one length sit side by side) and visits them position by position, lane l holding window p of its contig;
// the lanes with equal ids elect the lowest one, which adds their number.  gfx950 has no match-any instruction: one ballot per
// distinct id of the step, 1 when the 64 ids agree, 64 when they all differ.

// `times` occurrences of edge e -> its slot (1 .. n_slots - 1); 0 and *full = 1 when the table has no room (it is sized so that it has)
__device__ __forceinline__ uint32_t share_table_add(const MultDev &m, unsigned long long *keys, unsigned long long *vals, uint64_t n_slots, uint64_t hmask, int64_t e,
                                                    uint32_t times, uint32_t &n_new, uint64_t &sum_mult, unsigned long long *full) {
    uint64_t slot = mix64_share((uint64_t)e) & hmask & (n_slots - 1);
    if (slot == 0) slot = 1;
    for (uint64_t tries = 0; tries < n_slots; ++tries) {
        unsigned long long key = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (key == kShareEmpty) {
            key = atomicCAS(&keys[slot], kShareEmpty, (unsigned long long)e);
            if (key == kShareEmpty) {                                     // this lane made the key: it brings the multiplicity, once
                const uint32_t mult = g_edge_mult(m, e);
                atomicAdd(&vals[slot], ((unsigned long long)mult << 32) | times);
                ++n_new;
                sum_mult += mult;
                return (uint32_t)slot;
            }
        }
        if (key == (unsigned long long)e) {
            atomicAdd(&vals[slot], (unsigned long long)times);
            return (uint32_t)slot;
        }
        slot = (slot + 1) & (n_slots - 1);
        if (slot == 0) slot = 1;
    }
    atomicExch(full, 1ull);
    return 0;
}

// counters: [3] keys made, [4] the sum of their multiplicities, [5] set when the table ran full
__global__ __launch_bounds__(256) void share_count_kernel(MultDev m, const CovJob *jobs, uint32_t n_jobs, int k, const int64_t *ids, uint64_t win_done, uint32_t *slots,
                                                          unsigned long long *keys, unsigned long long *vals, uint64_t n_slots, uint64_t hmask,
                                                          unsigned long long *counters) {
    const int lane = lane_id();
    const uint32_t j = blockIdx.x * 64 + (uint32_t)lane;
    uint32_t n_win = 0;
    uint64_t base = 0;
    if (j < n_jobs) {
        const CovJob job = jobs[j];
        n_win = job.len > (uint32_t)k ? job.len - (uint32_t)k : 0;
        base = job.win_base;
    }
    const uint64_t longest = wave_max(n_win);
    uint32_t n_new = 0;
    uint64_t sum_mult = 0;
    // the four waves of a workgroup take turns of 64 positions; every lane stays to the end (the shuffle below reads any lane)
    for (uint64_t p0 = ((uint64_t)blockIdx.y * 4 + (uint64_t)wave_id()) * 64; p0 < longest; p0 += (uint64_t)gridDim.y * 256) {
        const uint64_t p1 = min(longest, p0 + 64);
        for (uint64_t p = p0; p < p1; ++p) {
            const bool in = p < n_win;
            const int64_t e = in ? ids[base + p] : -1;
            int leader = lane;
            uint32_t times = 1;
            uint64_t todo = __ballot(e >= 0);
            while (todo) {                                                // one turn per distinct id among the 64
                const int src = __ffsll((long long)todo) - 1;
                const int64_t e0 = wave_read64(e, src);
                const uint64_t same = __ballot(e == e0);
                if (e == e0) { leader = src; times = (uint32_t)__popcll(same); }
                todo &= ~same;
            }
            uint32_t slot = 0;
            if (e >= 0 && leader == lane) slot = share_table_add(m, keys, vals, n_slots, hmask, e, times, n_new, sum_mult, &counters[5]);
            slot = __shfl(slot, leader, 64);
            if (in) slots[win_done + base + p] = slot;
        }
    }
    n_new = wave_sum(n_new);
    sum_mult = wave_sum64(sum_mult);
    if (lane == 0) {
        if (n_new) atomicAdd(&counters[3], (unsigned long long)n_new);
        if (sum_mult) atomicAdd(&counters[4], (unsigned long long)sum_mult);
    }
}

// One wave per contig over the slot numbers of its windows, when every batch is counted: one 8-byte gather (occurrences low,
// multiplicity high; slot 0 = no edge = 0) and ONE 32-bit division per window -- mult <= 65535, so mult << 16 fits 32 bits and
// floor(mult * 65536 / share) is that quotient exactly.  The mass is an integer sum: no order matters.
__global__ __launch_bounds__(256) void share_mass_kernel(const uint64_t *woff, const uint32_t *lens, uint32_t n, const uint32_t *slots, const unsigned long long *vals,
                                                         mgta_contig_share *out, uint32_t *pw_share, uint16_t *pw_mult) {
    const int lane = lane_id();
    const uint32_t i = blockIdx.x * 4 + (uint32_t)wave_id();
    if (i >= n) return;                                                   // (whole waves leave)
    const uint64_t b = woff[i];
    const uint32_t n_win = (uint32_t)(woff[i + 1] - b);
    uint64_t mass = 0;
    uint32_t nc = 0, nu = 0, mx = 0;
    for (uint32_t q = lane; q < n_win; q += 64) {
        const unsigned long long v = vals[slots[b + q]];
        const uint32_t share = (uint32_t)v, mult = (uint32_t)(v >> 32);
        if (mult) {
            mass += (mult << 16) / share;
            ++nc;
            nu += share == 1u;
            mx = max(mx, share);
        }
        if (pw_share) pw_share[b + q] = share;
        if (pw_mult) pw_mult[b + q] = (uint16_t)mult;
    }
    mgta_contig_share res;
    res.mass = wave_sum64(mass); res.len = lens[i]; res.n_windows = n_win; res.n_covered = wave_sum(nc); res.n_unique = wave_sum(nu);
    res.max_share = wave_max(mx); res.reserved_ = 0;
    if (lane == 0) out[i] = res;
}

// ---- per-library coverage (mgta_contig_sample_coverage): the read windows of every library on the windows of a set of contigs --------
// The multiplicities of the graph are pooled over the read set, so this count comes from the reads.  Four phases.
// (1) share_walk_kernel over BOTH strands of every contig of a batch (the reverse complements lie mirrored behind the symbols, as for
// the read recruitment), then the edge ids go into an open-addressing table keyed by the edge id: 8 bytes of key, the share (the
// windows AS GIVEN on the key; a reverse-complement window adds 0) and, later, the key's dense number.  The lane that makes a key
// turns the edge's mark bit on.  Every window keeps two slot numbers for the whole call: that of its own edge and that of the edge
// of its reverse complement (0 = none).  (2) When all batches are in, the keys are numbered 1 .. n_keys and a row of n_libs 64-bit
// counts per key is zeroed (row 0 stays zero: "no edge").  (3) The read scan: match_walk_kernel's walk with count_all; a window whose
// edge is marked probes the table and adds 1 to counts[key][library] -- ONE add per read window, so a window that is its own reverse
// complement (one key, two equal slot numbers) is counted once.  (4) count(w, s) = counts[own][s] + counts[partner][s] where the two
// rows differ, divided by the share: one wave per contig.
//
// A read that occurs hundreds of times sits side by side in the read queue, so the 8 groups of a wave walk copies in step and hit the
// same (key, library) together: the group leaders with equal addresses elect the lowest lane, which adds their number.

constexpr int kSampleMaxLibs = 256;

// match_walk_kernel's walk over the reads [0, n_reads), every window counted.  Read r belongs to the library s with
// lib_end[s - 1] <= r < lib_end[s]; the boundaries sit in LDS, s is found by bisection for the first read of a queue chunk and moves
// on with the reads of the chunk (a boundary may fall anywhere inside it, and empty libraries are stepped over).
// counters: [0] queue head, [1] windows found by a step, [2] index searches, [3] hit windows, [4] read windows
__global__ __launch_bounds__(kCovThreads) void sample_scan_kernel(GraphDev g, const uint32_t *packed, const uint64_t *start, uint64_t n_reads, int reversed, uint32_t chunk,
                                                                  const uint32_t *marks, SampleTable t, unsigned long long *counts, const uint64_t *lib_end, int n_libs,
                                                                  unsigned long long *lib_hits, unsigned long long *counters) {
    __shared__ uint8_t s_seq[kCovGroups][kMatchMaxWindow];
    __shared__ uint64_t s_end[kSampleMaxLibs];
    __shared__ unsigned long long s_hits[kSampleMaxLibs];
    for (int i = threadIdx.x; i < n_libs; i += kCovThreads) { s_end[i] = lib_end[i]; s_hits[i] = 0; }
    __syncthreads();
    const int sub = threadIdx.x & 7, lane = lane_id();
    const int k = g.k;
    uint8_t *seq = s_seq[threadIdx.x >> 3];
    const uint32_t flip = reversed ? 3u : 0u;                             // base b -> symbol (b ^ flip) + 1: the complement when stored reversed
    uint32_t walked = 0, searched = 0;
    unsigned long long windows = 0, all_hits = 0;
    for (;;) {
        const unsigned long long first = grp_next_chunk(&counters[0], chunk, sub);
        if (first >= n_reads) break;
        const uint64_t r_end = min((unsigned long long)n_reads, first + chunk);
        int s = 0;
        for (int hi = n_libs - 1; s < hi;) {                              // the first library that ends behind read `first` (first < n_reads = the last end)
            const int mid = (s + hi) >> 1;
            if (s_end[mid] > first) hi = mid; else s = mid + 1;
        }
        for (uint64_t r = first; r < r_end; ++r) {
            while (s + 1 < n_libs && s_end[s] <= r) ++s;
            const uint64_t s0 = start[r], len = start[r + 1] - s0;
            const uint64_t n_win = len > (uint64_t)k ? len - (uint64_t)k : 0;
            windows += n_win;
            int64_t e = -1;                                               // the edge of the window before, -1 = the walk has to start again
            LineR L{};
            uint32_t hits = 0, w = 0;
            for (uint64_t p = 0; p < n_win; ++p) {
                const uint64_t q = s0 + p + (uint64_t)k;                  // the window's last base
                if (p == 0 || (q & 15) == 0) w = packed[q >> 4];
                const int c = (int)packed_symbol(w, q, flip);
                if (e >= 0) {
                    e = cov_step(g, L, e, c, sub);
                    if (e >= 0) ++walked;
                } else {
                    // every lane writes all k + 1 symbols itself and reads back only what it wrote (the same values in every lane of the group)
                    for (int i = 0; i <= k; ++i) {
                        const uint64_t qi = s0 + p + (uint64_t)i;
                        seq[i] = (uint8_t)packed_symbol(packed[qi >> 4], qi, flip);
                    }
                    e = g_index_edge(g, seq);
                    ++searched;
                    if (e >= 0) L = grp_load_line(g, (uint64_t)e >> 6, sub);
                }
                if (e >= 0 && edge_marked(marks, e)) {       // the one-bit filter in front of the table
                    ++hits;
                    if (sub == 0) {
                        const uint32_t slot = sample_table_find(t, e);
                        const int64_t at = slot ? (int64_t)((uint64_t)t.dense[slot] * (uint64_t)n_libs + (uint64_t)s) : -1;
                        // the group leaders that are here together: equal addresses elect the lowest lane
                        int leader = lane;
                        uint32_t times = 1;
                        uint64_t todo = __ballot(1);
                        while (todo) {
                            const int src = __ffsll((long long)todo) - 1;
                            const int64_t a0 = wave_read64(at, src);
                            const uint64_t same = __ballot(at == a0);
                            if (at == a0) { leader = src; times = (uint32_t)__popcll(same); }
                            todo &= ~same;
                        }
                        if (leader == lane && at >= 0) atomicAdd(&counts[at], (unsigned long long)times);
                    }
                }
            }
            if (sub == 0 && hits) {
                atomicAdd(&s_hits[s], (unsigned long long)hits);
                all_hits += hits;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_libs; i += kCovThreads)
        if (s_hits[i]) atomicAdd(&lib_hits[i], s_hits[i]);
    const uint32_t wk = wave_sum(sub == 0 ? walked : 0u), sc = wave_sum(sub == 0 ? searched : 0u);
    const uint64_t wn = wave_sum64(sub == 0 ? windows : 0ull), ht = wave_sum64(all_hits);
    if (lane == 0) {
        if (wk) atomicAdd(&counters[1], (unsigned long long)wk);
        if (sc) atomicAdd(&counters[2], (unsigned long long)sc);
        if (ht) atomicAdd(&counters[3], (unsigned long long)ht);
        if (wn) atomicAdd(&counters[4], (unsigned long long)wn);
    }
}

// floor(c * 65536 / share) without a 128-bit product: c = q * share + r gives q * 65536 + floor(r * 65536 / share), and r < 2^32
__device__ __forceinline__ uint64_t sample_q16(uint64_t c, uint32_t share) {
    if (c < (1ull << 48)) return (c << 16) / share;
    const uint64_t q = c / share, r = c % share;
    return (q << 16) + (r << 16) / share;
}

// One wave per contig, a lane per window, the libraries inside: per window two slot numbers -> two rows of counts, per library one
// gather from each row and one division.  The per-library sums are kept in LDS (n_libs 64-bit words per wave); lane l starts at
// library l mod n_libs, so the lanes of one add are on different words wherever n_libs allows.  Integer sums: no order matters.
__global__ __launch_bounds__(256) void sample_mass_kernel(const uint64_t *woff, const uint32_t *lens, uint32_t n, const uint32_t *slots_own, const uint32_t *slots_rc,
                                                          SampleTable t, const unsigned long long *counts, int n_libs, uint64_t *mass_out, mgta_contig_share *out,
                                                          uint64_t *pw_count, uint32_t *pw_share) {
    __shared__ unsigned long long s_mass[4][kSampleMaxLibs];
    const int lane = lane_id();
    const uint32_t i = blockIdx.x * 4 + (uint32_t)wave_id();
    if (i >= n) return;                                                   // (whole waves leave; the rest use wave-level ordering only)
    unsigned long long *acc = s_mass[wave_id()];
    for (int s = lane; s < n_libs; s += 64) acc[s] = 0;
    wave_lds_fence();
    const uint64_t b = woff[i];
    const uint32_t n_win = (uint32_t)(woff[i + 1] - b);
    const int s_first = lane % n_libs;
    uint64_t mass = 0;
    uint32_t nc = 0, nu = 0, mx = 0;
    for (uint32_t q = lane; q < n_win; q += 64) {
        const uint32_t so = slots_own[b + q], sr = slots_rc[b + q];
        uint32_t share = 0, d_own = 0, d_rc = 0;
        if (so) {                                                         // a window without an edge counts nothing, whatever its reverse complement finds
            share = t.share[so];
            d_own = t.dense[so];
            d_rc = sr && sr != so ? t.dense[sr] : 0u;                     // its own reverse complement: one row, counted once
        }
        const unsigned long long *row_own = counts + (uint64_t)d_own * (uint64_t)n_libs, *row_rc = counts + (uint64_t)d_rc * (uint64_t)n_libs;
        bool any = false;
        int s = s_first;
        for (int j = 0; j < n_libs; ++j) {
            const uint64_t c = so ? row_own[s] + row_rc[s] : 0ull;
            if (pw_count) pw_count[(b + q) * (uint64_t)n_libs + (uint64_t)s] = c;
            if (c) {
                const uint64_t m = sample_q16(c, share);
                atomicAdd(&acc[s], (unsigned long long)m);
                mass += m;
                any = true;
            }
            if (++s == n_libs) s = 0;
        }
        if (any) {
            ++nc;
            nu += share == 1u;
            mx = max(mx, share);
        }
        if (pw_share) pw_share[b + q] = share;
    }
    mgta_contig_share res;
    res.mass = wave_sum64(mass); res.len = lens[i]; res.n_windows = n_win; res.n_covered = wave_sum(nc); res.n_unique = wave_sum(nu);
    res.max_share = wave_max(mx); res.reserved_ = 0;
    if (lane == 0 && out) out[i] = res;
    wave_lds_fence();
    for (int s = lane; s < n_libs; s += 64) mass_out[(uint64_t)i * (uint64_t)n_libs + (uint64_t)s] = acc[s];
}

}  // namespace
}  // namespace mgta

using namespace mgta;

extern "C" {

int mgta_sdbg_edge_multiplicity(mgta_sdbg *g, const int64_t *edge_ids, int64_t n, uint16_t *mult) {
    if (!g || n < 0 || (n > 0 && (!edge_ids || !mult))) { set_error("mgta_sdbg_edge_multiplicity: bad argument"); return MGTA_EINVAL; }
    if (!g->has_mult) { set_error("mgta_sdbg_edge_multiplicity: the graph was loaded without multiplicities (mgta_ctx_keep_multiplicity)"); return MGTA_EINVAL; }
    for (int64_t i = 0; i < n; ++i)
        if (edge_ids[i] < 0 || edge_ids[i] >= g->dev.size) { set_error("mgta_sdbg_edge_multiplicity: edge id %lld out of range", (long long)edge_ids[i]); return MGTA_EINVAL; }
    if (n == 0) return MGTA_OK;
    return guarded("mgta_sdbg_edge_multiplicity", [&]() {
        mgta_ctx *ctx = g->ctx;
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        DevBuf d_e, d_m;
        d_e.alloc((size_t)n * 8); d_m.alloc((size_t)n * 2);
        MGTA_HIP_CHECK(hipMemcpyAsync(d_e.p, edge_ids, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(edge_mult_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, g->mult, d_e.as<int64_t>(), n, d_m.as<uint16_t>());
        MGTA_HIP_CHECK(hipGetLastError());
        MGTA_HIP_CHECK(hipMemcpyAsync(mult, d_m.p, (size_t)n * 2, hipMemcpyDeviceToHost, ctx->stream));
        MGTA_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return MGTA_OK;
    });
}

int mgta_contig_coverage(mgta_sdbg *g, const char *seqs, const uint64_t *offsets, int64_t n, mgta_contig_cov *per_contig, uint16_t *per_window,
                         int64_t *abundance, mgta_coverage_stats *stats) {
    if (!g || n < 0 || n > 0xFFFFFFF0ll || (n > 0 && (!offsets || !per_contig))) { set_error("mgta_contig_coverage: bad argument"); return MGTA_EINVAL; }
    if (!g->has_mult) { set_error("mgta_contig_coverage: the graph was loaded without multiplicities (mgta_ctx_keep_multiplicity)"); return MGTA_EINVAL; }
    const uint64_t k = (uint64_t)g->dev.k;
    if (!check_contigs("mgta_contig_coverage", seqs, offsets, n, k, kMaxContigLetters, 0, nullptr, nullptr)) return MGTA_EINVAL;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (abundance) memset(abundance, 0, 65536 * sizeof(int64_t));
    if (n == 0) return MGTA_OK;
    return guarded("mgta_contig_coverage", [&]() {
        mgta_ctx *ctx = g->ctx;
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        Timer t_walk(st), t_stats(st);
        const uint64_t cap = ctx->coverage_batch_windows ? ctx->coverage_batch_windows : 1ull << 29;   // windows per batch: 1 GB of per-window scratch
        DevBuf d_cnt, d_abund, d_sym, d_jobs, d_out;
        d_cnt.alloc(64);
        MGTA_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 64, st));
        uint32_t *d_marks = nullptr;
        if (abundance) {
            d_marks = marks_reset(g, st);
            d_abund.alloc(65536 * 8);
            MGTA_HIP_CHECK(hipMemsetAsync(d_abund.p, 0, 65536 * 8, st));
        }
        const int walk_per_cu = queue_per_cu(cov_walk_kernel);
        std::vector<CovJob> jobs;
        uint64_t win_done = 0, n_win = 0;
        double ms_walk = 0, ms_stats = 0;
        int64_t n_batches = 0;
        for (int64_t c0 = 0, c1; c0 < n; c0 = c1) {
            c1 = cut_batch(offsets, n, k, c0, cap, false, jobs, &n_win);
            const uint32_t nj = (uint32_t)jobs.size();
            const uint64_t n_bytes = offsets[c1] - offsets[c0];
            if (d_sym.bytes < n_bytes + 16) d_sym.alloc(n_bytes + 16, &ctx->live_bytes, &ctx->peak_bytes);
            if (d_jobs.bytes < (size_t)nj * sizeof(CovJob)) d_jobs.alloc((size_t)nj * sizeof(CovJob), &ctx->live_bytes, &ctx->peak_bytes);
            if (d_out.bytes < (size_t)nj * sizeof(mgta_contig_cov)) d_out.alloc((size_t)nj * sizeof(mgta_contig_cov), &ctx->live_bytes, &ctx->peak_bytes);
            uint16_t *d_pw = window_scratch(ctx, n_win * 2 + 64);
            MGTA_HIP_CHECK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)nj * sizeof(CovJob), hipMemcpyHostToDevice, st));
            MGTA_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 8, st));            // the queue head
            stage_symbols(ctx, st, d_sym, seqs + offsets[c0], n_bytes, false);
            const QueueLaunch q = queue_launch(ctx, walk_per_cu, nj, 64, 4);
            t_walk.start();
            if (g->dev.size > 0)
                hipLaunchKernelGGL(cov_walk_kernel, dim3(q.blocks), dim3(kCovThreads), 0, st, g->dev, g->mult, d_sym.as<uint8_t>(), d_jobs.as<CovJob>(), nj, q.chunk, d_pw,
                                   d_marks, d_abund.as<unsigned long long>(), d_cnt.as<unsigned long long>());
            else
                MGTA_HIP_CHECK(hipMemsetAsync(d_pw, 0, n_win * 2 + 64, st));
            MGTA_HIP_CHECK(hipGetLastError());
            t_walk.end();
            t_stats.start();
            hipLaunchKernelGGL(cov_stats_kernel, dim3((nj + 3) / 4), dim3(256), 0, st, d_jobs.as<CovJob>(), nj, (int)k, d_pw, d_out.as<mgta_contig_cov>());
            MGTA_HIP_CHECK(hipGetLastError());
            t_stats.end();
            MGTA_HIP_CHECK(hipMemcpyAsync(per_contig + c0, d_out.p, (size_t)nj * sizeof(mgta_contig_cov), hipMemcpyDeviceToHost, st));
            if (per_window && n_win) MGTA_HIP_CHECK(hipMemcpyAsync(per_window + win_done, d_pw, n_win * 2, hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipStreamSynchronize(st));                     // (jobs and the device buffers serve the next batch)
            ms_walk += t_walk.ms();
            ms_stats += t_stats.ms();
            win_done += n_win;
            ++n_batches;
        }
        unsigned long long cnt[3] = {0, 0, 0};
        MGTA_HIP_CHECK(hipMemcpyAsync(cnt, d_cnt.p, 24, hipMemcpyDeviceToHost, st));
        if (abundance) MGTA_HIP_CHECK(hipMemcpyAsync(abundance, d_abund.p, 65536 * 8, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        if (stats) {
            stats->n_contigs = n; stats->n_windows = (int64_t)win_done; stats->n_walked = (int64_t)cnt[1]; stats->n_index_searches = (int64_t)cnt[2];
            stats->groups_per_cu = (int64_t)walk_per_cu * kCovGroups;
            stats->n_batches = n_batches; stats->ms_walk = ms_walk; stats->ms_kernel = ms_walk + ms_stats;
        }
        return MGTA_OK;
    });
}

int mgta_reads_match_contigs(mgta_sdbg *g, const mgta_reads *reads, int reads_reversed, uint64_t n_short_reads, const char *seqs, const uint64_t *offsets, int64_t n,
                             uint64_t *match_bits, uint32_t *hit_windows, mgta_match_stats *stats) {
    if (!g || !reads) { set_error("mgta_reads_match_contigs: the graph and the reads must not be NULL"); return MGTA_EINVAL; }
    if (g->ctx != reads->ctx) { set_error("mgta_reads_match_contigs: the graph and the reads belong to different contexts"); return MGTA_EINVAL; }
    if (n_short_reads > reads->n_reads) {
        set_error("mgta_reads_match_contigs: n_short_reads = %llu, the library holds %llu reads", (unsigned long long)n_short_reads, (unsigned long long)reads->n_reads);
        return MGTA_EINVAL;
    }
    if (n_short_reads > 0 && !match_bits) { set_error("mgta_reads_match_contigs: match_bits must not be NULL"); return MGTA_EINVAL; }
    if (n < 0 || n > 0x7FFFFFF0ll || (n > 0 && !offsets)) { set_error("mgta_reads_match_contigs: bad contig count or offsets"); return MGTA_EINVAL; }
    const uint64_t k = (uint64_t)g->dev.k;
    uint64_t n_contig_win = 0;
    if (!check_contigs("mgta_reads_match_contigs", seqs, offsets, n, k, kMaxContigLetters, 0, &n_contig_win, nullptr)) return MGTA_EINVAL;
    if (g->dev.k + 1 > kMatchMaxWindow) { set_error("mgta_reads_match_contigs: k = %d (k + 1 <= %d is supported)", g->dev.k, kMatchMaxWindow); return MGTA_EINVAL; }
    const uint64_t n_bit_words = (n_short_reads + 63) / 64;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_bit_words) memset(match_bits, 0, n_bit_words * 8);
    if (hit_windows && n_short_reads) memset(hit_windows, 0, n_short_reads * 4);
    if (n == 0 || n_short_reads == 0) return MGTA_OK;
    return guarded("mgta_reads_match_contigs", [&]() {
        mgta_ctx *ctx = g->ctx;
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        // the two strands of every contig as one batch
        std::vector<CovJob> jobs;
        uint64_t n_win = 0;
        cut_batch(offsets, n, k, 0, ~0ull, true, jobs, &n_win);
        const uint32_t nj = (uint32_t)jobs.size();
        const uint64_t n_sym = offsets[n] - offsets[0];
        uint32_t *d_marks = marks_reset(g, st);
        DevBuf d_cnt, d_sym, d_jobs, d_bits, d_hits;
        d_cnt.alloc(128);
        d_sym.alloc(2 * n_sym + 16, &ctx->live_bytes, &ctx->peak_bytes);
        d_jobs.alloc((size_t)nj * sizeof(CovJob), &ctx->live_bytes, &ctx->peak_bytes);
        d_bits.alloc(n_bit_words * 8, &ctx->live_bytes, &ctx->peak_bytes);
        if (hit_windows) d_hits.alloc(n_short_reads * 4, &ctx->live_bytes, &ctx->peak_bytes);
        MGTA_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 128, st));
        MGTA_HIP_CHECK(hipMemsetAsync(d_bits.p, 0, n_bit_words * 8, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)nj * sizeof(CovJob), hipMemcpyHostToDevice, st));
        unsigned long long *cnt_mark = d_cnt.as<unsigned long long>(), *cnt_walk = cnt_mark + 8;
        const QueueLaunch q_mark = queue_launch(ctx, queue_per_cu(match_mark_kernel), nj, 64, 4),
                          q_walk = queue_launch(ctx, queue_per_cu(match_walk_kernel), n_short_reads, 256, 16);
        Timer t_mark(st), t_walk(st);
        stage_symbols(ctx, st, d_sym, seqs + offsets[0], n_sym, true, &t_mark);   // (t_mark starts behind the upload)
        hipLaunchKernelGGL(match_mark_kernel, dim3(q_mark.blocks), dim3(kCovThreads), 0, st, g->dev, d_sym.as<uint8_t>(), d_jobs.as<CovJob>(), nj, q_mark.chunk, d_marks,
                           cnt_mark);
        MGTA_HIP_CHECK(hipGetLastError());
        t_mark.end();
        t_walk.start();
        hipLaunchKernelGGL(match_walk_kernel, dim3(q_walk.blocks), dim3(kCovThreads), 0, st, g->dev, reads->d_packed, reads->d_start, n_short_reads, reads_reversed ? 1 : 0,
                           q_walk.chunk, d_marks, d_bits.as<uint32_t>(), d_hits.as<uint32_t>(), hit_windows ? 1 : 0, cnt_walk);
        MGTA_HIP_CHECK(hipGetLastError());
        t_walk.end();
        unsigned long long cnt[16] = {0};
        MGTA_HIP_CHECK(hipMemcpyAsync(cnt, d_cnt.p, 128, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(match_bits, d_bits.p, n_bit_words * 8, hipMemcpyDeviceToHost, st));
        if (hit_windows) MGTA_HIP_CHECK(hipMemcpyAsync(hit_windows, d_hits.p, n_short_reads * 4, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        if (stats) {
            stats->n_contigs = n; stats->n_contig_windows = (int64_t)n_contig_win; stats->n_marked_edges = (int64_t)cnt[1];
            stats->n_reads = (int64_t)n_short_reads; stats->n_read_windows = (int64_t)cnt[12];
            stats->n_walked = (int64_t)cnt[9]; stats->n_index_searches = (int64_t)cnt[10]; stats->n_matched_reads = (int64_t)cnt[11];
            stats->groups_per_cu = q_walk.groups_per_cu();
            stats->ms_mark = t_mark.ms(); stats->ms_walk = t_walk.ms();
        }
        return MGTA_OK;
    });
}

int mgta_ctx_set_share_hash_bits(mgta_ctx *ctx, int bits) {
    if (!ctx) { set_error("mgta_ctx_set_share_hash_bits: ctx must not be NULL"); return MGTA_EINVAL; }
    if (bits < 1 || bits > 64) { set_error("mgta_ctx_set_share_hash_bits: bits = %d (1 .. 64)", bits); return MGTA_EINVAL; }
    ctx->share_hash_bits = bits;
    return MGTA_OK;
}

int mgta_contig_share_coverage(mgta_sdbg *g, const char *seqs, const uint64_t *offsets, int64_t n, mgta_contig_share *per_contig, uint32_t *per_window_share,
                               uint16_t *per_window, mgta_share_stats *stats) {
    if (!g || n < 0 || (n > 0 && (!offsets || !per_contig))) { set_error("mgta_contig_share_coverage: bad argument"); return MGTA_EINVAL; }
    if (n > 0x7FFFFFFFll) { set_error("mgta_contig_share_coverage: %lld contigs (n < 2^31 is supported)", (long long)n); return MGTA_EINVAL; }
    if (!g->has_mult) { set_error("mgta_contig_share_coverage: the graph was loaded without multiplicities (mgta_ctx_keep_multiplicity)"); return MGTA_EINVAL; }
    const uint64_t k = (uint64_t)g->dev.k;
    uint64_t total_win = 0;
    if (!check_contigs("mgta_contig_share_coverage", seqs, offsets, n, k, kMaxContigLetters, kMaxCallWindows, &total_win, nullptr)) return MGTA_EINVAL;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return MGTA_OK;
    return guarded("mgta_contig_share_coverage", [&]() {
        mgta_ctx *ctx = g->ctx;
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        Timer t_walk(st), t_count(st), t_share(st);
        const uint64_t cap = ctx->coverage_batch_windows ? ctx->coverage_batch_windows : 1ull << 29;   // windows per batch: 4 GB of edge ids
        // the table is sized by the windows of the call -- or by the graph where that has fewer edges than the call has windows
        const uint64_t n_slots = table_slots(std::min<uint64_t>(total_win, (uint64_t)std::max<int64_t>(g->dev.size, 0))), hmask = table_hmask(ctx);
        DevBuf d_cnt, d_sym, d_jobs, d_keys, d_vals, d_slots, d_woff, d_lens, d_out, d_pws, d_pwm;
        d_cnt.alloc(64);
        MGTA_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 64, st));
        d_keys.alloc(n_slots * 8, &ctx->live_bytes, &ctx->peak_bytes);
        d_vals.alloc(n_slots * 8, &ctx->live_bytes, &ctx->peak_bytes);
        d_slots.alloc(total_win * 4 + 16, &ctx->live_bytes, &ctx->peak_bytes);
        MGTA_HIP_CHECK(hipMemsetAsync(d_keys.p, 0xFF, n_slots * 8, st));
        MGTA_HIP_CHECK(hipMemsetAsync(d_vals.p, 0, n_slots * 8, st));
        const int walk_per_cu = queue_per_cu(share_walk_kernel);
        std::vector<CovJob> jobs;
        uint64_t win_done = 0, n_win = 0;
        double ms_walk = 0, ms_count = 0;
        int64_t n_batches = 0;
        for (int64_t c0 = 0, c1; c0 < n; c0 = c1) {
            c1 = cut_batch(offsets, n, k, c0, cap, false, jobs, &n_win);
            const uint32_t nj = (uint32_t)jobs.size();
            const uint64_t batch_longest = contig_windows(jobs[0].len, k);
            const uint64_t n_bytes = offsets[c1] - offsets[c0];
            if (d_sym.bytes < n_bytes + 16) d_sym.alloc(n_bytes + 16, &ctx->live_bytes, &ctx->peak_bytes);
            if (d_jobs.bytes < (size_t)nj * sizeof(CovJob)) d_jobs.alloc((size_t)nj * sizeof(CovJob), &ctx->live_bytes, &ctx->peak_bytes);
            int64_t *d_ids = reinterpret_cast<int64_t *>(window_scratch(ctx, n_win * 8 + 64));
            MGTA_HIP_CHECK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)nj * sizeof(CovJob), hipMemcpyHostToDevice, st));
            MGTA_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 8, st));            // the queue head
            stage_symbols(ctx, st, d_sym, seqs + offsets[c0], n_bytes, false);
            const QueueLaunch q = queue_launch(ctx, walk_per_cu, nj, 64, 4);
            t_walk.start();
            if (g->dev.size > 0)
                hipLaunchKernelGGL(share_walk_kernel, dim3(q.blocks), dim3(kCovThreads), 0, st, g->dev, d_sym.as<uint8_t>(), d_jobs.as<CovJob>(), nj, q.chunk, d_ids,
                                   d_cnt.as<unsigned long long>());
            else
                MGTA_HIP_CHECK(hipMemsetAsync(d_ids, 0xFF, n_win * 8 + 64, st));   // no edge anywhere
            MGTA_HIP_CHECK(hipGetLastError());
            t_walk.end();
            t_count.start();
            if (batch_longest) {
                const unsigned gy = (unsigned)std::min<uint64_t>((batch_longest + 255) / 256, 1024);
                hipLaunchKernelGGL(share_count_kernel, dim3((nj + 63) / 64, gy), dim3(256), 0, st, g->mult, d_jobs.as<CovJob>(), nj, (int)k, d_ids, win_done,
                                   d_slots.as<uint32_t>(), d_keys.as<unsigned long long>(), d_vals.as<unsigned long long>(), n_slots, hmask,
                                   d_cnt.as<unsigned long long>());
            }
            MGTA_HIP_CHECK(hipGetLastError());
            t_count.end();
            MGTA_HIP_CHECK(hipStreamSynchronize(st));                     // (jobs and the device buffers serve the next batch)
            ms_walk += t_walk.ms();
            ms_count += t_count.ms();
            win_done += n_win;
            ++n_batches;
        }
        unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
        MGTA_HIP_CHECK(hipMemcpyAsync(cnt, d_cnt.p, 48, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        if (cnt[5]) { set_error("mgta_contig_share_coverage: the count table of %llu slots ran full", (unsigned long long)n_slots); return MGTA_EHIP; }
        // every batch is counted: the shares are final.  The batch buffers make room for the outputs.
        d_sym.release(); d_jobs.release();
        std::vector<uint32_t> lens;
        const std::vector<uint64_t> woff = window_offsets(offsets, n, k, &lens);
        d_woff.alloc(((size_t)n + 1) * 8, &ctx->live_bytes, &ctx->peak_bytes);
        d_lens.alloc((size_t)n * 4, &ctx->live_bytes, &ctx->peak_bytes);
        d_out.alloc((size_t)n * sizeof(mgta_contig_share), &ctx->live_bytes, &ctx->peak_bytes);
        if (per_window_share && total_win) d_pws.alloc(total_win * 4, &ctx->live_bytes, &ctx->peak_bytes);
        if (per_window && total_win) d_pwm.alloc(total_win * 2, &ctx->live_bytes, &ctx->peak_bytes);
        MGTA_HIP_CHECK(hipMemcpyAsync(d_woff.p, woff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_lens.p, lens.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        t_share.start();
        hipLaunchKernelGGL(share_mass_kernel, dim3((unsigned)(((uint64_t)n + 3) / 4)), dim3(256), 0, st, d_woff.as<uint64_t>(), d_lens.as<uint32_t>(), (uint32_t)n,
                           d_slots.as<uint32_t>(), d_vals.as<unsigned long long>(), d_out.as<mgta_contig_share>(), d_pws.as<uint32_t>(), d_pwm.as<uint16_t>());
        MGTA_HIP_CHECK(hipGetLastError());
        t_share.end();
        MGTA_HIP_CHECK(hipMemcpyAsync(per_contig, d_out.p, (size_t)n * sizeof(mgta_contig_share), hipMemcpyDeviceToHost, st));
        if (d_pws.p) MGTA_HIP_CHECK(hipMemcpyAsync(per_window_share, d_pws.p, total_win * 4, hipMemcpyDeviceToHost, st));
        if (d_pwm.p) MGTA_HIP_CHECK(hipMemcpyAsync(per_window, d_pwm.p, total_win * 2, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        if (stats) {
            uint64_t mass = 0, covered = 0;
            for (int64_t i = 0; i < n; ++i) { mass += per_contig[i].mass; covered += per_contig[i].n_covered; }
            stats->n_contigs = n; stats->n_windows = (int64_t)total_win; stats->n_walked = (int64_t)cnt[1]; stats->n_index_searches = (int64_t)cnt[2];
            stats->n_batches = n_batches; stats->n_covered = (int64_t)covered; stats->n_distinct_edges = (int64_t)cnt[3]; stats->total_mult = cnt[4];
            stats->total_mass = mass; stats->table_slots = n_slots; stats->table_bytes = n_slots * 16; stats->window_bytes = total_win * 4;
            stats->ms_walk = ms_walk; stats->ms_count = ms_count; stats->ms_share = t_share.ms(); stats->ms_total = ms_walk + ms_count + stats->ms_share;
        }
        return MGTA_OK;
    });
}

int mgta_contig_sample_coverage(mgta_sdbg *g, const mgta_reads *reads, int reads_reversed, const uint64_t *lib_end, int n_libs, const char *seqs, const uint64_t *offsets,
                                int64_t n, uint64_t *mass, mgta_contig_share *per_contig, uint64_t *per_window_count, uint32_t *per_window_share,
                                uint64_t *lib_hit_windows, mgta_sample_cov_stats *stats) {
    if (!g || !reads) { set_error("mgta_contig_sample_coverage: the graph and the reads must not be NULL"); return MGTA_EINVAL; }
    if (g->ctx != reads->ctx) { set_error("mgta_contig_sample_coverage: the graph and the reads belong to different contexts"); return MGTA_EINVAL; }
    if (n_libs < 1 || n_libs > kSampleMaxLibs) { set_error("mgta_contig_sample_coverage: n_libs = %d (1 .. %d libraries are supported)", n_libs, kSampleMaxLibs); return MGTA_EINVAL; }
    if (!lib_end || !mass) { set_error("mgta_contig_sample_coverage: lib_end and mass must not be NULL"); return MGTA_EINVAL; }
    for (int s = 1; s < n_libs; ++s)
        if (lib_end[s] < lib_end[s - 1]) { set_error("mgta_contig_sample_coverage: lib_end[%d] < lib_end[%d]: the ends must not descend", s, s - 1); return MGTA_EINVAL; }
    if (lib_end[n_libs - 1] > reads->n_reads) {
        set_error("mgta_contig_sample_coverage: lib_end[%d] = %llu, the upload holds %llu reads", n_libs - 1, (unsigned long long)lib_end[n_libs - 1],
                  (unsigned long long)reads->n_reads);
        return MGTA_EINVAL;
    }
    if (n < 0 || (n > 0 && !offsets)) { set_error("mgta_contig_sample_coverage: bad contig count or offsets"); return MGTA_EINVAL; }
    if (n > 0x7FFFFFFFll) { set_error("mgta_contig_sample_coverage: %lld contigs (n < 2^31 is supported)", (long long)n); return MGTA_EINVAL; }
    if (g->dev.k + 1 > kMatchMaxWindow) { set_error("mgta_contig_sample_coverage: k = %d (k + 1 <= %d is supported)", g->dev.k, kMatchMaxWindow); return MGTA_EINVAL; }
    const uint64_t k = (uint64_t)g->dev.k;
    uint64_t total_win = 0;
    if (!check_contigs("mgta_contig_sample_coverage", seqs, offsets, n, k, kMaxContigLetters, kMaxCallWindows, &total_win, nullptr)) return MGTA_EINVAL;
    // the table holds the edges of both strands: at most half full, a slot number is 32 bits
    const uint64_t most_keys = std::min<uint64_t>(2 * total_win, (uint64_t)std::max<int64_t>(g->dev.size, 0));
    if (2 * most_keys + 2 > (1ull << 32)) {
        set_error("mgta_contig_sample_coverage: %llu keys need a count table of more than 2^32 slots", (unsigned long long)most_keys);
        return MGTA_ENOMEM;
    }
    const uint64_t L = (uint64_t)n_libs;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (lib_hit_windows) memset(lib_hit_windows, 0, L * 8);
    if (n == 0) return MGTA_OK;
    return guarded("mgta_contig_sample_coverage", [&]() {
        mgta_ctx *ctx = g->ctx;
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        Timer t_walk(st), t_count(st), t_scan(st), t_mass(st);
        const uint64_t cap = ctx->coverage_batch_windows ? ctx->coverage_batch_windows : 1ull << 28;   // windows per batch: 4 GB of edge ids, both strands
        uint32_t *d_marks = marks_reset(g, st);
        DevBuf d_cnt, d_sym, d_jobs, d_own, d_rc, d_counts, d_ends, d_hits, d_woff, d_lens, d_out, d_mass, d_pwc, d_pws;
        d_cnt.alloc(128);
        MGTA_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 128, st));
        unsigned long long *cnt_mark = d_cnt.as<unsigned long long>(), *cnt_scan = cnt_mark + 8;
        SampleTableMem tm;
        sample_table_alloc(ctx, st, most_keys, &ctx->live_bytes, &ctx->peak_bytes, tm);
        const SampleTable &tab = tm.t;
        d_own.alloc(total_win * 4 + 16, &ctx->live_bytes, &ctx->peak_bytes);
        d_rc.alloc(total_win * 4 + 16, &ctx->live_bytes, &ctx->peak_bytes);
        // ---- the keys: both strands of every contig, batch by batch
        const int walk_per_cu = queue_per_cu(share_walk_kernel);
        std::vector<CovJob> jobs;
        uint64_t win_done = 0, n_win = 0;
        double ms_walk = 0, ms_count = 0;
        int64_t n_batches = 0;
        for (int64_t c0 = 0, c1; c0 < n; c0 = c1) {
            c1 = cut_batch(offsets, n, k, c0, cap, true, jobs, &n_win);
            const uint32_t nj = (uint32_t)jobs.size();
            const uint64_t batch_longest = contig_windows(jobs[0].len, k);
            const uint64_t n_bytes = offsets[c1] - offsets[c0];
            if (d_sym.bytes < 2 * n_bytes + 16) d_sym.alloc(2 * n_bytes + 16, &ctx->live_bytes, &ctx->peak_bytes);
            if (d_jobs.bytes < (size_t)nj * sizeof(CovJob)) d_jobs.alloc((size_t)nj * sizeof(CovJob), &ctx->live_bytes, &ctx->peak_bytes);
            int64_t *d_ids = reinterpret_cast<int64_t *>(window_scratch(ctx, 2 * n_win * 8 + 64));
            MGTA_HIP_CHECK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)nj * sizeof(CovJob), hipMemcpyHostToDevice, st));
            MGTA_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 8, st));            // the queue head
            stage_symbols(ctx, st, d_sym, seqs + offsets[c0], n_bytes, true);
            const QueueLaunch q = queue_launch(ctx, walk_per_cu, nj, 64, 4);
            t_walk.start();
            if (g->dev.size > 0)
                hipLaunchKernelGGL(share_walk_kernel, dim3(q.blocks), dim3(kCovThreads), 0, st, g->dev, d_sym.as<uint8_t>(), d_jobs.as<CovJob>(), nj, q.chunk, d_ids, cnt_mark);
            else
                MGTA_HIP_CHECK(hipMemsetAsync(d_ids, 0xFF, 2 * n_win * 8 + 64, st));   // no edge anywhere
            MGTA_HIP_CHECK(hipGetLastError());
            t_walk.end();
            t_count.start();
            if (batch_longest) {
                const unsigned gy = (unsigned)std::min<uint64_t>((batch_longest + 255) / 256, 1024);
                hipLaunchKernelGGL(sample_count_kernel, dim3((nj + 63) / 64, gy), dim3(256), 0, st, tab, d_jobs.as<CovJob>(), nj, (int)k, d_ids, n_win, win_done,
                                   d_own.as<uint32_t>(), d_rc.as<uint32_t>(), d_marks, cnt_mark);
            }
            MGTA_HIP_CHECK(hipGetLastError());
            t_count.end();
            MGTA_HIP_CHECK(hipStreamSynchronize(st));                     // (jobs and the device buffers serve the next batch)
            ms_walk += t_walk.ms();
            ms_count += t_count.ms();
            win_done += n_win;
            ++n_batches;
        }
        unsigned long long cnt[16] = {0};
        MGTA_HIP_CHECK(hipMemcpyAsync(cnt, d_cnt.p, 64, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        if (cnt[5]) { set_error("mgta_contig_sample_coverage: the count table of %llu slots ran full", (unsigned long long)tab.n_slots); return MGTA_EHIP; }
        // ---- every batch is in: the keys are final and get their numbers.  The batch buffers make room for the counts and the outputs.
        d_sym.release(); d_jobs.release();
        const uint64_t n_keys = cnt[3], n_scan = lib_end[n_libs - 1];
        const uint64_t count_b = (n_keys + 1) * L * 8;
        d_counts.alloc(count_b, &ctx->live_bytes, &ctx->peak_bytes);
        d_ends.alloc(L * 8); d_hits.alloc(L * 8);
        MGTA_HIP_CHECK(hipMemsetAsync(d_counts.p, 0, count_b, st));
        MGTA_HIP_CHECK(hipMemsetAsync(d_hits.p, 0, L * 8, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_ends.p, lib_end, L * 8, hipMemcpyHostToDevice, st));
        t_count.start();
        hipLaunchKernelGGL(sample_dense_kernel, dim3((unsigned)std::min<uint64_t>(tab.n_slots / 256, (uint64_t)ctx->num_cus * 16)), dim3(256), 0, st, tab, cnt_mark);
        MGTA_HIP_CHECK(hipGetLastError());
        t_count.end();
        // ---- the read scan
        const QueueLaunch q_scan = queue_launch(ctx, queue_per_cu(sample_scan_kernel), n_scan, 256, 16);
        t_scan.start();
        if (n_scan && g->dev.size > 0)
            hipLaunchKernelGGL(sample_scan_kernel, dim3(q_scan.blocks), dim3(kCovThreads), 0, st, g->dev, reads->d_packed, reads->d_start, n_scan, reads_reversed ? 1 : 0,
                               q_scan.chunk, d_marks, tab, d_counts.as<unsigned long long>(), d_ends.as<uint64_t>(), n_libs, d_hits.as<unsigned long long>(), cnt_scan);
        MGTA_HIP_CHECK(hipGetLastError());
        t_scan.end();
        // ---- the masses: one wave per contig
        std::vector<uint32_t> lens;
        const std::vector<uint64_t> woff = window_offsets(offsets, n, k, &lens);
        d_woff.alloc(((size_t)n + 1) * 8, &ctx->live_bytes, &ctx->peak_bytes);
        d_lens.alloc((size_t)n * 4, &ctx->live_bytes, &ctx->peak_bytes);
        d_out.alloc((size_t)n * sizeof(mgta_contig_share), &ctx->live_bytes, &ctx->peak_bytes);
        d_mass.alloc((size_t)n * L * 8, &ctx->live_bytes, &ctx->peak_bytes);
        if (per_window_count && total_win) d_pwc.alloc(total_win * L * 8, &ctx->live_bytes, &ctx->peak_bytes);
        if (per_window_share && total_win) d_pws.alloc(total_win * 4, &ctx->live_bytes, &ctx->peak_bytes);
        MGTA_HIP_CHECK(hipMemcpyAsync(d_woff.p, woff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_lens.p, lens.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        t_mass.start();
        hipLaunchKernelGGL(sample_mass_kernel, dim3((unsigned)(((uint64_t)n + 3) / 4)), dim3(256), 0, st, d_woff.as<uint64_t>(), d_lens.as<uint32_t>(), (uint32_t)n,
                           d_own.as<uint32_t>(), d_rc.as<uint32_t>(), tab, d_counts.as<unsigned long long>(), n_libs, d_mass.as<uint64_t>(), d_out.as<mgta_contig_share>(),
                           d_pwc.as<uint64_t>(), d_pws.as<uint32_t>());
        MGTA_HIP_CHECK(hipGetLastError());
        t_mass.end();
        std::vector<mgta_contig_share> rec((size_t)n);
        std::vector<uint64_t> hits((size_t)L);
        MGTA_HIP_CHECK(hipMemcpyAsync(mass, d_mass.p, (size_t)n * L * 8, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(rec.data(), d_out.p, (size_t)n * sizeof(mgta_contig_share), hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(hits.data(), d_hits.p, L * 8, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(cnt, d_cnt.p, 128, hipMemcpyDeviceToHost, st));
        if (d_pwc.p) MGTA_HIP_CHECK(hipMemcpyAsync(per_window_count, d_pwc.p, total_win * L * 8, hipMemcpyDeviceToHost, st));
        if (d_pws.p) MGTA_HIP_CHECK(hipMemcpyAsync(per_window_share, d_pws.p, total_win * 4, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        if (per_contig) memcpy(per_contig, rec.data(), (size_t)n * sizeof(mgta_contig_share));
        if (lib_hit_windows) memcpy(lib_hit_windows, hits.data(), L * 8);
        if (stats) {
            uint64_t total = 0, covered = 0;
            for (int64_t i = 0; i < n; ++i) { total += rec[(size_t)i].mass; covered += rec[(size_t)i].n_covered; }
            stats->n_contigs = n; stats->n_windows = (int64_t)total_win; stats->n_walked = (int64_t)cnt[1]; stats->n_index_searches = (int64_t)cnt[2];
            stats->n_batches = n_batches; stats->n_covered = (int64_t)covered; stats->n_keys = (int64_t)n_keys; stats->n_libs = n_libs;
            stats->n_reads = (int64_t)n_scan; stats->n_read_windows = (int64_t)cnt[12]; stats->n_read_walked = (int64_t)cnt[9];
            stats->n_read_index_searches = (int64_t)cnt[10]; stats->n_hit_windows = (int64_t)cnt[11]; stats->groups_per_cu = q_scan.groups_per_cu();
            stats->total_mass = total; stats->table_slots = tab.n_slots; stats->table_bytes = tab.n_slots * 16; stats->window_bytes = total_win * 8;
            stats->count_bytes = count_b;
            stats->ms_mark = ms_walk + ms_count + t_count.ms(); stats->ms_scan = t_scan.ms(); stats->ms_mass = t_mass.ms();
            stats->ms_total = stats->ms_mark + stats->ms_scan + stats->ms_mass;
        }
        return MGTA_OK;
    });
}

}  // extern "C"
