// cluster_tree.hpp — the complete-linkage merge tree of the kept pairs on the device (mgta_pairs_tree; the contract is in
// include/megagta_hip.h).  Included by cluster.hip only.
//
// Lists.  Every cluster is named by its lowest row and owns a list of (neighbour name, n_diff << 16 | n_overlap), 8 bytes an entry,
// ascending by name: the clusters all of whose cross pairs with it are kept, at the largest fraction over those pairs.  The lists
// are symmetric.  They are built from the sorted pairs: count per row (atomic adds; the counts do not depend on their order), scan
// (scan.hpp), fill.  The entries of row r towards higher rows are r's own pairs in their order and go straight to their place; those
// towards lower rows arrive through an atomic cursor in any order and are put in order by rank (tree_order_kernel; names are distinct),
// so the lists do not depend on timing.  A list lives in one of two buffers at the same offset, Lists::side says which.
//
// Rounds.  nn[x] = the neighbour of x with the smallest (fraction, name): for a fixed x that is the smallest key of the contract.  A
// round: (1) tree_merge_kernel, one wave per row: x < nn[x] and nn[nn[x]] == x is a merge of this round; the wave records it, sets
// partner[x] and partner[nn[x]] stamped with the round, and puts every name of the two old lists, and x, on the round's list of affected
// clusters (an atomic exchange on a stamp per cluster lets each in once).  (2) The host reads two counters back: no new merge ends the
// loop.  (3) tree_rewrite_kernel, one wave per affected cluster: it reads its own list, or the lists of its two halves, writes the
// new list into the other buffer of the lower half's segment, and takes the new nn on the way.  An entry towards u survives when the
// entries towards u and towards u's partner of this round are in all of our old lists (2 or 4 entries, found by binary search: the
// lists are sorted); it keeps the lower name and the largest of the fractions.  Survivors keep their order, so the lists stay sorted
// and only shrink.  A cluster that is not affected keeps its list and its nn.
// No kernel waits for another workgroup.  In one launch nothing is read that another workgroup writes: (1) reads nn, the lists and
// their sides, and writes partner, stamps and the lists of merges and of affected clusters (atomics, never read there); (3) reads
// partner and the old lists, and writes side / len / nn of the one or two clusters a wave owns and the other buffer of its segment.
// The order of the merge records and of the affected list depends on timing; the records are sorted by the host, the affected list
// only decides which wave does which cluster, and the counters are sums.
#pragma once
#include "common.hpp"
#include "device_utils.hpp"
#include "scan.hpp"

namespace mgta {
namespace tree {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kApart = 1u << 16;                     // 1 / 0: above every fraction
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;

struct Lists {
    const uint64_t *start;       // [n + 1] first entry of every row's segment
    uint2 *buf[2];               // [2 * n_pairs] each
    uint32_t *len;               // [n]
    uint32_t *side;              // [n] the buffer that holds the list
    uint32_t *nn, *nnf;          // [n] the nearest neighbour (kNone: no entry) and the fraction towards it
    uint64_t *partner;           // [n] round << 32 | the other half of the merge of that round
    uint32_t *stamp;             // [n] the last round the cluster was put on the affected list
    uint32_t *affected;          // [n]
    uint32_t *counters;          // [0] merges so far, [1] affected clusters of this round, [2] a cluster still has a neighbour, [3] lists rewritten so far
    unsigned long long *visited; // list entries read
    uint4 *merges;               // [n] (a, b, fraction, round)
    uint32_t n;
};

__device__ __forceinline__ bool frac_lt(uint32_t f, uint32_t g) { return (f >> 16) * (g & 0xFFFFu) < (g >> 16) * (f & 0xFFFFu); }   // both products < 2^32
__device__ __forceinline__ uint32_t frac_max(uint32_t f, uint32_t g) { return frac_lt(f, g) ? g : f; }
__device__ __forceinline__ bool key_lt(uint32_t f, uint32_t u, uint32_t g, uint32_t v) { return frac_lt(f, g) || (!frac_lt(g, f) && u < v); }

// the smallest (fraction, name) over the wave, in every lane
__device__ __forceinline__ void wave_min_key(uint32_t &f, uint32_t &u) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t g = __shfl_xor(f, d, 64), v = __shfl_xor(u, d, 64);
        if (key_lt(g, v, f, u)) { f = g; u = v; }
    }
}

// the entry towards `name` in a sorted list: its fraction, or false
__device__ __forceinline__ bool find(const uint2 *list, uint32_t len, uint32_t name, uint32_t &f) {
    uint32_t lo = 0, hi = len;
    while (lo < hi) {                                     // at most 32 steps
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (list[mid].x < name) lo = mid + 1; else hi = mid;
    }
    if (lo >= len) return false;
    const uint2 e = list[lo];
    if (e.x != name) return false;
    f = e.y;
    return true;
}

// ---- build ---------------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(kThreads) void tree_count_kernel(const mgta_row_pair *pairs, uint64_t n_pairs, uint32_t *deg, uint32_t *low) {
    const uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n_pairs) return;
    const mgta_row_pair p = pairs[e];
    atomicAdd(&deg[p.i], 1u);
    atomicAdd(&deg[p.j], 1u);
    atomicAdd(&low[p.j], 1u);
}

// first_pair[i] = the index of the first pair (i, *)
static __global__ __launch_bounds__(kThreads) void tree_first_kernel(const mgta_row_pair *pairs, uint64_t n_pairs, uint64_t *first_pair) {
    const uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n_pairs) return;
    const int32_t i = pairs[e].i;
    if (e == 0 || pairs[e - 1].i != i) first_pair[i] = e;
}

// the pair (i, j): into i's list at its place behind the lower names, into the unordered lower part of j's list (buffer 1)
static __global__ __launch_bounds__(kThreads) void tree_fill_kernel(const mgta_row_pair *pairs, uint64_t n_pairs, const uint64_t *start, const uint32_t *low,
                                                             const uint64_t *first_pair, uint32_t *cursor, uint2 *buf0, uint2 *buf1) {
    const uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n_pairs) return;
    const mgta_row_pair p = pairs[e];
    const uint32_t f = (uint32_t)p.n_diff << 16 | p.n_overlap;
    buf0[start[p.i] + low[p.i] + (e - first_pair[p.i])] = make_uint2((uint32_t)p.j, f);
    buf1[start[p.j] + atomicAdd(&cursor[p.j], 1u)] = make_uint2((uint32_t)p.i, f);
}

// one wave per row: the lower part of its list from buffer 1 into buffer 0 in the order of the names, and the row's first nn
static __global__ __launch_bounds__(kThreads) void tree_order_kernel(Lists L, const uint32_t *low, const uint32_t *deg) {
    const uint32_t x = blockIdx.x * kWaves + wave_id();
    if (x >= L.n) return;
    const uint64_t s = L.start[x];
    const uint32_t n_low = low[x], len = deg[x];
    const uint2 *src = L.buf[1] + s;
    uint2 *dst = L.buf[0] + s;
    uint32_t bf = kApart, bu = kNone;
    for (uint32_t k0 = 0; k0 < n_low; k0 += 64) {
        const uint32_t k = k0 + lane_id();
        const uint2 e = k < n_low ? src[k] : make_uint2(kNone, kApart);
        uint32_t rank = 0;
        for (uint32_t t = 0; t < n_low; ++t) rank += src[t].x < e.x;
        if (k < n_low) {
            dst[rank] = e;
            if (key_lt(e.y, e.x, bf, bu)) { bf = e.y; bu = e.x; }
        }
    }
    for (uint32_t k = n_low + lane_id(); k < len; k += 64) {
        const uint2 e = dst[k];                           // written by tree_fill_kernel
        if (key_lt(e.y, e.x, bf, bu)) { bf = e.y; bu = e.x; }
    }
    wave_min_key(bf, bu);
    if (lane_id() == 0) { L.len[x] = len; L.side[x] = 0; L.nn[x] = bu; L.nnf[x] = bf; }
}

// ---- a round -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void mark(const Lists &L, uint32_t u, bool valid, uint32_t round) {
    const bool fresh = valid && atomicExch(&L.stamp[u], round) != round;
    const uint64_t m = __ballot(fresh);
    if (m == 0) return;
    uint32_t base = 0;
    if (lane_id() == 0) base = atomicAdd(&L.counters[1], (uint32_t)__popcll(m));
    base = wave_uniform(base);
    if (fresh) L.affected[base + (uint32_t)__popcll(m & lanemask_lt())] = u;     // every cluster enters once a round: at most n entries
}

static __global__ __launch_bounds__(kThreads) void tree_merge_kernel(Lists L, uint32_t round) {
    const uint32_t x = blockIdx.x * kWaves + wave_id();
    if (x >= L.n) return;
    const uint32_t y = L.nn[x];
    if (y == kNone || y <= x || y >= L.n || L.nn[y] != x) return;
    if (lane_id() == 0) {
        const uint32_t slot = atomicAdd(&L.counters[0], 1u);                     // a merge removes a cluster: at most n - 1 of them
        L.merges[slot] = make_uint4(x, y, L.nnf[x], round);
        L.partner[x] = (uint64_t)round << 32 | y;
        L.partner[y] = (uint64_t)round << 32 | x;
    }
    mark(L, x, lane_id() == 0, round);
    for (int h = 0; h < 2; ++h) {
        const uint32_t c = h ? y : x, len = L.len[c];
        const uint2 *list = L.buf[L.side[c] & 1] + L.start[c];
        for (uint32_t k0 = 0; k0 < len; k0 += 64) {
            const uint32_t k = k0 + lane_id();
            const uint32_t u = k < len ? list[k].x : kNone;
            mark(L, u, k < len && u != x && u != y && u < L.n, round);
        }
    }
}

static __global__ __launch_bounds__(kThreads) void tree_rewrite_kernel(Lists L, uint32_t round, uint32_t n_affected) {
    const uint32_t w = blockIdx.x * kWaves + wave_id();
    if (w >= n_affected) return;
    const uint32_t x = L.affected[w];
    if (x >= L.n) return;
    const uint64_t px = L.partner[x];
    const bool merged = (uint32_t)(px >> 32) == round;
    const uint32_t y = merged ? (uint32_t)px : kNone;
    if (merged && y < x) return;                          // the higher half (a third merge's list named it): the lower half's wave does both
    const uint32_t sx = L.side[x] & 1, len_x = L.len[x], len_y = merged ? L.len[y] : 0;
    const uint2 *lx = L.buf[sx] + L.start[x];
    const uint2 *ly = merged ? L.buf[L.side[y] & 1] + L.start[y] : lx;
    uint2 *out = L.buf[sx ^ 1] + L.start[x];
    uint32_t base = 0, bf = kApart, bu = kNone;
    for (uint32_t k0 = 0; k0 < len_x; k0 += 64) {
        const uint32_t k = k0 + lane_id();
        bool keep = false;
        uint2 e = make_uint2(kNone, kApart);
        if (k < len_x) {
            e = lx[k];
            keep = e.x != y && e.x < L.n;
            uint32_t g;
            if (keep && merged) { keep = find(ly, len_y, e.x, g); if (keep) e.y = frac_max(e.y, g); }
            if (keep) {
                const uint64_t pu = L.partner[e.x];
                if ((uint32_t)(pu >> 32) == round) {
                    const uint32_t p = (uint32_t)pu;
                    keep = e.x < p && find(lx, len_x, p, g);                     // the union keeps the lower name
                    if (keep) e.y = frac_max(e.y, g);
                    if (keep && merged) { keep = find(ly, len_y, p, g); if (keep) e.y = frac_max(e.y, g); }
                }
            }
        }
        const uint64_t m = __ballot(keep);
        if (keep) {
            out[base + (uint32_t)__popcll(m & lanemask_lt())] = e;               // base + rank <= k: inside the segment
            if (key_lt(e.y, e.x, bf, bu)) { bf = e.y; bu = e.x; }
        }
        base += (uint32_t)__popcll(m);
    }
    wave_min_key(bf, bu);
    if (lane_id() == 0) {
        L.len[x] = base; L.side[x] = sx ^ 1; L.nn[x] = bu; L.nnf[x] = bf;
        if (merged) { L.len[y] = 0; L.nn[y] = kNone; L.nnf[y] = kApart; }
        atomicAdd(L.visited, (unsigned long long)len_x + len_y);
        atomicAdd(&L.counters[3], 1u);
    }
}

// after a round without a merge: does any cluster still have a neighbour?  (then the rounds went wrong: the smallest key is mutual)
static __global__ __launch_bounds__(kThreads) void tree_left_kernel(Lists L) {
    const uint32_t x = blockIdx.x * kThreads + threadIdx.x;
    if (x < L.n && L.nn[x] != kNone) L.counters[2] = 1u;
}

}  // namespace tree

struct TreeMerge { uint32_t a, b, f; };                   // f = n_diff << 16 | n_overlap, as found (not in lowest terms)

// The merges of the kept pairs P (checked by the caller; n >= 1), in the order the device recorded them.  Fills the device fields of *st.
inline int tree_impl(mgta_ctx *ctx, const char *who, const mgta_row_pair *P, uint64_t n_pairs, uint32_t n, std::vector<TreeMerge> &found, mgta_tree_stats *st) {
    using namespace tree;
    MGTA_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    uint64_t *live = &ctx->live_bytes, *peak = &ctx->peak_bytes;
    struct PeakOfCall {
        uint64_t *peak, before;
        ~PeakOfCall() { *peak = std::max(*peak, before); }
    } peak_of_call{peak, *peak};
    *peak = *live;
    found.clear();
    if (n_pairs == 0) { st->peak_bytes = 0; return (int)MGTA_OK; }
    if (n_pairs >= (uint64_t)kNone) { set_error("%s: %llu kept pairs (the linkage holds fewer than 2^32)", who, (unsigned long long)n_pairs); return (int)MGTA_ENOMEM; }

    const uint64_t E = 2 * n_pairs;
    const uint64_t need = n_pairs * sizeof(mgta_row_pair) + 2 * E * 8 + (uint64_t)n * 80 + scan_tmp_elems(n) * 8 + 64;
    size_t dev_free = 0, dev_total = 0;
    MGTA_HIP_CHECK(hipMemGetInfo(&dev_free, &dev_total));
    if ((ctx->mem_limit && *live + need > ctx->mem_limit) || need > dev_free) {
        set_error("%s: the lists of %llu kept pairs of %u rows need %llu bytes of device memory", who, (unsigned long long)n_pairs, n, (unsigned long long)need);
        return (int)MGTA_ENOMEM;
    }
    DevBuf d_pairs, d_buf0, d_buf1, d_start, d_len, d_side, d_nn, d_nnf, d_partner, d_stamp, d_aff, d_cnt, d_vis, d_merges, d_deg, d_low, d_cursor, d_first, d_tmp, d_total;
    d_pairs.alloc(n_pairs * sizeof(mgta_row_pair), live, peak);
    d_buf0.alloc(E * 8, live, peak); d_buf1.alloc(E * 8, live, peak);
    d_start.alloc(((size_t)n + 1) * 8, live, peak);
    d_len.alloc((size_t)n * 4, live, peak); d_side.alloc((size_t)n * 4, live, peak); d_nn.alloc((size_t)n * 4, live, peak); d_nnf.alloc((size_t)n * 4, live, peak);
    d_partner.alloc((size_t)n * 8, live, peak); d_stamp.alloc((size_t)n * 4, live, peak); d_aff.alloc((size_t)n * 4, live, peak);
    d_cnt.alloc(16, live, peak); d_vis.alloc(8, live, peak); d_merges.alloc((size_t)n * 16, live, peak);
    d_deg.alloc((size_t)n * 4, live, peak); d_low.alloc((size_t)n * 4, live, peak); d_cursor.alloc((size_t)n * 4, live, peak);
    d_first.alloc((size_t)n * 8, live, peak); d_tmp.alloc((size_t)scan_tmp_elems(n) * 8, live, peak); d_total.alloc(8, live, peak);

    Lists L;
    L.start = d_start.as<uint64_t>(); L.buf[0] = d_buf0.as<uint2>(); L.buf[1] = d_buf1.as<uint2>(); L.len = d_len.as<uint32_t>(); L.side = d_side.as<uint32_t>();
    L.nn = d_nn.as<uint32_t>(); L.nnf = d_nnf.as<uint32_t>(); L.partner = d_partner.as<uint64_t>(); L.stamp = d_stamp.as<uint32_t>();
    L.affected = d_aff.as<uint32_t>(); L.counters = d_cnt.as<uint32_t>(); L.visited = d_vis.as<unsigned long long>(); L.merges = d_merges.as<uint4>(); L.n = n;

    const unsigned pair_blocks = (unsigned)((n_pairs + kThreads - 1) / kThreads);               // n_pairs < 2^32: fits
    const unsigned wave_blocks = (unsigned)(((uint64_t)n + kWaves - 1) / kWaves);
    Timer t_build(s), t_round(s);
    MGTA_HIP_CHECK(hipMemcpyAsync(d_pairs.p, P, n_pairs * sizeof(mgta_row_pair), hipMemcpyHostToDevice, s));
    t_build.start();
    MGTA_HIP_CHECK(hipMemsetAsync(d_deg.p, 0, (size_t)n * 4, s));
    MGTA_HIP_CHECK(hipMemsetAsync(d_low.p, 0, (size_t)n * 4, s));
    MGTA_HIP_CHECK(hipMemsetAsync(d_cursor.p, 0, (size_t)n * 4, s));
    MGTA_HIP_CHECK(hipMemsetAsync(d_first.p, 0, (size_t)n * 8, s));
    MGTA_HIP_CHECK(hipMemsetAsync(d_partner.p, 0, (size_t)n * 8, s));
    MGTA_HIP_CHECK(hipMemsetAsync(d_stamp.p, 0, (size_t)n * 4, s));
    MGTA_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 16, s));
    MGTA_HIP_CHECK(hipMemsetAsync(d_vis.p, 0, 8, s));
    hipLaunchKernelGGL(tree_count_kernel, dim3(pair_blocks), dim3(kThreads), 0, s, d_pairs.as<mgta_row_pair>(), n_pairs, d_deg.as<uint32_t>(), d_low.as<uint32_t>());
    hipLaunchKernelGGL(tree_first_kernel, dim3(pair_blocks), dim3(kThreads), 0, s, d_pairs.as<mgta_row_pair>(), n_pairs, d_first.as<uint64_t>());
    exclusive_scan_u32(s, d_deg.as<uint32_t>(), n, d_start.as<uint64_t>(), d_tmp.as<uint64_t>(), d_total.as<uint64_t>());
    MGTA_HIP_CHECK(hipMemcpyAsync(d_start.as<uint64_t>() + n, d_total.p, 8, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(tree_fill_kernel, dim3(pair_blocks), dim3(kThreads), 0, s, d_pairs.as<mgta_row_pair>(), n_pairs, d_start.as<uint64_t>(), d_low.as<uint32_t>(),
                       d_first.as<uint64_t>(), d_cursor.as<uint32_t>(), L.buf[0], L.buf[1]);
    hipLaunchKernelGGL(tree_order_kernel, dim3(wave_blocks), dim3(kThreads), 0, s, L, d_low.as<uint32_t>(), d_deg.as<uint32_t>());
    st->ms_build = t_build.stop();
    d_pairs.release();

    uint32_t n_merges = 0;
    int64_t n_rounds = 0;
    double ms_rounds = 0;
    for (uint32_t round = 1;; ++round) {
        if (round > n) { set_error("%s: internal error: the rounds did not end after %u", who, n); return (int)MGTA_EHIP; }
        uint32_t back[2] = {0, 0};
        t_round.start();
        MGTA_HIP_CHECK(hipMemsetAsync(d_cnt.as<uint32_t>() + 1, 0, 4, s));
        hipLaunchKernelGGL(tree_merge_kernel, dim3(wave_blocks), dim3(kThreads), 0, s, L, round);
        MGTA_HIP_CHECK(hipMemcpyAsync(back, d_cnt.p, 8, hipMemcpyDeviceToHost, s));
        ms_rounds += t_round.stop();
        if (back[0] < n_merges || back[0] >= n || back[1] > n) { set_error("%s: internal error: %u merges and %u affected clusters of %u rows", who, back[0], back[1], n); return (int)MGTA_EHIP; }
        if (back[0] == n_merges) {
            uint32_t left = 0;
            hipLaunchKernelGGL(tree_left_kernel, dim3((unsigned)(((uint64_t)n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, L);
            MGTA_HIP_CHECK(hipGetLastError());
            MGTA_HIP_CHECK(hipMemcpyAsync(&left, d_cnt.as<uint32_t>() + 2, 4, hipMemcpyDeviceToHost, s));
            MGTA_HIP_CHECK(hipStreamSynchronize(s));
            if (left) { set_error("%s: internal error: round %u has candidates and no merge", who, round); return (int)MGTA_EHIP; }
            break;
        }
        n_merges = back[0];
        ++n_rounds;
        t_round.start();
        hipLaunchKernelGGL(tree_rewrite_kernel, dim3((back[1] + kWaves - 1) / kWaves), dim3(kThreads), 0, s, L, round, back[1]);
        ms_rounds += t_round.stop();
    }
    std::vector<uint4> raw(n_merges);
    unsigned long long visited = 0;
    if (n_merges) MGTA_HIP_CHECK(hipMemcpyAsync(raw.data(), d_merges.p, (size_t)n_merges * 16, hipMemcpyDeviceToHost, s));
    uint32_t n_rewritten = 0;
    MGTA_HIP_CHECK(hipMemcpyAsync(&visited, d_vis.p, 8, hipMemcpyDeviceToHost, s));
    MGTA_HIP_CHECK(hipMemcpyAsync(&n_rewritten, d_cnt.as<uint32_t>() + 3, 4, hipMemcpyDeviceToHost, s));
    MGTA_HIP_CHECK(hipStreamSynchronize(s));
    found.reserve(n_merges);
    for (const uint4 &m : raw) found.push_back(TreeMerge{m.x, m.y, m.z});
    st->n_rounds = n_rounds; st->n_lists_rewritten = n_rewritten; st->n_entries_visited = (int64_t)(E + visited);   // E: the first nn of every list
    st->ms_rounds = ms_rounds; st->peak_bytes = (int64_t)*peak;
    return (int)MGTA_OK;
}

}  // namespace mgta
