// cluster.hip — complete-linkage clusters of a gene's aligned contigs (mgta_rows_pairs, mgta_rows_cluster): the place of "cluster at
// 99% aa identity" in the reference's bin/post_proc.sh:57-85 (`Clustering.jar dmatrix -l 25`, `cluster`, `rep-seqs`).  The rule is this
// library's own (include/megagta_hip.h), not the jars'.
//
// Pairs, on the device.  All pairs of n rows of M bytes are O(n^2 M) byte work.  The rows are laid out once for it (cluster_layout_kernel):
// every byte is XORed with '-', so that a gap is 0, and columns are taken 32 at a time (a GROUP): 8 words of 4 bytes and one word with a
// bit per column that holds a residue.  The layout is word-major, U[(group * 9 + k) * n_pad + row]: the same word of 64 consecutive rows
// is 256 contiguous bytes, in device memory and in LDS.  With A, B the mask words of two rows and a, b a byte word,
//     n_overlap  = sum popc(A & B)
//     n_diff     = sum (bytes of a ^ b that are not 0) - sum popc(A ^ B)
// since a column where only one row has a residue is a non-zero byte of a ^ b (0 against non-zero), and two gaps are a zero byte.
// cluster_pairs_kernel: a workgroup of 256 lanes owns 64 x 64 pairs, 64 rows of each side staged in LDS kGroupsPerStage groups at a time;
// a lane owns 4 x 4 pairs: rows ty*4 .. +3 against rows tx*4 .. +3, so one 16-byte LDS read per side and word feeds 16 pair-words (the 16
// lanes tx = 0 .. 15 read 256 contiguous bytes, the 4 values of ty in a wave are broadcasts).  Per pair-word: xor, and, add, or, and,
// popcount-accumulate.  The two counts stay in 32 registers.  The result of a pair is one 32-bit word, n_diff << 16 | n_overlap when the
// pair is kept and 0 when it is apart (a kept pair has n_overlap >= min_overlap >= 1), written 16 bytes per lane into a dense
// tile of (row block) x (row block) words.
// Kept pairs leave by count -> scan -> write: one wave per row counts the non-zero words right of the diagonal, scan.hpp turns the counts
// into offsets, one wave per row writes its pairs in column order (ballot + prefix popcount).  The list of a tile is sorted by (i, j)
// with no dependence on the order of any atomic operation: there is none.
// Tiles.  Rows are taken in row blocks of R (mgta_ctx_set_cluster_tile, default 4096); the device works on one (block I, block J >= I)
// tile at a time: 4 R^2 bytes dense, the tile's kept pairs, and the laid-out rows (1.125 bytes per input byte) are all it holds.  The
// host puts the tiles of one block I together row by row, which is the (i, j) order.
//
// Linkage, on the host.  Connected components of the kept-pair graph by union-find; inside a component clusters are named by their
// lowest member, a hash map holds the distance of every pair of clusters whose cross pairs are all kept, a heap the candidates by
// (distance, lower name, higher name) with a version per cluster to drop stale ones.  Merging (a, b), a < b: a cluster x stays
// linkable to the union only if it was to both, at the larger of the two distances; everything else can never be merged with the
// union, because an apart cross pair stays.  Distances are fractions n_diff / n_overlap compared by cross-multiplication.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>
#include <queue>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "device_utils.hpp"
#include "scan.hpp"
#include "cluster_tree.hpp"

namespace mgta {
namespace {

constexpr int kPairThreads = 256;
constexpr int kTileSide = 64;             // rows of each side of a workgroup's pairs
constexpr int kWordsPerGroup = 9;         // 32 columns: 8 byte words + the mask word
constexpr int kGroupsPerStage = 4;        // 128 columns in LDS at a time
constexpr int kStageWords = kGroupsPerStage * kWordsPerGroup;
constexpr int64_t kDefaultTileRows = 4096;
constexpr int64_t kMaxColumns = 65536;    // M < this: both counts fit 16 bits

// one thread per (group, row): 32 columns of a row -> 8 byte words (gap = 0) and the residue mask; rows from n on are gaps
__global__ __launch_bounds__(256) void cluster_layout_kernel(const uint8_t *rows, uint32_t n, uint32_t M, uint32_t n_groups, uint64_t n_pad, uint32_t *U) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)n_groups * n_pad) return;
    const uint64_t row = t % n_pad;
    const uint32_t g = (uint32_t)(t / n_pad);
    uint32_t w[8], mask = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = 0;
    if (row < n) {
        const uint8_t *p = rows + row * (uint64_t)M;
        const uint32_t c0 = g * 32, c1 = min(M, c0 + 32);
        for (uint32_t c = c0; c < c1; ++c) {
            const uint32_t x = (uint32_t)p[c] ^ (uint32_t)'-';
            w[(c - c0) >> 2] |= x << (8 * ((c - c0) & 3));
            mask |= (x != 0 ? 1u : 0u) << (c - c0);
        }
    }
    uint32_t *dst = U + (uint64_t)g * kWordsPerGroup * n_pad + row;
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[(uint64_t)k * n_pad] = w[k];
    dst[8ull * n_pad] = mask;
}

struct PairArgs {
    const uint32_t *U;
    uint64_t n_pad;
    uint32_t n, n_groups;
    uint32_t i0, j0;             // first row of each side of the tile
    uint32_t ld;                 // words of a row of the dense tile (a multiple of 64)
    uint32_t min_overlap;
    double cutoff;
    uint32_t *dense;
};

// the bytes of x that are not 0, counted
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x) { return (uint32_t)__popc((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u); }

__global__ __launch_bounds__(kPairThreads) void cluster_pairs_kernel(PairArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t sa[kStageWords * kTileSide];
    __shared__ __attribute__((aligned(16))) uint32_t sb[kStageWords * kTileSide];
    const uint32_t ra = a.i0 + blockIdx.y * kTileSide, rb = a.j0 + blockIdx.x * kTileSide;     // first rows of the two sides
    if (rb + (kTileSide - 1) <= ra) return;                                                   // every j of this workgroup <= every i
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    uint32_t diff[4][4], ov[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { diff[r][c] = 0; ov[r][c] = 0; }

    for (uint32_t g0 = 0; g0 < a.n_groups; g0 += kGroupsPerStage) {
        const uint32_t words = min((uint32_t)kGroupsPerStage, a.n_groups - g0) * kWordsPerGroup;
        __syncthreads();
        for (uint32_t idx = threadIdx.x; idx < words * kTileSide; idx += kPairThreads) {
            const uint64_t src = ((uint64_t)g0 * kWordsPerGroup + (idx >> 6)) * a.n_pad + (idx & 63);
            sa[idx] = a.U[src + ra];
            sb[idx] = a.U[src + rb];
        }
        __syncthreads();
        for (uint32_t w = 0; w < words; w += kWordsPerGroup) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint4 va = *reinterpret_cast<const uint4 *>(&sa[(w + k) * kTileSide + ty * 4]);
                const uint4 vb = *reinterpret_cast<const uint4 *>(&sb[(w + k) * kTileSide + tx * 4]);
                const uint32_t xa[4] = {va.x, va.y, va.z, va.w}, xb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) diff[r][c] += nonzero_bytes(xa[r] ^ xb[c]);
            }
            const uint4 ma = *reinterpret_cast<const uint4 *>(&sa[(w + 8) * kTileSide + ty * 4]);
            const uint4 mb = *reinterpret_cast<const uint4 *>(&sb[(w + 8) * kTileSide + tx * 4]);
            const uint32_t xa[4] = {ma.x, ma.y, ma.z, ma.w}, xb[4] = {mb.x, mb.y, mb.z, mb.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    ov[r][c] += (uint32_t)__popc(xa[r] & xb[c]);
                    diff[r][c] -= (uint32_t)__popc(xa[r] ^ xb[c]);       // the one-sided columns of this group, all counted above
                }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t i = ra + ty * 4 + r;
        uint32_t out[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t j = rb + tx * 4 + c;
            const bool kept = i < j && j < a.n && ov[r][c] >= a.min_overlap && (double)diff[r][c] <= a.cutoff * (double)ov[r][c];
            out[c] = kept ? (diff[r][c] << 16 | ov[r][c]) : 0u;
        }
        *reinterpret_cast<uint4 *>(&a.dense[(uint64_t)(blockIdx.y * kTileSide + ty * 4 + r) * a.ld + blockIdx.x * kTileSide + tx * 4]) =
            make_uint4(out[0], out[1], out[2], out[3]);
    }
}

// a word of the dense tile counts when it is right of the diagonal: the workgroups left of it did not run and wrote nothing
__device__ __forceinline__ uint32_t dense_word(const uint32_t *dense, uint32_t ld, uint32_t row, uint32_t col, uint32_t n_cols, uint32_t i, uint32_t j0) {
    if (col >= n_cols || j0 + col <= i) return 0;
    return dense[(uint64_t)row * ld + col];
}

// one wave per row of the tile
__global__ __launch_bounds__(256) void cluster_count_kernel(const uint32_t *dense, uint32_t ld, uint32_t n_rows, uint32_t n_cols, uint32_t i0, uint32_t j0, uint32_t *count) {
    const uint32_t row = blockIdx.x * 4 + wave_id();
    if (row >= n_rows) return;
    uint32_t c = 0;
    for (uint32_t col = lane_id(); col < n_cols; col += 64) c += dense_word(dense, ld, row, col, n_cols, i0 + row, j0) != 0;
    c = wave_sum(c);
    if (lane_id() == 0) count[row] = c;
}

__global__ __launch_bounds__(256) void cluster_write_kernel(const uint32_t *dense, uint32_t ld, uint32_t n_rows, uint32_t n_cols, uint32_t i0, uint32_t j0,
                                                            const uint64_t *offset, mgta_row_pair *pairs) {
    const uint32_t row = blockIdx.x * 4 + wave_id();
    if (row >= n_rows) return;
    uint64_t base = offset[row];
    for (uint32_t col0 = 0; col0 < n_cols; col0 += 64) {
        const uint32_t col = col0 + lane_id();
        const uint32_t v = dense_word(dense, ld, row, col, n_cols, i0 + row, j0);
        const uint64_t kept = __ballot(v != 0);
        if (v != 0) {
            mgta_row_pair p;
            p.i = (int32_t)(i0 + row); p.j = (int32_t)(j0 + col); p.n_diff = (uint16_t)(v >> 16); p.n_overlap = (uint16_t)(v & 0xFFFFu);
            pairs[base + (uint64_t)__popcll(kept & lanemask_lt())] = p;
        }
        base += (uint64_t)__popcll(kept);
    }
}

// ---- the pairs of all rows, sorted by (i, j) ------------------------------------------------------------------------------------------
// out == nullptr only counts.  The caller has checked the arguments.
int pairs_impl(mgta_ctx *ctx, const char *who, const uint8_t *rows, int64_t n, int64_t M, int64_t min_overlap, double cutoff, std::vector<mgta_row_pair> *out,
               int64_t *n_pairs, mgta_cluster_stats *stats) {
    MGTA_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    uint64_t *live = &ctx->live_bytes, *peak = &ctx->peak_bytes;
    struct PeakOfCall {                                                   // peak_bytes is this call's while it runs, the context's again on every way out
        uint64_t *peak, before;
        ~PeakOfCall() { *peak = std::max(*peak, before); }
    } peak_of_call{peak, *peak};
    *peak = *live;
    const uint32_t nn = (uint32_t)n, mm = (uint32_t)M;
    const uint32_t n_groups = (mm + 31) / 32;
    const uint64_t n_pad = (((uint64_t)nn + 63) / 64 + 1) * 64;          // a workgroup may start at any row and reads 64
    const uint64_t R = ctx->cluster_tile_rows ? ctx->cluster_tile_rows : (uint64_t)kDefaultTileRows;
    const uint32_t side = (uint32_t)std::min<uint64_t>(R, nn);            // rows of the largest tile
    const uint32_t side_blocks = (side + kTileSide - 1) / kTileSide;
    const uint32_t ld = side_blocks * kTileSide;

    Timer t_a(st), t_b(st);
    double ms = 0;
    DevBuf d_U, d_dense, d_count, d_offset, d_tmp, d_total, d_pairs;
    d_U.alloc((size_t)n_groups * kWordsPerGroup * n_pad * 4, live, peak);
    {
        DevBuf d_rows;
        d_rows.alloc((size_t)nn * mm, live, peak);
        MGTA_HIP_CHECK(hipMemcpyAsync(d_rows.p, rows, (size_t)nn * mm, hipMemcpyHostToDevice, st));
        const uint64_t threads = (uint64_t)n_groups * n_pad;
        if ((threads + 255) / 256 > 0x7FFFFFFFull) {                      // (rows of that size do not fit any device: the allocations above fail first)
            set_error("%s: %lld rows of %lld columns are more than one launch lays out", who, (long long)n, (long long)M);
            return (int)MGTA_ENOMEM;
        }
        t_a.start();
        hipLaunchKernelGGL(cluster_layout_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, d_rows.as<uint8_t>(), nn, mm, n_groups, n_pad, d_U.as<uint32_t>());
        MGTA_HIP_CHECK(hipGetLastError());
        t_a.end();
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        ms += t_a.ms();
    }
    d_dense.alloc((size_t)ld * ld * 4, live, peak);
    d_count.alloc((size_t)side * 4, live, peak);
    d_offset.alloc((size_t)side * 8, live, peak);
    d_tmp.alloc((size_t)scan_tmp_elems(side) * 8, live, peak);
    d_total.alloc(8, live, peak);

    int blocks_per_cu = 0;
    MGTA_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, cluster_pairs_kernel, kPairThreads, 0));
    int64_t total = 0, n_tiles = 0, max_grid = 0;
    std::vector<std::vector<mgta_row_pair>> part;                         // the tiles of one block I, and where their rows start
    std::vector<std::vector<uint64_t>> part_off;
    auto no_room = [&](int64_t found) {
        set_error("%s: the kept pairs do not fit the memory the call may use: %lld found so far", who, (long long)found);
        return (int)MGTA_ENOMEM;
    };
    for (uint64_t i0 = 0; i0 < nn; i0 += R) {
        const uint32_t n_rows = (uint32_t)std::min<uint64_t>(R, nn - i0);
        part.clear(); part_off.clear();
        for (uint64_t j0 = i0; j0 < nn; j0 += R) {
            const uint32_t n_cols = (uint32_t)std::min<uint64_t>(R, nn - j0);
            PairArgs pa;
            pa.U = d_U.as<uint32_t>(); pa.n_pad = n_pad; pa.n = nn; pa.n_groups = n_groups; pa.i0 = (uint32_t)i0; pa.j0 = (uint32_t)j0; pa.ld = ld;
            pa.min_overlap = (uint32_t)std::min<int64_t>(min_overlap, kMaxColumns); pa.cutoff = cutoff; pa.dense = d_dense.as<uint32_t>();
            const dim3 grid((n_cols + kTileSide - 1) / kTileSide, (n_rows + kTileSide - 1) / kTileSide);
            t_a.start();
            hipLaunchKernelGGL(cluster_pairs_kernel, grid, dim3(kPairThreads), 0, st, pa);
            hipLaunchKernelGGL(cluster_count_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, st, d_dense.as<uint32_t>(), ld, n_rows, n_cols, (uint32_t)i0, (uint32_t)j0,
                               d_count.as<uint32_t>());
            exclusive_scan_u32(st, d_count.as<uint32_t>(), n_rows, d_offset.as<uint64_t>(), d_tmp.as<uint64_t>(), d_total.as<uint64_t>());
            MGTA_HIP_CHECK(hipGetLastError());
            t_a.end();
            uint64_t tile_total = 0;
            MGTA_HIP_CHECK(hipMemcpyAsync(&tile_total, d_total.p, 8, hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
            ms += t_a.ms();
            ++n_tiles; max_grid = std::max<int64_t>(max_grid, (int64_t)grid.x * grid.y);
            total += (int64_t)tile_total;
            if (!out || tile_total == 0) continue;
            const size_t bytes = (size_t)tile_total * sizeof(mgta_row_pair);
            if (d_pairs.bytes < bytes) {
                d_pairs.release();
                if (ctx->mem_limit && *live + bytes > ctx->mem_limit) return no_room(total);
                try { d_pairs.alloc(bytes, live, peak); }
                catch (const HipError &e) { if (e.code == MGTA_ENOMEM) return no_room(total); throw; }
            }
            t_b.start();
            hipLaunchKernelGGL(cluster_write_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, st, d_dense.as<uint32_t>(), ld, n_rows, n_cols, (uint32_t)i0, (uint32_t)j0,
                               d_offset.as<uint64_t>(), d_pairs.as<mgta_row_pair>());
            MGTA_HIP_CHECK(hipGetLastError());
            t_b.end();
            try {
                part.emplace_back((size_t)tile_total);
                part_off.emplace_back((size_t)n_rows + 1);
            } catch (const std::bad_alloc &) { return no_room(total); }
            MGTA_HIP_CHECK(hipMemcpyAsync(part.back().data(), d_pairs.p, bytes, hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipMemcpyAsync(part_off.back().data(), d_offset.p, (size_t)n_rows * 8, hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
            part_off.back()[n_rows] = tile_total;
            ms += t_b.ms();
        }
        if (!out) continue;
        // the rows of block I in order, every row's pairs tile after tile: sorted by (i, j)
        try {
            if (part.size() == 1) out->insert(out->end(), part[0].begin(), part[0].end());
            else
                for (uint32_t r = 0; r < n_rows; ++r)
                    for (size_t t = 0; t < part.size(); ++t) out->insert(out->end(), part[t].begin() + (ptrdiff_t)part_off[t][r], part[t].begin() + (ptrdiff_t)part_off[t][r + 1]);
        } catch (const std::bad_alloc &) { return no_room(total); }
    }
    *n_pairs = total;
    if (stats) {
        stats->n_rows = n; stats->n_pairs_kept = total; stats->n_tiles = n_tiles; stats->blocks_per_cu = blocks_per_cu; stats->grid_blocks = max_grid;
        stats->lds_bytes = 2 * kStageWords * kTileSide * 4; stats->peak_bytes = (int64_t)*peak; stats->ms_pairs = ms;
    }
    return (int)MGTA_OK;
}

int check_rows(const char *who, mgta_ctx *ctx, const uint8_t *rows, int64_t n, int64_t M, int64_t min_overlap, double cutoff) {
    if (!ctx) { set_error("%s: ctx must not be NULL", who); return MGTA_EINVAL; }
    if (n < 0) { set_error("%s: n = %lld must not be negative", who, (long long)n); return MGTA_EINVAL; }
    if (n >= (1ll << 31)) { set_error("%s: n = %lld (the limit is n < 2^31 rows)", who, (long long)n); return MGTA_EINVAL; }
    if (M < 1 || M >= kMaxColumns) { set_error("%s: M = %lld (the limit is 1 <= M < 65536 columns)", who, (long long)M); return MGTA_EINVAL; }
    if (min_overlap < 1) { set_error("%s: min_overlap = %lld must be at least 1", who, (long long)min_overlap); return MGTA_EINVAL; }
    if (!(cutoff >= 0.0 && cutoff <= 1.0)) { set_error("%s: cutoff = %g must lie in [0, 1]", who, cutoff); return MGTA_EINVAL; }
    if (n > 0 && !rows) { set_error("%s: rows must not be NULL", who); return MGTA_EINVAL; }
    return MGTA_OK;
}

// ---- complete linkage over the kept pairs ---------------------------------------------------------------------------------------------
struct Frac { uint32_t d, o; };                                          // n_diff / n_overlap, o >= 1
inline bool frac_less(Frac a, Frac b) { return (uint64_t)a.d * b.o < (uint64_t)b.d * a.o; }

struct Cand { Frac f; uint32_t a, b, va, vb; };                          // clusters a < b (their lowest members) at versions va, vb
struct CandAfter {                                                       // the heap's top is the smallest (distance, a, b)
    bool operator()(const Cand &x, const Cand &y) const {
        if (frac_less(x.f, y.f)) return false;
        if (frac_less(y.f, x.f)) return true;
        return x.a != y.a ? x.a > y.a : x.b > y.b;
    }
};

// one component: members 0 .. m - 1 in row order, its pairs (u < v) in those numbers; into[x] = the cluster x went into (itself: a name)
void link_component(uint32_t m, const std::vector<uint32_t> &pu, const std::vector<uint32_t> &pv, const std::vector<Frac> &pf, std::vector<uint32_t> &into,
                    int64_t &n_pops) {
    into.resize(m);
    std::iota(into.begin(), into.end(), 0u);
    if (m < 2) return;
    auto key = [](uint32_t x, uint32_t y) { return x < y ? ((uint64_t)x << 32 | y) : ((uint64_t)y << 32 | x); };
    std::unordered_map<uint64_t, Frac> dist;                             // the pairs of clusters whose cross pairs are all kept
    dist.reserve(pu.size() * 2);
    std::vector<std::vector<uint32_t>> nbr(m);                           // who a cluster may be linkable to (dist decides)
    std::vector<uint32_t> ver(m, 0);
    std::vector<uint8_t> alive(m, 1);
    std::priority_queue<Cand, std::vector<Cand>, CandAfter> heap;
    for (size_t e = 0; e < pu.size(); ++e) {
        dist.emplace(key(pu[e], pv[e]), pf[e]);
        nbr[pu[e]].push_back(pv[e]);
        nbr[pv[e]].push_back(pu[e]);
        heap.push(Cand{pf[e], pu[e], pv[e], 0, 0});
    }
    std::vector<uint32_t> keep;
    while (!heap.empty()) {
        const Cand c = heap.top();
        heap.pop();
        ++n_pops;
        if (!alive[c.a] || !alive[c.b] || ver[c.a] != c.va || ver[c.b] != c.vb) continue;
        const uint32_t a = c.a, b = c.b;                                  // b goes into a, the lower name
        keep.clear();
        for (uint32_t x : nbr[a]) {
            if (x == b || !alive[x]) continue;
            auto ia = dist.find(key(a, x));
            if (ia == dist.end()) continue;
            auto ib = dist.find(key(b, x));
            if (ib == dist.end()) { dist.erase(ia); continue; }
            if (frac_less(ia->second, ib->second)) ia->second = ib->second;
            keep.push_back(x);
        }
        for (uint32_t x : nbr[b]) dist.erase(key(b, x));
        nbr[b].clear(); nbr[b].shrink_to_fit();
        alive[b] = 0;
        into[b] = a;
        ++ver[a];
        nbr[a] = keep;
        for (uint32_t x : keep) {
            const Frac f = dist.find(key(a, x))->second;
            if (a < x) heap.push(Cand{f, a, x, ver[a], ver[x]});
            else heap.push(Cand{f, x, a, ver[x], ver[a]});
        }
    }
}

struct ClusterCounts { int64_t n_unaligned, n_clusters, n_singletons, largest; };

// name[i] = the lowest row of i's cluster -> the four outputs: numbers by the lowest member, the representative by lens then index
ClusterCounts number_clusters(const mgta_row_pair *P, size_t n_pairs, const uint32_t *n_res, const int64_t *lens, uint32_t nn, const std::vector<uint32_t> &name,
                              int32_t *cluster, int64_t *rep, uint16_t *rep_diff, uint16_t *rep_overlap) {
    const uint32_t kNone = 0xFFFFFFFFu;
    std::vector<int32_t> number(nn, -1);
    std::vector<uint32_t> best(nn, kNone), csize(nn, 0);
    int32_t n_clusters = 0;
    for (uint32_t i = 0; i < nn; ++i) {
        if (n_res[i] == 0) continue;
        const uint32_t c = name[i];
        if (c == i) number[i] = n_clusters++;
        ++csize[c];
        if (best[c] == kNone || lens[i] > lens[best[c]]) best[c] = i;
    }
    int64_t n_unaligned = 0, n_singletons = 0, largest = 0;
    for (uint32_t i = 0; i < nn; ++i) {
        if (n_res[i] == 0) { cluster[i] = -1; rep[i] = -1; rep_diff[i] = 0; rep_overlap[i] = 0; ++n_unaligned; continue; }
        const uint32_t c = name[i];
        cluster[i] = number[c];
        rep[i] = (int64_t)best[c];
        rep_diff[i] = 0;
        rep_overlap[i] = (uint16_t)n_res[i];                          // the representative's own; a member's comes from its pair below
        if (c == i) { n_singletons += csize[c] == 1; largest = std::max<int64_t>(largest, csize[c]); }
    }
    for (size_t e_ = 0; e_ < n_pairs; ++e_) {
        const mgta_row_pair &p = P[e_];
        if (rep[p.i] == (int64_t)p.j) { rep_diff[p.i] = p.n_diff; rep_overlap[p.i] = p.n_overlap; }
        if (rep[p.j] == (int64_t)p.i) { rep_diff[p.j] = p.n_diff; rep_overlap[p.j] = p.n_overlap; }
    }
    return ClusterCounts{n_unaligned, (int64_t)n_clusters, n_singletons, largest};
}

// the clusters of nn rows from their kept pairs (sorted by (i, j)), the residue columns of every row and the lengths; fills the
// linkage's fields of *stats and leaves the others alone
int link_rows(const char *who, const mgta_row_pair *P, size_t n_pairs, const uint32_t *n_res, const int64_t *lens, uint32_t nn, int32_t *cluster, int64_t *rep,
              uint16_t *rep_diff, uint16_t *rep_overlap, mgta_cluster_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t kNone = 0xFFFFFFFFu;
    if (n_pairs >= (size_t)kNone) { set_error("%s: %zu kept pairs (the linkage holds fewer than 2^32)", who, n_pairs); return (int)MGTA_ENOMEM; }

    // components of the kept-pair graph: the root of a component is its lowest row
    std::vector<uint32_t> root(nn);
    std::iota(root.begin(), root.end(), 0u);
    auto find = [&](uint32_t x) {
        while (root[x] != x) { root[x] = root[root[x]]; x = root[x]; }
        return x;
    };
    for (size_t e_ = 0; e_ < n_pairs; ++e_) {
        const mgta_row_pair &p = P[e_];
        const uint32_t a = find((uint32_t)p.i), b = find((uint32_t)p.j);
        if (a != b) root[std::max(a, b)] = std::min(a, b);
    }
    for (uint32_t i = 0; i < nn; ++i) root[i] = root[root[i]];      // root[i] <= i, so root[root[i]] is final already: every path is one step now
    // members of a component in row order, a row's number inside it, and the pairs of every component together
    std::vector<uint32_t> local(nn), size(nn, 0);
    for (uint32_t i = 0; i < nn; ++i) local[i] = size[root[i]]++;
    std::vector<uint64_t> first(nn + 1ull, 0);
    for (size_t e_ = 0; e_ < n_pairs; ++e_) ++first[root[(uint32_t)P[e_].i] + 1ull];
    for (uint32_t i = 0; i < nn; ++i) first[i + 1ull] += first[i];
    std::vector<uint32_t> order(n_pairs);
    {
        std::vector<uint64_t> next(first.begin(), first.end() - 1);
        for (size_t e = 0; e < n_pairs; ++e) order[next[root[(uint32_t)P[e].i]]++] = (uint32_t)e;
    }

    // link every component; name[i] = the lowest row of i's cluster
    std::vector<uint32_t> name(nn);
    std::iota(name.begin(), name.end(), 0u);

    std::vector<uint32_t> pu, pv, into;
    std::vector<Frac> pf;
    int64_t n_pops = 0, n_components = 0;
    std::vector<uint64_t> member_first(nn + 1ull, 0);
    for (uint32_t i = 0; i < nn; ++i) member_first[root[i] + 1ull]++;
    for (uint32_t i = 0; i < nn; ++i) member_first[i + 1ull] += member_first[i];
    std::vector<uint32_t> member(nn);
    {
        std::vector<uint64_t> next(member_first.begin(), member_first.end() - 1);
        for (uint32_t i = 0; i < nn; ++i) member[next[root[i]]++] = i;
    }
    for (uint32_t c = 0; c < nn; ++c) {
        if (root[c] != c || n_res[c] == 0) continue;                  // (a row without residues has no pair: a component of its own, not counted)
        ++n_components;
        const uint64_t e0 = first[c], e1 = first[c + 1ull];
        if (e0 == e1) continue;
        pu.clear(); pv.clear(); pf.clear();
        for (uint64_t e = e0; e < e1; ++e) {
            const mgta_row_pair &p = P[order[e]];
            pu.push_back(local[(uint32_t)p.i]); pv.push_back(local[(uint32_t)p.j]); pf.push_back(Frac{p.n_diff, p.n_overlap});
        }
        link_component(size[c], pu, pv, pf, into, n_pops);
        const uint32_t *mem = member.data() + member_first[c];
        for (uint32_t x = 0; x < size[c]; ++x) {
            uint32_t y = x;
            while (into[y] != y) y = into[y];
            name[mem[x]] = mem[y];
        }
    }

    const ClusterCounts cc = number_clusters(P, n_pairs, n_res, lens, nn, name, cluster, rep, rep_diff, rep_overlap);
    if (stats) {
        stats->n_rows = nn; stats->n_pairs_kept = (int64_t)n_pairs;
        stats->n_unaligned = cc.n_unaligned; stats->n_clusters = cc.n_clusters; stats->n_singletons = cc.n_singletons; stats->largest_cluster = cc.largest;
        stats->n_components = n_components; stats->n_link_pops = n_pops;
        stats->ms_link = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return (int)MGTA_OK;
}

// ---- the merge tree: what the host does around cluster_tree.hpp ------------------------------------------------------------------------
// the pair list of mgta_pairs_link and of the tree entries: every message names `who`
int check_pair_list(const char *who, const mgta_row_pair *pairs, int64_t n_pairs, const int32_t *n_residues, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (n_residues[i] < 0 || n_residues[i] >= kMaxColumns) { set_error("%s: n_residues[%lld] = %d (0 .. 65535)", who, (long long)i, n_residues[i]); return MGTA_EINVAL; }
    for (int64_t e = 0; e < n_pairs; ++e) {
        const mgta_row_pair &p = pairs[e];
        if (p.i < 0 || p.i >= p.j || p.j >= n || p.n_overlap < 1 || p.n_diff > p.n_overlap || n_residues[p.i] == 0 || n_residues[p.j] == 0) {
            set_error("%s: pair %lld = (%d, %d, %u / %u): 0 <= i < j < n, 1 <= n_overlap, n_diff <= n_overlap, both rows with residues", who, (long long)e, p.i, p.j,
                      (unsigned)p.n_diff, (unsigned)p.n_overlap);
            return MGTA_EINVAL;
        }
        if (e > 0 && !(pairs[e - 1].i < p.i || (pairs[e - 1].i == p.i && pairs[e - 1].j < p.j))) {
            set_error("%s: pair %lld: the pairs must ascend by (i, j)", who, (long long)e);
            return MGTA_EINVAL;
        }
    }
    return MGTA_OK;
}

// what the device found -> the list of the contract: fractions in lowest terms, ascending by (fraction, a, b)
void finish_merges(const std::vector<TreeMerge> &found, std::vector<mgta_tree_merge> &out) {
    out.clear();
    out.reserve(found.size());
    for (const TreeMerge &m : found) {
        const uint32_t d = m.f >> 16, o = m.f & 0xFFFFu, g = d ? std::gcd(d, o) : o;
        out.push_back(mgta_tree_merge{(int32_t)m.a, (int32_t)m.b, (uint16_t)(d / g), (uint16_t)(o / g)});
    }
    std::sort(out.begin(), out.end(), [](const mgta_tree_merge &x, const mgta_tree_merge &y) {
        const Frac fx{x.n_diff, x.n_overlap}, fy{y.n_diff, y.n_overlap};
        if (frac_less(fx, fy)) return true;
        if (frac_less(fy, fx)) return false;
        return x.a != y.a ? x.a < y.a : x.b < y.b;
    });
}

// one cut of the tree (the caller has checked pairs, merges and the rest); adds to n_cut_fallbacks and ms_cut, sets the counts of the cut
int cut_rows(const char *who, const mgta_row_pair *P, size_t n_pairs, const mgta_tree_merge *T, size_t n_merges, const uint32_t *n_res, const int64_t *lens, uint32_t nn,
             double cutoff, int32_t *cluster, int64_t *rep, uint16_t *rep_diff, uint16_t *rep_overlap, mgta_tree_stats *st) {
    const auto t0 = std::chrono::steady_clock::now();
    bool any_kept = false, any_apart = false;
    Frac hi{0, 1}, lo{0, 1};
    size_t n_kept = 0;
    for (size_t e = 0; e < n_pairs; ++e) {
        const Frac f{P[e].n_diff, P[e].n_overlap};
        if ((double)f.d <= cutoff * (double)f.o) {
            if (!any_kept || frac_less(hi, f)) hi = f;
            any_kept = true; ++n_kept;
        } else {
            if (!any_apart || frac_less(f, lo)) lo = f;
            any_apart = true;
        }
    }
    ClusterCounts cc;
    if (!any_apart || !any_kept || frac_less(hi, lo)) {
        // the merges up to hi: b goes into a < b, and every row above its cluster's name was a `b` once
        std::vector<uint32_t> name(nn);
        std::iota(name.begin(), name.end(), 0u);
        if (any_kept)
            for (size_t m = 0; m < n_merges; ++m)
                if (!frac_less(hi, Frac{T[m].n_diff, T[m].n_overlap})) name[(uint32_t)T[m].b] = (uint32_t)T[m].a;
        for (uint32_t i = 0; i < nn; ++i) name[i] = name[name[i]];       // name[i] <= i is final already
        cc = number_clusters(P, n_pairs, n_res, lens, nn, name, cluster, rep, rep_diff, rep_overlap);
    } else {
        std::vector<mgta_row_pair> kept;
        kept.reserve(n_kept);
        for (size_t e = 0; e < n_pairs; ++e)
            if ((double)P[e].n_diff <= cutoff * (double)P[e].n_overlap) kept.push_back(P[e]);
        mgta_cluster_stats cs;
        memset(&cs, 0, sizeof cs);
        const int r = link_rows(who, kept.data(), kept.size(), n_res, lens, nn, cluster, rep, rep_diff, rep_overlap, &cs);
        if (r != MGTA_OK) return r;
        cc = ClusterCounts{cs.n_unaligned, cs.n_clusters, cs.n_singletons, cs.largest_cluster};
        if (st) ++st->n_cut_fallbacks;
    }
    if (st) {
        st->n_unaligned = cc.n_unaligned; st->n_clusters = cc.n_clusters; st->n_singletons = cc.n_singletons; st->largest_cluster = cc.largest;
        st->ms_cut += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return (int)MGTA_OK;
}

int check_merges(const char *who, const mgta_tree_merge *T, int64_t n_merges, const int32_t *n_residues, int64_t n) {
    if (n_merges < 0 || n_merges > std::max<int64_t>(0, n - 1)) { set_error("%s: n_merges = %lld (0 .. n - 1)", who, (long long)n_merges); return MGTA_EINVAL; }
    if (n_merges > 0 && !T) { set_error("%s: merges must not be NULL", who); return MGTA_EINVAL; }
    std::vector<uint8_t> gone((size_t)n, 0);
    for (int64_t m = 0; m < n_merges; ++m) {
        const mgta_tree_merge &t = T[m];
        if (t.a < 0 || t.a >= t.b || t.b >= n || t.n_overlap < 1 || t.n_diff > t.n_overlap || n_residues[t.a] == 0 || n_residues[t.b] == 0 || gone[(size_t)t.b]) {
            set_error("%s: merge %lld = (%d, %d, %u / %u): 0 <= a < b < n, 1 <= n_overlap, n_diff <= n_overlap, both rows with residues, b merged once", who, (long long)m,
                      t.a, t.b, (unsigned)t.n_diff, (unsigned)t.n_overlap);
            return MGTA_EINVAL;
        }
        gone[(size_t)t.b] = 1;
        if (m > 0 && frac_less(Frac{t.n_diff, t.n_overlap}, Frac{T[m - 1].n_diff, T[m - 1].n_overlap})) {
            set_error("%s: merge %lld: the merges must ascend by their fraction", who, (long long)m);
            return MGTA_EINVAL;
        }
    }
    return MGTA_OK;
}

std::vector<uint32_t> residue_columns(const uint8_t *rows, uint32_t nn, int64_t M) {
    std::vector<uint32_t> n_res(nn);
    for (uint32_t i = 0; i < nn; ++i) {
        const uint8_t *p = rows + (size_t)i * (size_t)M;
        uint32_t c = 0;
        for (int64_t k = 0; k < M; ++k) c += p[k] != (uint8_t)'-';
        n_res[i] = c;
    }
    return n_res;
}

}  // namespace
}  // namespace mgta

using namespace mgta;

extern "C" {

int mgta_ctx_set_cluster_tile(mgta_ctx *ctx, int64_t rows_per_tile) {
    if (!ctx) { set_error("mgta_ctx_set_cluster_tile: ctx must not be NULL"); return MGTA_EINVAL; }
    if (rows_per_tile < 0 || rows_per_tile > 32768) { set_error("mgta_ctx_set_cluster_tile: rows_per_tile = %lld (0 .. 32768)", (long long)rows_per_tile); return MGTA_EINVAL; }
    ctx->cluster_tile_rows = (uint64_t)rows_per_tile;
    return MGTA_OK;
}

int mgta_rows_pairs(mgta_ctx *ctx, const uint8_t *rows, int64_t n, int64_t M, int64_t min_overlap, double cutoff, mgta_row_pair *pairs, int64_t cap, int64_t *n_pairs,
                    mgta_cluster_stats *stats) {
    const char *who = "mgta_rows_pairs";
    const int rc = check_rows(who, ctx, rows, n, M, min_overlap, cutoff);
    if (rc != MGTA_OK) return rc;
    if (cap < 0) { set_error("%s: cap = %lld must not be negative", who, (long long)cap); return MGTA_EINVAL; }
    if (cap > 0 && !pairs) { set_error("%s: pairs must not be NULL when cap > 0", who); return MGTA_EINVAL; }
    if (!n_pairs) { set_error("%s: n_pairs must not be NULL", who); return MGTA_EINVAL; }
    if (stats) memset(stats, 0, sizeof(*stats));
    *n_pairs = 0;
    if (n == 0) return MGTA_OK;
    return guarded(who, [&]() {
        std::vector<mgta_row_pair> found;
        int64_t count = 0;
        const int r = pairs_impl(ctx, who, rows, n, M, min_overlap, cutoff, cap > 0 ? &found : nullptr, &count, stats);
        if (r != MGTA_OK) return r;
        *n_pairs = count;
        if (cap > 0 && count <= cap && count > 0) memcpy(pairs, found.data(), (size_t)count * sizeof(mgta_row_pair));
        return (int)MGTA_OK;
    });
}

int mgta_rows_cluster(mgta_ctx *ctx, const uint8_t *rows, const int64_t *lens, int64_t n, int64_t M, int64_t min_overlap, double cutoff, int32_t *cluster, int64_t *rep,
                      uint16_t *rep_diff, uint16_t *rep_overlap, mgta_cluster_stats *stats) {
    const char *who = "mgta_rows_cluster";
    const int rc = check_rows(who, ctx, rows, n, M, min_overlap, cutoff);
    if (rc != MGTA_OK) return rc;
    if (n > 0 && !lens) { set_error("%s: lens must not be NULL", who); return MGTA_EINVAL; }
    if (n > 0 && (!cluster || !rep || !rep_diff || !rep_overlap)) { set_error("%s: cluster, rep, rep_diff and rep_overlap must not be NULL", who); return MGTA_EINVAL; }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return MGTA_OK;
    return guarded(who, [&]() {
        std::vector<mgta_row_pair> P;
        int64_t count = 0;
        mgta_cluster_stats s;
        memset(&s, 0, sizeof s);
        const int r = pairs_impl(ctx, who, rows, n, M, min_overlap, cutoff, &P, &count, &s);
        if (r != MGTA_OK) return r;
        const uint32_t nn = (uint32_t)n;
        const std::vector<uint32_t> n_res = residue_columns(rows, nn, M);   // a row without any is in no cluster
        if (stats) *stats = s;
        return link_rows(who, P.data(), P.size(), n_res.data(), lens, nn, cluster, rep, rep_diff, rep_overlap, stats);
    });
}

int mgta_pairs_link(const mgta_row_pair *pairs, int64_t n_pairs, const int32_t *n_residues, const int64_t *lens, int64_t n, int32_t *cluster, int64_t *rep,
                    uint16_t *rep_diff, uint16_t *rep_overlap, mgta_cluster_stats *stats) {
    const char *who = "mgta_pairs_link";
    if (n < 0 || n >= (1ll << 31)) { set_error("%s: n = %lld (0 <= n < 2^31 rows)", who, (long long)n); return MGTA_EINVAL; }
    if (n_pairs < 0) { set_error("%s: n_pairs = %lld must not be negative", who, (long long)n_pairs); return MGTA_EINVAL; }
    if (n_pairs > 0 && !pairs) { set_error("%s: pairs must not be NULL", who); return MGTA_EINVAL; }
    if (n > 0 && (!n_residues || !lens)) { set_error("%s: n_residues and lens must not be NULL", who); return MGTA_EINVAL; }
    if (n > 0 && (!cluster || !rep || !rep_diff || !rep_overlap)) { set_error("%s: cluster, rep, rep_diff and rep_overlap must not be NULL", who); return MGTA_EINVAL; }
    const int rc = check_pair_list(who, pairs, n_pairs, n_residues, n);
    if (rc != MGTA_OK) return rc;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return MGTA_OK;
    return guarded(who, [&]() {
        std::vector<uint32_t> n_res((size_t)n);
        for (int64_t i = 0; i < n; ++i) n_res[(size_t)i] = (uint32_t)n_residues[i];
        return link_rows(who, pairs, (size_t)n_pairs, n_res.data(), lens, (uint32_t)n, cluster, rep, rep_diff, rep_overlap, stats);
    });
}

int mgta_pairs_tree(mgta_ctx *ctx, const mgta_row_pair *pairs, int64_t n_pairs, const int32_t *n_residues, int64_t n, mgta_tree_merge *merges, int64_t cap,
                    int64_t *n_merges, mgta_tree_stats *stats) {
    const char *who = "mgta_pairs_tree";
    if (!ctx) { set_error("%s: ctx must not be NULL", who); return MGTA_EINVAL; }
    if (n < 0 || n >= (1ll << 31)) { set_error("%s: n = %lld (0 <= n < 2^31 rows)", who, (long long)n); return MGTA_EINVAL; }
    if (n_pairs < 0) { set_error("%s: n_pairs = %lld must not be negative", who, (long long)n_pairs); return MGTA_EINVAL; }
    if (n_pairs > 0 && !pairs) { set_error("%s: pairs must not be NULL", who); return MGTA_EINVAL; }
    if (n > 0 && !n_residues) { set_error("%s: n_residues must not be NULL", who); return MGTA_EINVAL; }
    if (cap < 0) { set_error("%s: cap = %lld must not be negative", who, (long long)cap); return MGTA_EINVAL; }
    if (cap > 0 && !merges) { set_error("%s: merges must not be NULL when cap > 0", who); return MGTA_EINVAL; }
    if (!n_merges) { set_error("%s: n_merges must not be NULL", who); return MGTA_EINVAL; }
    const int rc = check_pair_list(who, pairs, n_pairs, n_residues, n);
    if (rc != MGTA_OK) return rc;
    if (stats) memset(stats, 0, sizeof(*stats));
    *n_merges = 0;
    if (n == 0) return MGTA_OK;
    return guarded(who, [&]() {
        mgta_tree_stats s;
        memset(&s, 0, sizeof s);
        std::vector<TreeMerge> found;
        const int r = tree_impl(ctx, who, pairs, (uint64_t)n_pairs, (uint32_t)n, found, &s);
        if (r != MGTA_OK) return r;
        std::vector<mgta_tree_merge> T;
        finish_merges(found, T);
        s.n_rows = n; s.n_pairs = n_pairs; s.n_merges = (int64_t)T.size();
        *n_merges = (int64_t)T.size();
        if (!T.empty() && (int64_t)T.size() <= cap) memcpy(merges, T.data(), T.size() * sizeof(mgta_tree_merge));
        if (stats) *stats = s;
        return (int)MGTA_OK;
    });
}

int mgta_tree_cut(const mgta_row_pair *pairs, int64_t n_pairs, const mgta_tree_merge *merges, int64_t n_merges, const int32_t *n_residues, const int64_t *lens, int64_t n,
                  double cutoff, int32_t *cluster, int64_t *rep, uint16_t *rep_diff, uint16_t *rep_overlap, mgta_tree_stats *stats) {
    const char *who = "mgta_tree_cut";
    if (n < 0 || n >= (1ll << 31)) { set_error("%s: n = %lld (0 <= n < 2^31 rows)", who, (long long)n); return MGTA_EINVAL; }
    if (n_pairs < 0) { set_error("%s: n_pairs = %lld must not be negative", who, (long long)n_pairs); return MGTA_EINVAL; }
    if (n_pairs > 0 && !pairs) { set_error("%s: pairs must not be NULL", who); return MGTA_EINVAL; }
    if (n > 0 && (!n_residues || !lens)) { set_error("%s: n_residues and lens must not be NULL", who); return MGTA_EINVAL; }
    if (n > 0 && (!cluster || !rep || !rep_diff || !rep_overlap)) { set_error("%s: cluster, rep, rep_diff and rep_overlap must not be NULL", who); return MGTA_EINVAL; }
    if (!(cutoff >= 0.0 && cutoff <= 1.0)) { set_error("%s: cutoff = %g must lie in [0, 1]", who, cutoff); return MGTA_EINVAL; }
    int rc = check_pair_list(who, pairs, n_pairs, n_residues, n);
    if (rc != MGTA_OK) return rc;
    rc = check_merges(who, merges, n_merges, n_residues, n);
    if (rc != MGTA_OK) return rc;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return MGTA_OK;
    return guarded(who, [&]() {
        std::vector<uint32_t> n_res((size_t)n);
        for (int64_t i = 0; i < n; ++i) n_res[(size_t)i] = (uint32_t)n_residues[i];
        if (stats) { stats->n_rows = n; stats->n_pairs = n_pairs; stats->n_merges = n_merges; }
        return cut_rows(who, pairs, (size_t)n_pairs, merges, (size_t)n_merges, n_res.data(), lens, (uint32_t)n, cutoff, cluster, rep, rep_diff, rep_overlap, stats);
    });
}

int mgta_rows_clusters(mgta_ctx *ctx, const uint8_t *rows, const int64_t *lens, int64_t n, int64_t M, int64_t min_overlap, const double *cutoffs, int64_t n_cutoffs,
                       int32_t *cluster, int64_t *rep, uint16_t *rep_diff, uint16_t *rep_overlap, mgta_tree_merge *merges, int64_t *n_merges, mgta_tree_stats *stats) {
    const char *who = "mgta_rows_clusters";
    if (n_cutoffs < 1 || !cutoffs) { set_error("%s: n_cutoffs = %lld: at least one cut-off, cutoffs must not be NULL", who, (long long)n_cutoffs); return MGTA_EINVAL; }
    double D = 0.0;
    for (int64_t k = 0; k < n_cutoffs; ++k) {
        const int rc = check_rows(who, ctx, rows, n, M, min_overlap, cutoffs[k]);
        if (rc != MGTA_OK) return rc;
        D = std::max(D, cutoffs[k]);
    }
    if (n > 0 && !lens) { set_error("%s: lens must not be NULL", who); return MGTA_EINVAL; }
    if (n > 0 && (!cluster || !rep || !rep_diff || !rep_overlap)) { set_error("%s: cluster, rep, rep_diff and rep_overlap must not be NULL", who); return MGTA_EINVAL; }
    if (merges && !n_merges) { set_error("%s: n_merges must not be NULL when merges is given", who); return MGTA_EINVAL; }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_merges) *n_merges = 0;
    if (n == 0) return MGTA_OK;
    return guarded(who, [&]() {
        std::vector<mgta_row_pair> P;
        int64_t count = 0;
        mgta_cluster_stats ps;
        memset(&ps, 0, sizeof ps);
        int r = pairs_impl(ctx, who, rows, n, M, min_overlap, D, &P, &count, &ps);
        if (r != MGTA_OK) return r;
        const uint32_t nn = (uint32_t)n;
        const std::vector<uint32_t> n_res = residue_columns(rows, nn, M);
        mgta_tree_stats s;
        memset(&s, 0, sizeof s);
        std::vector<TreeMerge> found;
        r = tree_impl(ctx, who, P.data(), P.size(), nn, found, &s);
        if (r != MGTA_OK) return r;
        std::vector<mgta_tree_merge> T;
        finish_merges(found, T);
        s.n_rows = n; s.n_pairs = count; s.n_merges = (int64_t)T.size(); s.ms_pairs = ps.ms_pairs; s.peak_bytes = std::max<int64_t>(s.peak_bytes, ps.peak_bytes);
        for (int64_t k = 0; k < n_cutoffs; ++k) {
            r = cut_rows(who, P.data(), P.size(), T.data(), T.size(), n_res.data(), lens, nn, cutoffs[k], cluster + k * n, rep + k * n, rep_diff + k * n, rep_overlap + k * n, &s);
            if (r != MGTA_OK) return r;
        }
        if (n_merges) *n_merges = (int64_t)T.size();
        if (merges && !T.empty()) memcpy(merges, T.data(), T.size() * sizeof(mgta_tree_merge));
        if (stats) *stats = s;
        return (int)MGTA_OK;
    });
}

}  // extern "C"
