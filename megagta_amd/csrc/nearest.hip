// nearest.hip — the closest reference protein of every contig (mgta_seqs_nearest): the place of FrameBot / `AlignmentTool pairwise-knn`
// in the reference's bin/post_proc.sh:106-111.  The rule is this library's own (include/megagta_hip.h): three-state pairwise dynamic
// programming over match / insert / delete, global in the contig, local in the reference, int32, first candidate wins a tie.
//
// Sweep (nearest_sweep_kernel).  The references are one run of columns: column g is residue g of their concatenation, and one byte per
// column holds its residue class and whether it is the first column of its reference.  The host cuts the run, at reference boundaries,
// into segments (one when there are contigs enough to fill the device); a work item is (contig, segment), items are taken longest
// contig first from one atomic head, one wave owns an item.  Lanes own columns, 64 at a time (a strip); at step t of a strip lane l
// computes row i = t - l + 1 of its column, so the cells of one anti-diagonal are computed together.  The recurrence is written from
// the cell outwards: the lane of cell (i, j) computes what its neighbours need,
//     D = max(M, X, Y)[i][j]                  the candidate of M[i+1][j+1]  (taken by lane l + 1 two steps later)
//     Y' = max(M[i][j] - go, Y[i][j] - ge)    Y[i][j+1]                     (taken by lane l + 1 at the next step)
//     X' = max(M[i][j] - go, X[i][j] - ge)    X[i+1][j]                     (its own next step)
// D, Y' and the contig's residue class move to lane l + 1 by one DPP wave shift each (v_mov_b32 wave_shr:1, no LDS); lane 0 takes
// them from LDS instead: the contig's classes, and per row what lane 63 of the strip before left there (one wave, LDS in program
// order: row t is read before the rows <= t - 63 are written, in place).  A lane whose column is the first of its reference takes
// "undefined" for D and Y', so nothing crosses a reference boundary and a strip carries no per-reference bubble.  `sub` sits in LDS,
// 32 bytes per reference class.  A lane whose row is L keeps the best (score, lowest column) in registers; one wave reduction per
// item gives the key (score biased) << 32 | ~column, and the largest key of a contig's items names highest score, lowest reference
// and lowest end column at once.  No atomics on the hot path and no dependence on any order.
//   MODE 0  the score pass.
//   MODE 1  the score pass that also fills `scores`: the lane of row L raises scores[contig][reference of its column] (an integer
//           atomicMax per defined cell of the last row: order does not matter).
//   MODE 2  the trace pass: an item is (contig, its nearest reference), and every cell stores its three choices in one byte, bits 0-1
//           the state D came from (0 M, 1 X, 2 Y), bit 2 Y' came from Y, bit 3 X' came from X, at ((i - 1 + l) mod L) * w + l of its
//           strip of width w: a step's lanes write one run of bytes, and a pair takes exactly L * R bytes.
//
// Undefined is the sentinel kUndef = -2^30.  A defined value is a sum of at most 4096 substitution scores and the cost of at most
// 8192 gap residues: |v| <= 127 * 4096 + 1024 * 8192 < 2^24 < 2^29.  A value derived from the sentinel is the sentinel plus the terms
// of a monotone path of cells inside one reference, at most 8191 steps and 128 more on lanes outside the rows, each step between
// -(128 + 1024) and +127 with at most 4096 + 128 steps upwards: it stays inside [-2^30 - 9.6e6, -2^30 + 5.4e5], below every defined
// value (so it never wins a max against one), below kDefinedFloor = -2^29 (so it is never reported) and above INT32_MIN (no wrap).
//
// Walk (nearest_trace_kernel).  One thread per pair walks the bytes back from (L, lowest end column) and writes the record and the path.
#include <algorithm>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "device_utils.hpp"

namespace mgta {
namespace {

constexpr int kNearestMaxLen = 4096;                // residues of a contig or a reference: 9 bytes of LDS per row of the wave that owns the contig
constexpr size_t kNearestLdsBudget = 80 * 1024;     // of a workgroup: two fit a CU
constexpr int kSubLdsBytes = 27 * 32;               // sub[reference class][contig class], rows padded to 32
constexpr int32_t kUndef = -(1 << 30);
constexpr int32_t kDefinedFloor = -(1 << 29);
constexpr int kFirstColumn = 32;                    // bit of a column's byte: the first column of its reference (bits 0-4: the class)

struct SweepArgs {
    const uint8_t *seqs;         // the letters of every contig
    const uint64_t *off;         // [n + 1] into seqs
    const uint32_t *order;       // contig numbers, longest first (MODE 2: the batch's)
    const uint8_t *rcls;         // [n_cols] class | kFirstColumn of every reference column
    const uint32_t *seg;         // MODE 0, 1: [n_seg + 1] the columns where the segments start
    const uint32_t *pair_c0;     // MODE 2: [n_items] first column of the item's reference
    const uint32_t *pair_w;      // MODE 2: [n_items] its columns
    const uint64_t *cell_base;   // MODE 2: [n_items] where the traceback bytes of the item start
    const int32_t *col_ref;      // MODE 1: [n_cols] the reference of a column
    const int8_t *sub;           // [27 * 27]
    int32_t go, ge;
    uint64_t n_items;
    uint32_t n_seg;
    uint64_t n_ref;
    unsigned long long *keys;    // MODE 0, 1: [n_items]
    int32_t *scores;             // MODE 1: [n * n_ref], INT32_MIN before the launch
    uint8_t *tb;                 // MODE 2: traceback bytes of the batch
    int32_t *score;              // MODE 2: [n_items]
    int32_t *jend;               // MODE 2: [n_items] end column inside the reference, 1-based
    uint32_t rows_lds;           // rows a wave has in LDS (>= the longest contig, a multiple of 8)
    unsigned long long *head;
};

__device__ __forceinline__ uint32_t residue_class(uint32_t b) {           // 1 .. 26 for an ASCII letter of either case, else 0
    const uint32_t c = (b | 32u) - 'a';
    return (b < 128u && c < 26u) ? c + 1u : 0u;
}

// lane l takes v of lane l - 1, lane 0 keeps `first`: one v_mov_b32 with the DPP control wave_shr:1
__device__ __forceinline__ int32_t from_left(int32_t v, int32_t first) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xF, 0xF, false); }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

template <int MODE>
__global__ __launch_bounds__(256) void nearest_sweep_kernel(SweepArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    // [sub 27 x 32 B][boundary: waves x rows_lds x (D, Y')][classes: waves x rows_lds B]
    int8_t *s_sub = reinterpret_cast<int8_t *>(lds_raw);
    const int n_waves = blockDim.x >> 6;
    int2 *s_bound = reinterpret_cast<int2 *>(lds_raw + kSubLdsBytes) + (size_t)wave_id() * a.rows_lds;
    uint8_t *s_x = lds_raw + kSubLdsBytes + (size_t)n_waves * a.rows_lds * 8 + (size_t)wave_id() * a.rows_lds;
    for (int c = threadIdx.x; c < kSubLdsBytes; c += blockDim.x) {
        const int cy = c >> 5, cx = c & 31;
        s_sub[c] = cx < 27 ? a.sub[cx * 27 + cy] : (int8_t)0;
    }
    __syncthreads();
    const int lane = lane_id();
    const int32_t go = a.go, ge = a.ge;

    for (;;) {
        // every lane takes part and only lane 0 counts (as align_fill_kernel does: no leader-only branch in front of the wave-wide read)
        unsigned long long k = atomicAdd(a.head, lane == 0 ? 1ull : 0ull);
        k = wave_uniform((uint64_t)k);
        if (k >= a.n_items) break;
        uint32_t idx, c0, c1;
        if (MODE == 2) {
            idx = a.order[k]; c0 = a.pair_c0[k]; c1 = c0 + a.pair_w[k];
        } else {
            const uint64_t ci = k / a.n_seg;
            const uint32_t sg = (uint32_t)(k - ci * a.n_seg);
            idx = a.order[ci]; c0 = a.seg[sg]; c1 = a.seg[sg + 1];
        }
        const uint64_t o0 = a.off[idx];
        const int L = (int)(a.off[idx + 1] - o0);
        if (L == 0 || c1 == c0) {
            if (lane == 0) {
                if (MODE == 2) { a.score[k] = kUndef; a.jend[k] = 0; }
                else a.keys[k] = 0;
            }
            continue;
        }
        for (int p = lane; p < L; p += 64) s_x[p] = (uint8_t)residue_class(a.seqs[o0 + p]);
        wave_lds_fence();
        uint8_t *tb = MODE == 2 ? a.tb + a.cell_base[k] : nullptr;
        int32_t best = INT32_MIN;
        uint32_t best_g = 0;
        const int n_strips = (int)((c1 - c0 + 63) / 64);
        for (int s = 0; s < n_strips; ++s) {
            const int w = (int)min(64u, c1 - c0 - 64u * (uint32_t)s);
            const uint32_t g = c0 + 64u * (uint32_t)s + (uint32_t)lane;
            const bool own = lane < w;
            const uint32_t rc = own ? a.rcls[g] : 0u;                     // (idle lanes: class 0, and nothing of theirs is kept)
            const int cy32 = (int)(rc & 31u) << 5;
            const bool first = (rc & kFirstColumn) != 0;
            const int32_t ref_id = (MODE == 1 && own) ? a.col_ref[g] : 0;
            const bool last_strip = s == n_strips - 1;
            uint8_t *tbs = MODE == 2 ? tb + (size_t)s * 64 * L : nullptr;
            int32_t d_out = kUndef, y_out = kUndef, d_held = kUndef, v_x = kUndef, cx_out = 0;
            const int n_steps = L + w - 1;
            int i = 1 - lane;                                             // this lane's row
            int t_mod = 0;                                                // t mod L
            for (int t = 0; t < n_steps; ++t, ++i) {
                // lane 0's row is t + 1: every lane reads its slot (one address, a broadcast) and only lane 0 keeps it
                const int r0 = min(t, L - 1);
                const int2 bd = s_bound[r0];
                const int32_t cx0 = s_x[r0];
                // what the left neighbour computed at the last step: D of its row i (for this lane's row i + 1), Y[i][j], the class of x_i
                int32_t d_new = from_left(d_out, bd.x), v_y = from_left(y_out, bd.y);
                const int32_t cx = from_left(cx_out, cx0);
                cx_out = cx;
                if (first) { d_new = kUndef; v_y = kUndef; }
                int32_t d_use = d_held;
                d_held = d_new;
                if (i == 1) { d_use = 0; v_x = kUndef; }                  // row 1: B, and no insert state
                const int32_t v_m = d_use + (int32_t)s_sub[cy32 + cx];
                const int32_t open = v_m - go, y_ext = v_y - ge, x_ext = v_x - ge;
                int32_t D = v_m, Y = open, X = open;
                if (MODE == 2) {
                    uint32_t ch = 0;
                    if (v_x > D) { D = v_x; ch = 1; }
                    if (v_y > D) { D = v_y; ch = 2; }
                    if (y_ext > Y) { Y = y_ext; ch |= 4; }
                    if (x_ext > X) { X = x_ext; ch |= 8; }
                    if (own && i >= 1 && i <= L) tbs[(size_t)t_mod * w + lane] = (uint8_t)ch;   // (i - 1 + lane) mod L = t mod L
                    if (++t_mod == L) t_mod = 0;
                } else {
                    D = max(max(v_m, v_x), v_y); Y = max(open, y_ext); X = max(open, x_ext);
                }
                if (own && i == L) {
                    if (v_m > best) { best = v_m; best_g = g; }           // strips ascend: an equal score keeps the lower column
                    if (MODE == 1 && v_m >= kDefinedFloor) atomicMax(a.scores + (size_t)idx * a.n_ref + (size_t)ref_id, v_m);
                }
                if (!last_strip && lane == 63 && i >= 1 && i <= L) s_bound[i - 1] = make_int2(D, Y);
                d_out = D; y_out = Y; v_x = X;
            }
            wave_lds_fence();
        }
        // the score and the lowest column that reaches it
        const unsigned long long key = wave_max_u64(((unsigned long long)((uint32_t)best ^ 0x80000000u) << 32) | (uint32_t)~best_g);
        if (lane == 0) {
            if (MODE == 2) {
                a.score[k] = (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
                a.jend[k] = (int32_t)(~(uint32_t)key - c0) + 1;
            } else a.keys[k] = key;
        }
    }
}

struct WalkArgs {
    const uint8_t *seqs;
    const uint64_t *off;
    const uint32_t *order;
    const uint8_t *rcls;
    const uint32_t *pair_c0;
    const uint32_t *pair_w;
    const uint64_t *cell_base;
    const uint64_t *path_base;   // [count] where the path slot (L + R bytes) of a batch item starts
    uint32_t count;
    const uint8_t *tb;
    const int32_t *score;
    const int32_t *jend;
    mgta_nearest_rec *recs;      // [count]; ref is the host's to fill
    char *path;                  // or NULL
    int32_t *path_len;           // [count] (with path)
};

__device__ __forceinline__ uint8_t nearest_tb_at(const uint8_t *tb, int L, int R, int i, int j) {
    const int s = (j - 1) >> 6, l = (j - 1) & 63, w = min(64, R - 64 * s);
    return tb[(size_t)s * 64 * L + (size_t)((i - 1 + l) % L) * w + l];
}

__global__ __launch_bounds__(256) void nearest_trace_kernel(WalkArgs a) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.count) return;
    const uint32_t idx = a.order[k];
    const uint64_t o0 = a.off[idx];
    const int L = (int)(a.off[idx + 1] - o0), R = (int)a.pair_w[k];
    const int32_t score = a.score[k];
    mgta_nearest_rec r;
    r.status = 1; r.ref = -1; r.score = 0; r.ref_from = 0; r.ref_to = 0; r.n_match = 0; r.n_ident = 0; r.n_insert = 0; r.n_delete = 0;
    int plen = 0;
    if (L > 0 && R > 0 && score >= kDefinedFloor) {
        const uint8_t *x = a.seqs + o0;
        const uint8_t *y = a.rcls + a.pair_c0[k];
        const uint8_t *tb = a.tb + a.cell_base[k];
        char *slot = a.path ? a.path + a.path_base[k] : nullptr;
        const int slot_len = L + R;
        int i = L, j = a.jend[k], state = 0;
        r.status = 0; r.score = score; r.ref_to = j;
        // every step consumes a residue or a column: at most L + R of them
        for (int guard = 0; guard < L + R && i >= 1 && j >= 1 && j <= R; ++guard) {
            if (slot) slot[slot_len - 1 - plen] = state == 0 ? 'M' : state == 1 ? 'I' : 'D';
            ++plen;
            if (state == 0) {
                ++r.n_match;
                const uint32_t cx = residue_class(x[i - 1]), cy = y[j - 1] & 31u;
                r.n_ident += cx == cy && cx != 0;
                r.ref_from = j;
                if (i == 1) break;
                if (j == 1) break;                                        // (not reached: M[i > 1][1] is undefined)
                state = nearest_tb_at(tb, L, R, i - 1, j - 1) & 3;
                --i; --j;
            } else if (state == 1) {
                ++r.n_insert;
                if (i == 1) break;                                        // (not reached: X[1][.] is undefined)
                state = (nearest_tb_at(tb, L, R, i - 1, j) & 8) ? 1 : 0;
                --i;
            } else {
                ++r.n_delete;
                if (j == 1) break;                                        // (not reached: Y[.][1] is undefined)
                state = (nearest_tb_at(tb, L, R, i, j - 1) & 4) ? 2 : 0;
                --j;
            }
        }
        if (slot)
            for (int p = 0; p < plen; ++p) slot[p] = slot[slot_len - plen + p];   // forwards: the source is never behind the target
    }
    a.recs[k] = r;
    if (a.path_len) a.path_len[k] = plen;
}

template <int MODE> void launch_sweep(mgta_ctx *ctx, const SweepArgs &a, int waves, size_t lds, uint64_t n_items, int *blocks_per_cu, unsigned *grid_out) {
    MGTA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(nearest_sweep_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // workgroups a CU holds at once: what the runtime answers for these registers and this LDS (never assumed)
    int bpc = 0;
    MGTA_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, nearest_sweep_kernel<MODE>, waves * 64, lds));
    bpc = std::max(1, bpc);
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ctx->num_cus * (uint64_t)bpc, (n_items + waves - 1) / waves));
    hipLaunchKernelGGL(nearest_sweep_kernel<MODE>, dim3(grid), dim3(waves * 64), lds, ctx->stream, a);
    MGTA_HIP_CHECK(hipGetLastError());
    *blocks_per_cu = bpc; *grid_out = grid;
}

}  // namespace
}  // namespace mgta

using namespace mgta;

extern "C" {

int mgta_ctx_set_nearest_batch(mgta_ctx *ctx, int64_t cells) {
    if (!ctx) { set_error("mgta_ctx_set_nearest_batch: ctx must not be NULL"); return MGTA_EINVAL; }
    if (cells < 0) { set_error("mgta_ctx_set_nearest_batch: cells = %lld must not be negative", (long long)cells); return MGTA_EINVAL; }
    ctx->nearest_batch_cells = (uint64_t)cells;
    return MGTA_OK;
}

int mgta_seqs_nearest(mgta_ctx *ctx, const char *seqs, const uint64_t *offsets, int64_t n, const char *refs, const uint64_t *ref_offsets, int64_t n_ref,
                      const int8_t *sub, int32_t gap_open, int32_t gap_extend, mgta_nearest_rec *recs, int32_t *scores, char *path, int32_t *path_len,
                      mgta_nearest_stats *stats) {
    if (!ctx) { set_error("mgta_seqs_nearest: ctx must not be NULL"); return MGTA_EINVAL; }
    if (n < 0) { set_error("mgta_seqs_nearest: n = %lld must not be negative", (long long)n); return MGTA_EINVAL; }
    if (n_ref < 0) { set_error("mgta_seqs_nearest: n_ref = %lld must not be negative", (long long)n_ref); return MGTA_EINVAL; }
    if (n >= (1ll << 31)) { set_error("mgta_seqs_nearest: n = %lld (the limit is n < 2^31 contigs)", (long long)n); return MGTA_EINVAL; }
    if (n_ref >= (1ll << 31)) { set_error("mgta_seqs_nearest: n_ref = %lld (the limit is n_ref < 2^31 references)", (long long)n_ref); return MGTA_EINVAL; }
    if (gap_extend < 0 || gap_extend > gap_open || gap_open > 1024) {
        set_error("mgta_seqs_nearest: gap_open = %d, gap_extend = %d (the rule needs 0 <= gap_extend <= gap_open <= 1024)", gap_open, gap_extend);
        return MGTA_EINVAL;
    }
    if (n > 0 && !offsets) { set_error("mgta_seqs_nearest: offsets must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && !recs) { set_error("mgta_seqs_nearest: recs must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && !sub) { set_error("mgta_seqs_nearest: sub must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && n_ref > 0 && !ref_offsets) { set_error("mgta_seqs_nearest: ref_offsets must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && path && !path_len) { set_error("mgta_seqs_nearest: path_len must not be NULL when path is given"); return MGTA_EINVAL; }
    for (int64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) { set_error("mgta_seqs_nearest: contig %lld: offsets must ascend", (long long)i); return MGTA_EINVAL; }
        if (offsets[i + 1] - offsets[i] > (uint64_t)kNearestMaxLen) {
            set_error("mgta_seqs_nearest: contig %lld holds %llu residues (the limit is %d residues per contig)", (long long)i,
                      (unsigned long long)(offsets[i + 1] - offsets[i]), kNearestMaxLen);
            return MGTA_EINVAL;
        }
    }
    for (int64_t i = 0; n > 0 && i < n_ref; ++i) {
        if (ref_offsets[i + 1] < ref_offsets[i]) { set_error("mgta_seqs_nearest: reference %lld: ref_offsets must ascend", (long long)i); return MGTA_EINVAL; }
        if (ref_offsets[i + 1] - ref_offsets[i] > (uint64_t)kNearestMaxLen) {
            set_error("mgta_seqs_nearest: reference %lld holds %llu residues (the limit is %d residues per reference)", (long long)i,
                      (unsigned long long)(ref_offsets[i + 1] - ref_offsets[i]), kNearestMaxLen);
            return MGTA_EINVAL;
        }
    }
    const uint64_t n_letters = n > 0 ? offsets[n] - offsets[0] : 0, n_cols = (n > 0 && n_ref > 0) ? ref_offsets[n_ref] - ref_offsets[0] : 0;
    if (n_cols >= (1ull << 31)) {
        set_error("mgta_seqs_nearest: the references hold %llu residues together (the limit is fewer than 2^31 residues in all references)", (unsigned long long)n_cols);
        return MGTA_EINVAL;
    }
    if (n_letters && !seqs) { set_error("mgta_seqs_nearest: seqs must not be NULL"); return MGTA_EINVAL; }
    if (n_cols && !refs) { set_error("mgta_seqs_nearest: refs must not be NULL"); return MGTA_EINVAL; }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return MGTA_OK;
    return guarded("mgta_seqs_nearest", [&]() {
        const uint32_t nn = (uint32_t)n;
        mgta_nearest_rec none;
        none.status = 1; none.ref = -1; none.score = 0; none.ref_from = 0; none.ref_to = 0; none.n_match = 0; none.n_ident = 0; none.n_insert = 0; none.n_delete = 0;
        const unsigned __int128 all_cells = (unsigned __int128)n_letters * n_cols;
        if (stats) {
            stats->n_seqs = n; stats->n_refs = n_ref; stats->n_pairs = n * n_ref;
            stats->n_cells = all_cells > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)all_cells;
        }
        if (n_letters == 0 || n_cols == 0) {                              // no pair has a score
            for (uint32_t i = 0; i < nn; ++i) recs[i] = none;
            if (scores) std::fill(scores, scores + (size_t)n * (size_t)n_ref, INT32_MIN);
            if (path) std::fill(path_len, path_len + nn, 0);
            if (stats) stats->n_unaligned = n;
            return (int)MGTA_OK;
        }
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        uint64_t *live = &ctx->live_bytes, *peak = &ctx->peak_bytes;
        struct PeakOfCall {                                               // peak_bytes is this call's while it runs, the context's again on every way out
            uint64_t *peak, before;
            ~PeakOfCall() { *peak = std::max(*peak, before); }
        } peak_of_call{peak, *peak};
        *peak = *live;

        // the contigs: letters, where they start, longest first
        std::vector<uint64_t> rel((size_t)nn + 1);
        for (uint32_t i = 0; i <= nn; ++i) rel[i] = offsets[i] - offsets[0];
        std::vector<uint32_t> order(nn);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return rel[x + 1] - rel[x] > rel[y + 1] - rel[y]; });
        // the columns: class and first-column bit; where every reference starts
        const uint32_t nc = (uint32_t)n_cols;
        std::vector<uint32_t> rstart((size_t)n_ref + 1);
        for (int64_t r = 0; r <= n_ref; ++r) rstart[(size_t)r] = (uint32_t)(ref_offsets[r] - ref_offsets[0]);
        std::vector<uint8_t> rcls(nc);
        const unsigned char *rtext = reinterpret_cast<const unsigned char *>(refs) + ref_offsets[0];
        for (uint32_t g = 0; g < nc; ++g) {
            const uint32_t b = rtext[g], c = (b | 32u) - 'a';
            rcls[g] = (uint8_t)((b < 128u && c < 26u) ? c + 1u : 0u);
        }
        for (int64_t r = 0; r < n_ref; ++r)
            if (rstart[(size_t)r + 1] > rstart[(size_t)r]) rcls[rstart[(size_t)r]] |= kFirstColumn;
        // segments: whole references, enough of them that (contig, segment) items fill the device when the contigs are few
        const uint64_t want_items = (uint64_t)ctx->num_cus * 32;
        const uint64_t want_seg = std::max<uint64_t>(1, std::min<uint64_t>((want_items + nn - 1) / nn, std::max<uint64_t>(1, n_cols / 1024)));
        const uint64_t seg_cols = (n_cols + want_seg - 1) / want_seg;
        std::vector<uint32_t> seg{0u};
        for (int64_t r = 0; r < n_ref; ++r)
            if ((uint64_t)(rstart[(size_t)r + 1] - seg.back()) >= seg_cols && rstart[(size_t)r + 1] > seg.back()) seg.push_back(rstart[(size_t)r + 1]);
        if (seg.back() != nc) seg.push_back(nc);
        const uint32_t n_seg = (uint32_t)seg.size() - 1;
        const uint64_t n_items = (uint64_t)nn * n_seg;

        const uint32_t l_max = (uint32_t)(rel[order[0] + 1] - rel[order[0]]);
        const uint32_t rows_lds = (std::max(1u, l_max) + 7u) & ~7u;
        int waves = 4;
        while (waves > 1 && kSubLdsBytes + (size_t)waves * rows_lds * 9 > kNearestLdsBudget) waves >>= 1;
        const size_t lds = kSubLdsBytes + (size_t)waves * rows_lds * 9;

        DevBuf d_seqs, d_off, d_order, d_rcls, d_seg, d_sub, d_head, d_keys, d_colref, d_scores;
        d_seqs.alloc(n_letters + 16, live, peak);
        d_off.alloc((size_t)(nn + 1) * 8, live, peak);
        d_order.alloc((size_t)nn * 4, live, peak);
        d_rcls.alloc((size_t)nc + 16, live, peak);
        d_seg.alloc((size_t)(n_seg + 1) * 4, live, peak);
        d_sub.alloc(27 * 27, live, peak);
        d_head.alloc(64, live, peak);
        d_keys.alloc((size_t)n_items * 8, live, peak);
        MGTA_HIP_CHECK(hipMemcpyAsync(d_seqs.p, seqs + offsets[0], n_letters, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_off.p, rel.data(), (size_t)(nn + 1) * 8, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_order.p, order.data(), (size_t)nn * 4, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_rcls.p, rcls.data(), nc, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_seg.p, seg.data(), (size_t)(n_seg + 1) * 4, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_sub.p, sub, 27 * 27, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemsetAsync(d_head.p, 0, 64, st));
        std::vector<int32_t> col_ref;
        if (scores) {
            col_ref.resize(nc);
            for (int64_t r = 0; r < n_ref; ++r) std::fill(col_ref.begin() + rstart[(size_t)r], col_ref.begin() + rstart[(size_t)r + 1], (int32_t)r);
            d_colref.alloc((size_t)nc * 4, live, peak);
            d_scores.alloc((size_t)n * (size_t)n_ref * 4, live, peak);
            MGTA_HIP_CHECK(hipMemcpyAsync(d_colref.p, col_ref.data(), (size_t)nc * 4, hipMemcpyHostToDevice, st));
            MGTA_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)d_scores.p, (int)0x80000000u, (size_t)n * (size_t)n_ref, st));
        }

        SweepArgs sa;
        memset(&sa, 0, sizeof sa);
        sa.seqs = d_seqs.as<uint8_t>(); sa.off = d_off.as<uint64_t>(); sa.order = d_order.as<uint32_t>(); sa.rcls = d_rcls.as<uint8_t>(); sa.seg = d_seg.as<uint32_t>();
        sa.col_ref = d_colref.as<int32_t>(); sa.sub = d_sub.as<int8_t>(); sa.go = gap_open; sa.ge = gap_extend; sa.n_items = n_items; sa.n_seg = n_seg;
        sa.n_ref = (uint64_t)n_ref; sa.keys = d_keys.as<unsigned long long>(); sa.scores = d_scores.as<int32_t>(); sa.rows_lds = rows_lds;
        sa.head = d_head.as<unsigned long long>();
        Timer t_score(st), t_trace(st);
        int blocks_per_cu = 0;
        unsigned grid = 0;
        t_score.start();
        if (scores) launch_sweep<1>(ctx, sa, waves, lds, n_items, &blocks_per_cu, &grid);
        else launch_sweep<0>(ctx, sa, waves, lds, n_items, &blocks_per_cu, &grid);
        t_score.end();
        std::vector<unsigned long long> keys((size_t)n_items);
        MGTA_HIP_CHECK(hipMemcpyAsync(keys.data(), d_keys.p, (size_t)n_items * 8, hipMemcpyDeviceToHost, st));
        if (scores) MGTA_HIP_CHECK(hipMemcpyAsync(scores, d_scores.p, (size_t)n * (size_t)n_ref * 4, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        const double ms_score = t_score.ms();
        d_keys.release(); d_scores.release(); d_colref.release(); d_seg.release();

        // the nearest reference of every contig: the largest key of its items
        std::vector<uint32_t> t_order;                                    // the aligned contigs, longest first
        std::vector<uint32_t> near_ref(nn, 0), near_c0(nn, 0);
        for (uint32_t ci = 0; ci < nn; ++ci) {
            const uint32_t idx = order[ci];
            unsigned long long key = 0;
            for (uint32_t s = 0; s < n_seg; ++s) key = std::max(key, keys[(size_t)ci * n_seg + s]);
            const int32_t best = (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
            recs[idx] = none;
            if (path) path_len[idx] = 0;
            if (best < kDefinedFloor) continue;
            const uint32_t g = ~(uint32_t)key;
            const uint32_t r = (uint32_t)(std::upper_bound(rstart.begin(), rstart.end(), g) - rstart.begin()) - 1;   // the last reference that starts at or before g
            near_ref[idx] = r; near_c0[idx] = rstart[r];
            t_order.push_back(idx);
        }
        const uint32_t n_al = (uint32_t)t_order.size();

        // cells of a batch: the switch, or half of what the context may still take (one traceback byte per cell)
        uint64_t cap = ctx->nearest_batch_cells;
        if (!cap) {
            size_t free_b = 0, total_b = 0;
            MGTA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            uint64_t avail = free_b;
            if (ctx->mem_limit) avail = std::min<uint64_t>(avail, ctx->mem_limit > ctx->live_bytes ? ctx->mem_limit - ctx->live_bytes : 0);
            cap = std::max<uint64_t>(avail / 2, 1);
        }
        double ms_trace = 0;
        int64_t n_batches = 0, n_trace_cells = 0;
        if (n_al) MGTA_HIP_CHECK(hipMemcpyAsync(d_order.p, t_order.data(), (size_t)n_al * 4, hipMemcpyHostToDevice, st));
        std::vector<uint64_t> cell_base, path_base;
        std::vector<uint32_t> pair_c0, pair_w;
        std::vector<mgta_nearest_rec> h_recs;
        std::vector<char> h_path;
        std::vector<int32_t> h_plen;
        for (uint32_t b0 = 0; b0 < n_al;) {
            // the batch [b0, b1): at least one pair
            uint32_t b1 = b0;
            uint64_t cells = 0, path_bytes = 0;
            cell_base.clear(); path_base.clear(); pair_c0.clear(); pair_w.clear();
            while (b1 < n_al) {
                const uint32_t idx = t_order[b1], r = near_ref[idx];
                const uint64_t L = rel[idx + 1] - rel[idx], R = rstart[r + 1] - rstart[r];
                if (b1 > b0 && cells + L * R > cap) break;
                cell_base.push_back(cells); path_base.push_back(path_bytes); pair_c0.push_back(rstart[r]); pair_w.push_back((uint32_t)R);
                cells += L * R; path_bytes += L + R;
                ++b1;
            }
            const uint32_t count = b1 - b0;
            DevBuf d_tb, d_cbase, d_pbase, d_c0, d_w, d_score, d_jend, d_recs, d_path, d_plen;
            d_tb.alloc(cells + 16, live, peak);
            d_cbase.alloc((size_t)count * 8, live, peak);
            d_c0.alloc((size_t)count * 4, live, peak);
            d_w.alloc((size_t)count * 4, live, peak);
            d_score.alloc((size_t)count * 4, live, peak);
            d_jend.alloc((size_t)count * 4, live, peak);
            d_recs.alloc((size_t)count * sizeof(mgta_nearest_rec), live, peak);
            MGTA_HIP_CHECK(hipMemcpyAsync(d_cbase.p, cell_base.data(), (size_t)count * 8, hipMemcpyHostToDevice, st));
            MGTA_HIP_CHECK(hipMemcpyAsync(d_c0.p, pair_c0.data(), (size_t)count * 4, hipMemcpyHostToDevice, st));
            MGTA_HIP_CHECK(hipMemcpyAsync(d_w.p, pair_w.data(), (size_t)count * 4, hipMemcpyHostToDevice, st));
            if (path) {
                d_pbase.alloc((size_t)count * 8, live, peak);
                d_path.alloc(path_bytes, live, peak);
                d_plen.alloc((size_t)count * 4, live, peak);
                MGTA_HIP_CHECK(hipMemcpyAsync(d_pbase.p, path_base.data(), (size_t)count * 8, hipMemcpyHostToDevice, st));
            }
            MGTA_HIP_CHECK(hipMemsetAsync(d_head.p, 0, 64, st));

            SweepArgs fa = sa;
            fa.order = d_order.as<uint32_t>() + b0; fa.seg = nullptr; fa.col_ref = nullptr; fa.keys = nullptr; fa.scores = nullptr; fa.n_seg = 1;
            fa.pair_c0 = d_c0.as<uint32_t>(); fa.pair_w = d_w.as<uint32_t>(); fa.cell_base = d_cbase.as<uint64_t>(); fa.n_items = count;
            fa.tb = d_tb.as<uint8_t>(); fa.score = d_score.as<int32_t>(); fa.jend = d_jend.as<int32_t>();
            int bpc2 = 0;
            unsigned grid2 = 0;
            t_trace.start();
            launch_sweep<2>(ctx, fa, waves, lds, count, &bpc2, &grid2);
            WalkArgs wa;
            wa.seqs = fa.seqs; wa.off = fa.off; wa.order = fa.order; wa.rcls = fa.rcls; wa.pair_c0 = fa.pair_c0; wa.pair_w = fa.pair_w; wa.cell_base = fa.cell_base;
            wa.path_base = d_pbase.as<uint64_t>(); wa.count = count; wa.tb = fa.tb; wa.score = fa.score; wa.jend = fa.jend; wa.recs = d_recs.as<mgta_nearest_rec>();
            wa.path = path ? d_path.as<char>() : nullptr; wa.path_len = path ? d_plen.as<int32_t>() : nullptr;
            hipLaunchKernelGGL(nearest_trace_kernel, dim3((count + 255) / 256), dim3(256), 0, st, wa);
            MGTA_HIP_CHECK(hipGetLastError());
            t_trace.end();

            h_recs.resize(count);
            MGTA_HIP_CHECK(hipMemcpyAsync(h_recs.data(), d_recs.p, (size_t)count * sizeof(mgta_nearest_rec), hipMemcpyDeviceToHost, st));
            if (path) {
                h_path.resize(path_bytes);
                h_plen.resize(count);
                MGTA_HIP_CHECK(hipMemcpyAsync(h_path.data(), d_path.p, path_bytes, hipMemcpyDeviceToHost, st));
                MGTA_HIP_CHECK(hipMemcpyAsync(h_plen.data(), d_plen.p, (size_t)count * 4, hipMemcpyDeviceToHost, st));
            }
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
            ms_trace += t_trace.ms();
            for (uint32_t k = 0; k < count; ++k) {
                const uint32_t idx = t_order[b0 + k];
                if (h_recs[k].status != 0) {
                    set_error("mgta_seqs_nearest: contig %u: the trace pass found no score where the score pass found one", idx);
                    return (int)MGTA_EHIP;
                }
                recs[idx] = h_recs[k];
                recs[idx].ref = (int32_t)near_ref[idx];
                if (path) {
                    path_len[idx] = h_plen[k];
                    memcpy(path + offsets[idx] + (uint64_t)idx * kNearestMaxLen, h_path.data() + path_base[k], (size_t)h_plen[k]);
                }
            }
            n_trace_cells += (int64_t)cells; ++n_batches;
            b0 = b1;
        }
        if (stats) {
            stats->n_unaligned = n - (int64_t)n_al; stats->n_trace_cells = n_trace_cells; stats->n_batches = n_batches; stats->n_segments = n_seg;
            stats->blocks_per_cu = blocks_per_cu; stats->waves_per_block = waves; stats->grid_blocks = grid; stats->lds_bytes = (int64_t)lds;
            stats->peak_bytes = (int64_t)ctx->peak_bytes; stats->ms_score = ms_score; stats->ms_trace = ms_trace;
        }
        return (int)MGTA_OK;
    });
}

}  // extern "C"
