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
#include <vector>

#include "seq_dp.hpp"

namespace mgta {
namespace {

constexpr int kNearestMaxLen = 4096;                // residues of a contig or a reference: 9 bytes of LDS per row of the wave that owns the contig
constexpr size_t kNearestLdsBudget = 80 * 1024;     // of a workgroup: two fit a CU

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
    stage_sub(s_sub, a.sub);
    const int lane = lane_id();
    const int32_t go = a.go, ge = a.ge;

    for (;;) {
        const unsigned long long k = next_item(a.head);
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
        int n_ident = 0;
        const Walked w = trace_walk(a.tb + a.cell_base[k], L, R, a.jend[k], a.path ? a.path + a.path_base[k] : nullptr, [&](int i, int j) {
            const uint32_t cx = residue_class(x[i - 1]), cy = y[j - 1] & 31u;
            n_ident += cx == cy && cx != 0;
        });
        r.status = 0; r.score = score; r.ref_to = a.jend[k]; r.ref_from = w.from; r.n_match = w.n_match; r.n_ident = n_ident; r.n_insert = w.n_insert; r.n_delete = w.n_delete;
        plen = w.plen;
    }
    a.recs[k] = r;
    if (a.path_len) a.path_len[k] = plen;
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
    if (!check_seq_count("mgta_seqs_nearest", kContigs, n)) return MGTA_EINVAL;
    if (!check_seq_count("mgta_seqs_nearest", kReferences, n_ref)) return MGTA_EINVAL;
    if (gap_extend < 0 || gap_extend > gap_open || gap_open > 1024) {
        set_error("mgta_seqs_nearest: gap_open = %d, gap_extend = %d (the rule needs 0 <= gap_extend <= gap_open <= 1024)", gap_open, gap_extend);
        return MGTA_EINVAL;
    }
    if (n > 0 && !offsets) { set_error("mgta_seqs_nearest: offsets must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && !recs) { set_error("mgta_seqs_nearest: recs must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && !sub) { set_error("mgta_seqs_nearest: sub must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && n_ref > 0 && !ref_offsets) { set_error("mgta_seqs_nearest: ref_offsets must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && path && !path_len) { set_error("mgta_seqs_nearest: path_len must not be NULL when path is given"); return MGTA_EINVAL; }
    if (!check_seq_offsets("mgta_seqs_nearest", kContigs, offsets, n, kNearestMaxLen)) return MGTA_EINVAL;
    if (!check_seq_offsets("mgta_seqs_nearest", kReferences, ref_offsets, n > 0 ? n_ref : 0, kNearestMaxLen)) return MGTA_EINVAL;
    const uint64_t n_letters = n > 0 ? offsets[n] - offsets[0] : 0, n_cols = (n > 0 && n_ref > 0) ? ref_offsets[n_ref] - ref_offsets[0] : 0;
    if (!check_ref_columns("mgta_seqs_nearest", n_cols)) return MGTA_EINVAL;
    if (!check_seq_letters("mgta_seqs_nearest", kContigs, seqs, n_letters)) return MGTA_EINVAL;
    if (!check_seq_letters("mgta_seqs_nearest", kReferences, refs, n_cols)) return MGTA_EINVAL;
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
        PeakOfCall peak_of_call(ctx);

        // the contigs: letters, where they start, longest first
        const std::vector<uint64_t> rel = rel_offsets(offsets, n);
        const std::vector<uint32_t> order = longest_first(rel);
        // the columns: class and first-column bit; where every reference starts
        const uint32_t nc = (uint32_t)n_cols;
        std::vector<uint32_t> rstart;
        std::vector<uint8_t> rcls;
        ref_columns(refs, ref_offsets, n_ref, rstart, rcls);
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
        const int waves = waves_that_fit(rows_lds, 9, kSubLdsBytes, kNearestLdsBudget);
        const size_t lds = kSubLdsBytes + (size_t)waves * rows_lds * 9;

        SeqStage dev;
        dev.upload(ctx, seqs, offsets, rel, &order);
        DevBuf d_rcls, d_seg, d_sub, d_keys, d_colref, d_scores;
        d_rcls.alloc((size_t)nc + 16, live, peak);
        d_seg.alloc((size_t)(n_seg + 1) * 4, live, peak);
        d_sub.alloc(27 * 27, live, peak);
        d_keys.alloc((size_t)n_items * 8, live, peak);
        MGTA_HIP_CHECK(hipMemcpyAsync(d_rcls.p, rcls.data(), nc, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_seg.p, seg.data(), (size_t)(n_seg + 1) * 4, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_sub.p, sub, 27 * 27, hipMemcpyHostToDevice, st));
        dev.reset_head(st);
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
        sa.seqs = dev.seqs.as<uint8_t>(); sa.off = dev.off.as<uint64_t>(); sa.order = dev.order.as<uint32_t>(); sa.rcls = d_rcls.as<uint8_t>(); sa.seg = d_seg.as<uint32_t>();
        sa.col_ref = d_colref.as<int32_t>(); sa.sub = d_sub.as<int8_t>(); sa.go = gap_open; sa.ge = gap_extend; sa.n_items = n_items; sa.n_seg = n_seg;
        sa.n_ref = (uint64_t)n_ref; sa.keys = d_keys.as<unsigned long long>(); sa.scores = d_scores.as<int32_t>(); sa.rows_lds = rows_lds;
        sa.head = dev.head.as<unsigned long long>();
        Timer t_score(st), t_trace(st);
        t_score.start();
        const WaveLaunch sweep = launch_waves(ctx, scores ? nearest_sweep_kernel<1> : nearest_sweep_kernel<0>, sa, waves, lds, n_items);
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

        const uint64_t cap = batch_cap(ctx, ctx->nearest_batch_cells, 1);    // one traceback byte per cell
        double ms_trace = 0;
        int64_t n_batches = 0, n_trace_cells = 0;
        if (n_al) MGTA_HIP_CHECK(hipMemcpyAsync(dev.order.p, t_order.data(), (size_t)n_al * 4, hipMemcpyHostToDevice, st));
        std::vector<uint64_t> cell_base, path_base;
        std::vector<uint32_t> pair_c0, pair_w;
        std::vector<mgta_nearest_rec> h_recs;
        std::vector<char> h_path;
        std::vector<int32_t> h_plen;
        for (uint32_t b0 = 0; b0 < n_al;) {
            // the batch [b0, b1): a pair is a contig and its nearest reference
            uint64_t cells = 0, path_bytes = 0;
            const auto ref_of = [&](uint32_t k) { return near_ref[t_order[k]]; };
            const uint32_t b1 = cut_cells(b0, n_al, cap, [&](uint32_t k) { return rel[t_order[k] + 1] - rel[t_order[k]]; },
                                          [&](uint32_t k) { return (uint64_t)(rstart[ref_of(k) + 1] - rstart[ref_of(k)]); }, cell_base, &path_base, &cells, &path_bytes);
            const uint32_t count = b1 - b0;
            pair_c0.clear(); pair_w.clear();
            for (uint32_t k = b0; k < b1; ++k) { pair_c0.push_back(rstart[ref_of(k)]); pair_w.push_back(rstart[ref_of(k) + 1] - rstart[ref_of(k)]); }
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
            dev.reset_head(st);

            SweepArgs fa = sa;
            fa.order = dev.order.as<uint32_t>() + b0; fa.seg = nullptr; fa.col_ref = nullptr; fa.keys = nullptr; fa.scores = nullptr; fa.n_seg = 1;
            fa.pair_c0 = d_c0.as<uint32_t>(); fa.pair_w = d_w.as<uint32_t>(); fa.cell_base = d_cbase.as<uint64_t>(); fa.n_items = count;
            fa.tb = d_tb.as<uint8_t>(); fa.score = d_score.as<int32_t>(); fa.jend = d_jend.as<int32_t>();
            t_trace.start();
            launch_waves(ctx, nearest_sweep_kernel<2>, fa, waves, lds, count);
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
            stats->blocks_per_cu = sweep.blocks_per_cu; stats->waves_per_block = waves; stats->grid_blocks = sweep.grid; stats->lds_bytes = (int64_t)lds;
            stats->peak_bytes = (int64_t)ctx->peak_bytes; stats->ms_score = ms_score; stats->ms_trace = ms_trace;
        }
        return (int)MGTA_OK;
    });
}

}  // extern "C"
