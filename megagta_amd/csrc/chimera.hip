// chimera.hip — contigs that two references explain better than one (mgta_seqs_chimera): the place of the chimera removal in the
// reference's bin/post_proc.sh:89-95.  The rule is this library's own (include/megagta_hip.h), built on the score of
// mgta_seqs_nearest: for every prefix x[1..b] and every suffix x[b..L] of a contig the two best references, then per breakpoint
// the best pair of different references against the best single reference that is given the same free jump.
//
// Sweep (chimera_sweep_kernel).  nearest.hip turned round: there a lane owns a column and the maximum over a contig's LAST row is
// wanted; here the maximum of EVERY row over every reference is wanted, so a lane owns a row and keeps that maximum in a register.
// The references are one run of columns, one byte per column: bits 0-4 the residue class, bit 5 "first column of its reference",
// bit 6 "a column" (the lanes that wait in front of or behind the run see 0).  The run is cut at reference boundaries into
// segments (first column, column behind the last); a work item is (contig, direction, group of consecutive segments), taken
// longest contig first from one atomic head by one wave.  Rows go in strips of 64: lane l owns row 64 s + l + 1 and at step t computes column t - l of the segment, so the cells
// of one anti-diagonal are computed together.  From the cell (i, j) outwards:
//     D  = max(M, X, Y)[i][j]                 the candidate of M[i+1][j+1]  (taken by lane l + 1 two steps later)
//     X' = max(M[i][j] - go, X[i][j] - ge)    X[i+1][j]                     (taken by lane l + 1 at the next step)
//     Y' = max(M[i][j] - go, Y[i][j] - ge)    Y[i][j+1]                     (its own next step)
// D, X' and the column byte move to lane l + 1 by one DPP wave shift each (v_mov_b32 wave_shr:1).  Lane 0 takes the column byte
// from a register block of 64 columns (one coalesced load per 64 steps, v_readlane per step) and, in every strip but the first,
// (D, X') of the row above from the boundary buffer: row 64 of a strip leaves them there per column, 8 bytes, in device memory,
// one buffer per resident wave, read back the same way in blocks of 64.  The buffer is used in place: column j is read (and waited
// for) at step j or earlier and written at step j + 63; between two strips the wave's stores are made visible to its own loads by
// an agent fence.  At a column flagged "first" a lane folds the maximum of the reference it has just left into its top two
// (score, reference) registers, bumps its reference counter, and takes "undefined" for D and Y'; one flagged column behind the
// segment's end makes the last fold.  References ascend and the fold is strict, so the lower index keeps a tie.  The top two of a
// row live in device memory between the segments of an item (same lane, same address); the groups of a (contig, direction) are
// folded by chimera_tops_kernel, which also turns the counter (references with residues) into the reference index.  `sub` sits in
// LDS, 32 bytes per reference class; nothing else does.  The suffix pass is the same kernel over the reversed contig and the run
// of reversed references (in the same order): the row of the reversed prefix of length L - b + 1 is the suffix that starts at b.
//   MODE 0  top two of every row, both directions.
//   MODE 1  the parents pass: the segments of an item are the three references N, A, B of its contig, in place in the same run of
//           columns (counters 0, 1, 2), and at each fold the row's maximum over the finished reference is stored as int32 (INT32_MIN =
//           undefined) instead of being folded.
//
// Undefined is nearest.hip's sentinel kUndef = -2^30 and kDefinedFloor = -2^29 is its floor.  A defined value is below 2^24 in size
// (include/megagta_hip.h).  A value derived from the sentinel is the sentinel plus the terms of a monotone path of cells inside one
// reference, at most 8191 steps, 63 more on the lanes past row L and 126 more on lanes in front of and behind the run, each step
// between -(128 + 1024) and +127 with at most 4096 + 189 of them upwards: it stays inside [-2^30 - 9.7e6, -2^30 + 5.5e5], below
// every defined value, below the floor and above INT32_MIN.  two, one and gain are sums of two defined values: below 2^25.
//
// Steps 2 to 5 of the rule are O(L) per contig and run on the host inside the library.
#include <algorithm>
#include <vector>

#include "seq_dp.hpp"

namespace mgta {
namespace {

constexpr int kChimeraMaxLen = 4096;
constexpr uint32_t kIsColumn = 64;                  // bit of a column's byte: a column of the segment
constexpr uint64_t kDefaultSegment = 4096;          // columns of a segment (plus what the last reference needs to end)
constexpr int kSweepWaves = 4;

struct ChimItem {
    uint32_t contig, dir;        // dir 1: the reversed contig
    uint32_t seg_lo, seg_hi;     // its segments
    uint64_t col_add;            // where its columns start in rcls (the reversed run lies behind the forward one)
    uint64_t out_base;           // MODE 0: first int4 of its (group, direction) plane; MODE 1: first int32 of its direction's three planes
};

struct ChimArgs {
    const uint8_t *seqs;         // the letters of every contig
    const uint64_t *off;         // [n + 1] into seqs
    const uint8_t *rcls;         // class | kFirstColumn of every column
    const uint2 *seg;            // [n_seg] first column of a segment and the column behind its last
    const uint32_t *segref;      // [n_seg] the counter of the first reference of a segment
    const ChimItem *items;
    const int8_t *sub;           // [27 * 27]
    int32_t go, ge;
    uint64_t n_items;
    uint64_t n_rows;             // letters of all contigs: the size of a plane
    int4 *part;                  // MODE 0: [groups * 2 planes][n_rows] (score 1, counter 1, score 2, counter 2)
    int32_t *rowmax;             // MODE 1: [2 directions][3 references][n_rows]
    int2 *bound;                 // [resident waves][bound_stride] (D, X') of a strip's last row, or NULL when no contig has a second strip
    uint64_t bound_stride;
    unsigned long long *head;
};

template <int MODE>
__global__ __launch_bounds__(kSweepWaves * 64) void chimera_sweep_kernel(ChimArgs a) {
    __shared__ int8_t s_sub[kSubLdsBytes];
    stage_sub(s_sub, a.sub);
    const int lane = lane_id();
    const int32_t go = a.go, ge = a.ge;
    int2 *bound = a.bound ? a.bound + ((size_t)blockIdx.x * kSweepWaves + (size_t)wave_id()) * a.bound_stride : nullptr;

    for (;;) {
        const unsigned long long k = next_item(a.head);
        if (k >= a.n_items) break;
        const ChimItem it = a.items[k];
        const uint64_t o0 = a.off[it.contig];
        const int L = (int)(a.off[it.contig + 1] - o0);
        if (L == 0) continue;
        const int n_strips = (L + 63) >> 6;
        for (uint32_t sg = it.seg_lo; sg < it.seg_hi; ++sg) {
            const uint2 cut = a.seg[sg];
            const uint32_t c0 = cut.x;
            const int W = (int)(cut.y - c0);
            const int32_t first_ref = (int32_t)a.segref[sg];
            const uint8_t *cols = a.rcls + it.col_add + c0;
            for (int s = 0; s < n_strips; ++s) {
                const int rows = min(64, L - 64 * s);
                const bool mine = lane < rows;
                const int row0 = 64 * s + lane;
                const uint64_t pos = o0 + (uint64_t)(mine ? (it.dir ? L - 1 - row0 : row0) : 0);   // the letter and the place in a plane
                const int cx = mine ? (int)residue_class(a.seqs[pos]) : 0;
                const bool row_one = s == 0 && lane == 0, last_strip = s == n_strips - 1;
                int32_t s1 = INT32_MIN, r1 = -1, s2 = INT32_MIN, r2 = -1;
                if (MODE == 0 && sg > it.seg_lo && mine) {
                    const int4 v = a.part[it.out_base + pos];
                    s1 = v.x; r1 = v.y; s2 = v.z; r2 = v.w;
                }
                int32_t ref = first_ref - 1;                                                        // bumped at the first column
                int32_t d_out = kUndef, x_out = kUndef, d_held = kUndef, v_y = kUndef, cb_out = 0, best = INT32_MIN;
                const int n_steps = W + rows;                                                       // lane l meets the column behind the end at step W + l
                for (int t0 = 0; t0 < n_steps; t0 += 64) {
                    // the next 64 columns, one per lane: the byte, and what the strip above left
                    const int j = t0 + lane;
                    const int32_t blk_cb = j < W ? (int32_t)((uint32_t)cols[j] | kIsColumn) : (j == W ? (int32_t)kFirstColumn : 0);
                    int2 blk = make_int2(kUndef, kUndef);
                    if (s > 0 && j < W) blk = bound[j];
                    const int te = min(64, n_steps - t0);
                    for (int tt = 0; tt < te; ++tt) {
                        const int32_t cb = from_left(cb_out, __builtin_amdgcn_readlane(blk_cb, tt));
                        const int32_t d_new = from_left(d_out, __builtin_amdgcn_readlane(blk.x, tt));
                        int32_t v_x = from_left(x_out, __builtin_amdgcn_readlane(blk.y, tt));
                        cb_out = cb;
                        int32_t d_use = d_held;
                        d_held = d_new;
                        if ((uint32_t)cb & kFirstColumn) {
                            const int32_t m = best >= kDefinedFloor ? best : INT32_MIN;
                            if (MODE == 1) {
                                if (ref >= first_ref && mine) a.rowmax[it.out_base + (uint64_t)ref * a.n_rows + pos] = m;
                            } else {
                                if (m > s1) { s2 = s1; r2 = r1; s1 = m; r1 = ref; }
                                else if (m > s2) { s2 = m; r2 = ref; }
                            }
                            ++ref;
                            best = INT32_MIN; d_use = kUndef; v_y = kUndef;
                        }
                        if (row_one) { d_use = 0; v_x = kUndef; }                                   // row 1: B, and no insert state
                        const int32_t v_m = d_use + (int32_t)s_sub[(((uint32_t)cb & 31u) << 5) + cx];
                        const int32_t open = v_m - go;
                        const int32_t D = max(max(v_m, v_x), v_y), X = max(open, v_x - ge), Y = max(open, v_y - ge);
                        const bool column = ((uint32_t)cb & kIsColumn) != 0;
                        best = column ? max(best, v_m) : best;
                        if (!last_strip && lane == 63 && column) bound[t0 + tt - 63] = make_int2(D, X);
                        d_out = D; x_out = X; v_y = Y;
                    }
                }
                if (MODE == 0 && mine) a.part[it.out_base + pos] = make_int4(s1, r1, s2, r2);
                if (!last_strip) __threadfence();                                                   // lane 63's stores, the next strip's loads
            }
        }
    }
}

// the groups of a (row, direction) folded, the counter turned into the reference: tops[row * 8 + direction * 4 ..]
__global__ __launch_bounds__(256) void chimera_tops_kernel(const int4 *part, uint64_t n_rows, uint32_t n_groups, const int32_t *nz_ref, int4 *tops) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_rows * 2) return;
    const uint64_t p = q >> 1, dir = q & 1;
    int32_t s1 = INT32_MIN, r1 = -1, s2 = INT32_MIN, r2 = -1;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const int4 v = part[((uint64_t)g * 2 + dir) * n_rows + p];
        if (v.x > s1) { s2 = s1; r2 = r1; s1 = v.x; r1 = v.y; }
        else if (v.x > s2) { s2 = v.x; r2 = v.y; }
        if (v.z > s2) { s2 = v.z; r2 = v.w; }                                                       // (never above s1: v.z <= v.x)
    }
    tops[q] = make_int4(s1, r1 >= 0 ? nz_ref[r1] : -1, s2, r2 >= 0 ? nz_ref[r2] : -1);
}

template <int MODE> void launch_sweep(mgta_ctx *ctx, const ChimArgs &a, unsigned grid) {
    hipLaunchKernelGGL(chimera_sweep_kernel<MODE>, dim3(grid), dim3(kSweepWaves * 64), 0, ctx->stream, a);
    MGTA_HIP_CHECK(hipGetLastError());
}

// steps 2 to 5 for one contig: t = its rows of tops (8 per row)
struct Pair { bool have = false; int32_t lref = -1, lscore = 0, rref = -1, rscore = 0; };
inline Pair pair_at(const int32_t *t, int b) {                          // breakpoint b, 1-based: P of row b, S of row b + 1
    const int32_t *p = t + (size_t)(b - 1) * 8, *s = t + (size_t)b * 8 + 4;
    Pair out;
    if (p[1] < 0 || s[1] < 0) return out;
    if (p[1] != s[1]) { out.have = true; out.lref = p[1]; out.lscore = p[0]; out.rref = s[1]; out.rscore = s[0]; return out; }
    const bool c1 = s[3] >= 0, c2 = p[3] >= 0;
    if (!c1 && !c2) return out;
    out.have = true;
    if (c1 && (!c2 || p[0] + s[2] >= p[2] + s[0])) { out.lref = p[1]; out.lscore = p[0]; out.rref = s[3]; out.rscore = s[2]; }
    else { out.lref = p[3]; out.lscore = p[2]; out.rref = s[1]; out.rscore = s[0]; }
    return out;
}

}  // namespace
}  // namespace mgta

using namespace mgta;

extern "C" {

int mgta_ctx_set_chimera_segment(mgta_ctx *ctx, int64_t columns) {
    if (!ctx) { set_error("mgta_ctx_set_chimera_segment: ctx must not be NULL"); return MGTA_EINVAL; }
    if (columns < 0) { set_error("mgta_ctx_set_chimera_segment: columns = %lld must not be negative", (long long)columns); return MGTA_EINVAL; }
    ctx->chimera_segment_cols = (uint64_t)columns;
    return MGTA_OK;
}

int mgta_ctx_set_chimera_groups(mgta_ctx *ctx, int64_t groups) {
    if (!ctx) { set_error("mgta_ctx_set_chimera_groups: ctx must not be NULL"); return MGTA_EINVAL; }
    if (groups < 0) { set_error("mgta_ctx_set_chimera_groups: groups = %lld must not be negative", (long long)groups); return MGTA_EINVAL; }
    ctx->chimera_groups = (uint64_t)groups;
    return MGTA_OK;
}

int mgta_seqs_chimera(mgta_ctx *ctx, const char *seqs, const uint64_t *offsets, int64_t n, const char *refs, const uint64_t *ref_offsets, int64_t n_ref,
                      const int8_t *sub, int32_t gap_open, int32_t gap_extend, int32_t min_seg, int32_t min_gain, mgta_chimera_rec *recs, int32_t *tops,
                      mgta_chimera_stats *stats) {
    if (!ctx) { set_error("mgta_seqs_chimera: ctx must not be NULL"); return MGTA_EINVAL; }
    if (n < 0) { set_error("mgta_seqs_chimera: n = %lld must not be negative", (long long)n); return MGTA_EINVAL; }
    if (n_ref < 0) { set_error("mgta_seqs_chimera: n_ref = %lld must not be negative", (long long)n_ref); return MGTA_EINVAL; }
    if (!check_seq_count("mgta_seqs_chimera", kContigs, n)) return MGTA_EINVAL;
    if (!check_seq_count("mgta_seqs_chimera", kReferences, n_ref)) return MGTA_EINVAL;
    if (gap_extend < 0 || gap_extend > gap_open || gap_open > 1024) {
        set_error("mgta_seqs_chimera: gap_open = %d, gap_extend = %d (the rule needs 0 <= gap_extend <= gap_open <= 1024)", gap_open, gap_extend);
        return MGTA_EINVAL;
    }
    if (min_seg < 1 || min_seg > kChimeraMaxLen) { set_error("mgta_seqs_chimera: min_seg = %d (the rule needs 1 <= min_seg <= %d)", min_seg, kChimeraMaxLen); return MGTA_EINVAL; }
    if (min_gain < 1 || min_gain > (1 << 20)) { set_error("mgta_seqs_chimera: min_gain = %d (the rule needs 1 <= min_gain <= 2^20)", min_gain); return MGTA_EINVAL; }
    if (n > 0 && !offsets) { set_error("mgta_seqs_chimera: offsets must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && !recs) { set_error("mgta_seqs_chimera: recs must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && !sub) { set_error("mgta_seqs_chimera: sub must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && n_ref > 0 && !ref_offsets) { set_error("mgta_seqs_chimera: ref_offsets must not be NULL"); return MGTA_EINVAL; }
    if (!check_seq_offsets("mgta_seqs_chimera", kContigs, offsets, n, kChimeraMaxLen)) return MGTA_EINVAL;
    if (!check_seq_offsets("mgta_seqs_chimera", kReferences, ref_offsets, n > 0 ? n_ref : 0, kChimeraMaxLen)) return MGTA_EINVAL;
    const uint64_t n_letters = n > 0 ? offsets[n] - offsets[0] : 0, n_cols = (n > 0 && n_ref > 0) ? ref_offsets[n_ref] - ref_offsets[0] : 0;
    if (!check_ref_columns("mgta_seqs_chimera", n_cols)) return MGTA_EINVAL;
    if (!check_seq_letters("mgta_seqs_chimera", kContigs, seqs, n_letters)) return MGTA_EINVAL;
    if (!check_seq_letters("mgta_seqs_chimera", kReferences, refs, n_cols)) return MGTA_EINVAL;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return MGTA_OK;
    return guarded("mgta_seqs_chimera", [&]() {
        const uint32_t nn = (uint32_t)n;
        mgta_chimera_rec none;
        memset(&none, 0, sizeof none);
        none.status = 2; none.ref = -1; none.left_ref = -1; none.right_ref = -1;
        if (stats) { stats->n_seqs = n; stats->n_refs = n_ref; }
        int32_t *tops_out = tops ? tops + offsets[0] * 8 : nullptr;       // row b of contig c at (offsets[c] + b - 1) * 8
        if (n_letters == 0 || n_cols == 0) {                              // no prefix and no suffix has a score
            for (uint32_t i = 0; i < nn; ++i) recs[i] = none;
            if (tops_out)
                for (uint64_t q = 0; q < n_letters * 4; ++q) { tops_out[q * 2] = INT32_MIN; tops_out[q * 2 + 1] = -1; }
            if (stats) stats->n_unchecked = n;
            return (int)MGTA_OK;
        }
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        uint64_t *live = &ctx->live_bytes, *peak = &ctx->peak_bytes;
        PeakOfCall peak_of_call(ctx);

        // the contigs: where they start, longest first
        const std::vector<uint64_t> rel = rel_offsets(offsets, n);
        const std::vector<uint32_t> order = longest_first(rel);
        const uint32_t l_max = (uint32_t)(rel[order[0] + 1] - rel[order[0]]);
        // the columns, forwards and, behind them, with every reference reversed in its place: class and first-column bit
        const uint32_t nc = (uint32_t)n_cols;
        std::vector<uint32_t> rstart;
        std::vector<uint8_t> rcls;
        ref_columns(refs, ref_offsets, n_ref, rstart, rcls);
        rcls.resize((size_t)nc * 2);
        std::vector<int32_t> nz_ref;                                      // the references that have residues
        std::vector<uint32_t> nz_at((size_t)n_ref + 1);                   // how many of them lie before reference r
        for (int64_t r = 0; r < n_ref; ++r) {
            const uint32_t b = rstart[(size_t)r], e = rstart[(size_t)r + 1];
            nz_at[(size_t)r] = (uint32_t)nz_ref.size();
            if (e == b) continue;
            nz_ref.push_back((int32_t)r);
            for (uint32_t g = b; g < e; ++g) rcls[(size_t)nc + (b + (e - 1 - g))] = rcls[g] & 31u;
            rcls[(size_t)nc + b] |= kFirstColumn;
        }
        nz_at[(size_t)n_ref] = (uint32_t)nz_ref.size();
        // segments: whole references, as few columns over the target as the last reference needs
        const uint64_t seg_cols = ctx->chimera_segment_cols ? ctx->chimera_segment_cols : kDefaultSegment;
        std::vector<uint2> seg;
        std::vector<uint32_t> segref{0u};
        uint32_t seg_from = 0;
        for (int64_t r = 0; r < n_ref; ++r) {
            const uint32_t e = rstart[(size_t)r + 1];
            if (e > seg_from && (uint64_t)(e - seg_from) >= seg_cols && e != nc) {
                seg.push_back(make_uint2(seg_from, e)); segref.push_back(nz_at[(size_t)r + 1]);
                seg_from = e;
            }
        }
        seg.push_back(make_uint2(seg_from, nc));
        const uint32_t n_seg = (uint32_t)seg.size();
        uint32_t w_max = 0;                                               // (no reference is longer: a segment holds whole references)
        for (uint32_t s = 0; s < n_seg; ++s) w_max = std::max(w_max, seg[s].y - seg[s].x);
        // groups of segments: one when the contigs fill the device, more when they are few
        const uint64_t want_items = (uint64_t)ctx->num_cus * 32;
        const uint64_t ask_groups = ctx->chimera_groups ? ctx->chimera_groups : (want_items + 2ull * nn - 1) / (2ull * nn);
        const uint32_t want_groups = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_seg, ask_groups));
        const uint32_t per_group = (n_seg + want_groups - 1) / want_groups;
        const uint32_t n_groups = (n_seg + per_group - 1) / per_group;    // none of them empty
        std::vector<ChimItem> items;
        items.reserve((size_t)nn * 2 * n_groups);
        for (uint32_t ci = 0; ci < nn; ++ci)
            for (uint32_t g = 0; g < n_groups; ++g)
                for (uint32_t dir = 0; dir < 2; ++dir) {
                    ChimItem it;
                    it.contig = order[ci]; it.dir = dir; it.seg_lo = std::min(n_seg, g * per_group); it.seg_hi = std::min(n_seg, (g + 1) * per_group);
                    it.col_add = dir ? nc : 0; it.out_base = ((uint64_t)g * 2 + dir) * n_letters;
                    items.push_back(it);
                }
        const uint64_t n_items = items.size();

        int bpc = 0;
        MGTA_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, chimera_sweep_kernel<0>, kSweepWaves * 64, 0));
        bpc = std::max(1, std::min(bpc, 4));                              // 16 waves a CU: every resident wave has a boundary buffer
        const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ctx->num_cus * (uint64_t)bpc, (n_items + kSweepWaves - 1) / kSweepWaves));
        const uint64_t bound_stride = l_max > 64 ? (((uint64_t)w_max + 63) & ~63ull) : 0;

        SeqStage dev;
        dev.upload(ctx, seqs, offsets, rel, nullptr);
        DevBuf d_rcls, d_seg, d_segref, d_items, d_sub, d_part, d_tops, d_nz, d_bound;
        d_rcls.alloc((size_t)nc * 2 + 16, live, peak);
        d_seg.alloc((size_t)n_seg * sizeof(uint2), live, peak);
        d_segref.alloc((size_t)n_seg * 4, live, peak);
        d_items.alloc((size_t)n_items * sizeof(ChimItem), live, peak);
        d_sub.alloc(27 * 27, live, peak);
        d_nz.alloc(nz_ref.size() * 4, live, peak);
        d_part.alloc((size_t)n_groups * 2 * n_letters * sizeof(int4), live, peak);
        d_tops.alloc((size_t)n_letters * 2 * sizeof(int4), live, peak);
        if (bound_stride) d_bound.alloc((size_t)grid * kSweepWaves * bound_stride * sizeof(int2), live, peak);
        MGTA_HIP_CHECK(hipMemcpyAsync(d_rcls.p, rcls.data(), (size_t)nc * 2, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_seg.p, seg.data(), (size_t)n_seg * sizeof(uint2), hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_segref.p, segref.data(), (size_t)n_seg * 4, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_items.p, items.data(), (size_t)n_items * sizeof(ChimItem), hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_sub.p, sub, 27 * 27, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_nz.p, nz_ref.data(), nz_ref.size() * 4, hipMemcpyHostToDevice, st));
        dev.reset_head(st);

        ChimArgs sa;
        memset(&sa, 0, sizeof sa);
        sa.seqs = dev.seqs.as<uint8_t>(); sa.off = dev.off.as<uint64_t>(); sa.rcls = d_rcls.as<uint8_t>(); sa.seg = d_seg.as<uint2>(); sa.segref = d_segref.as<uint32_t>();
        sa.items = d_items.as<ChimItem>(); sa.sub = d_sub.as<int8_t>(); sa.go = gap_open; sa.ge = gap_extend; sa.n_items = n_items; sa.n_rows = n_letters;
        sa.part = d_part.as<int4>(); sa.bound = bound_stride ? d_bound.as<int2>() : nullptr; sa.bound_stride = bound_stride; sa.head = dev.head.as<unsigned long long>();
        Timer t_top(st), t_par(st);
        t_top.start();
        launch_sweep<0>(ctx, sa, grid);
        hipLaunchKernelGGL(chimera_tops_kernel, dim3((unsigned)((n_letters * 2 + 255) / 256)), dim3(256), 0, st, d_part.as<int4>(), n_letters, n_groups, d_nz.as<int32_t>(),
                           d_tops.as<int4>());
        MGTA_HIP_CHECK(hipGetLastError());
        t_top.end();
        std::vector<int32_t> own_tops;
        if (!tops_out) { own_tops.resize((size_t)n_letters * 8); tops_out = own_tops.data(); }
        MGTA_HIP_CHECK(hipMemcpyAsync(tops_out, d_tops.p, (size_t)n_letters * 8 * 4, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        const double ms_top = t_top.ms();
        d_part.release(); d_tops.release(); d_items.release(); d_seg.release(); d_segref.release(); d_nz.release();

        // steps 2 and 3: the pair of every breakpoint, the break; the contigs that have one go to the parents pass
        struct Checked { uint32_t idx; int32_t brk, par[3]; Pair pair; };
        std::vector<Checked> checked;
        for (uint32_t i = 0; i < nn; ++i) {
            const int L = (int)(rel[i + 1] - rel[i]);
            const int32_t *t = tops_out + rel[i] * 8;
            recs[i] = none;
            if (L > 0 && t[(size_t)(L - 1) * 8 + 1] >= 0) { recs[i].ref = t[(size_t)(L - 1) * 8 + 1]; recs[i].score = t[(size_t)(L - 1) * 8]; }
            Checked c;
            c.idx = i; c.brk = 0;
            int64_t two = 0;
            for (int b = min_seg; b <= L - min_seg; ++b) {
                const Pair p = pair_at(t, b);
                if (p.have && (!c.brk || (int64_t)p.lscore + p.rscore > two)) { c.brk = b; c.pair = p; two = (int64_t)p.lscore + p.rscore; }
            }
            if (!c.brk) continue;
            c.par[0] = recs[i].ref >= 0 ? recs[i].ref : c.pair.lref; c.par[1] = c.pair.lref; c.par[2] = c.pair.rref;
            checked.push_back(c);
        }
        {                                                                 // longest first
            std::vector<Checked> sorted;
            sorted.reserve(checked.size());
            for (uint32_t q : longest_first((uint32_t)checked.size(), [&](uint32_t q) { return rel[checked[q].idx + 1] - rel[checked[q].idx]; })) sorted.push_back(checked[q]);
            checked.swap(sorted);
        }

        // step 4: the rows' maxima over N, A, B in both directions
        double ms_par = 0;
        int64_t par_cells = 0;
        const uint64_t n_par = checked.size();
        std::vector<int32_t> rowmax;
        if (n_par) {
            // an item's segments are its three references where they lie in the run: nothing is copied
            std::vector<uint2> pseg;
            std::vector<uint32_t> psegref;
            std::vector<ChimItem> pitems;
            pseg.reserve(n_par * 3); psegref.reserve(n_par * 3); pitems.reserve(n_par * 2);
            for (const Checked &c : checked) {
                const uint32_t lo = (uint32_t)pseg.size();
                for (int q = 0; q < 3; ++q) {
                    const uint32_t b = rstart[(size_t)c.par[q]], e = rstart[(size_t)c.par[q] + 1];
                    pseg.push_back(make_uint2(b, e)); psegref.push_back((uint32_t)q);
                    par_cells += 2 * (int64_t)(e - b) * (int64_t)(rel[c.idx + 1] - rel[c.idx]);
                }
                for (uint32_t dir = 0; dir < 2; ++dir) {
                    ChimItem it;
                    it.contig = c.idx; it.dir = dir; it.seg_lo = lo; it.seg_hi = lo + 3; it.col_add = dir ? nc : 0; it.out_base = (uint64_t)dir * 3 * n_letters;
                    pitems.push_back(it);
                }
            }
            DevBuf d_pseg, d_psegref, d_pitems, d_rowmax;
            d_pseg.alloc(pseg.size() * sizeof(uint2), live, peak);
            d_psegref.alloc(psegref.size() * 4, live, peak);
            d_pitems.alloc(pitems.size() * sizeof(ChimItem), live, peak);
            d_rowmax.alloc((size_t)n_letters * 6 * 4, live, peak);
            MGTA_HIP_CHECK(hipMemcpyAsync(d_pseg.p, pseg.data(), pseg.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
            MGTA_HIP_CHECK(hipMemcpyAsync(d_psegref.p, psegref.data(), psegref.size() * 4, hipMemcpyHostToDevice, st));
            MGTA_HIP_CHECK(hipMemcpyAsync(d_pitems.p, pitems.data(), pitems.size() * sizeof(ChimItem), hipMemcpyHostToDevice, st));
            dev.reset_head(st);
            ChimArgs pa = sa;
            pa.seg = d_pseg.as<uint2>(); pa.segref = d_psegref.as<uint32_t>(); pa.items = d_pitems.as<ChimItem>(); pa.n_items = pitems.size();
            pa.part = nullptr; pa.rowmax = d_rowmax.as<int32_t>();
            const unsigned pgrid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(grid, (pitems.size() + kSweepWaves - 1) / kSweepWaves));   // never more waves than buffers
            t_par.start();
            launch_sweep<1>(ctx, pa, pgrid);
            t_par.end();
            rowmax.resize((size_t)n_letters * 6);
            MGTA_HIP_CHECK(hipMemcpyAsync(rowmax.data(), d_rowmax.p, (size_t)n_letters * 6 * 4, hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
            ms_par = t_par.ms();
        }

        // steps 4 and 5
        int64_t n_chim = 0;
        for (const Checked &c : checked) {
            const uint32_t i = c.idx;
            const int L = (int)(rel[i + 1] - rel[i]);
            int64_t one = recs[i].ref >= 0 ? (int64_t)recs[i].score : INT64_MIN;
            for (int q = 0; q < 3; ++q) {
                const int32_t *P = rowmax.data() + (size_t)q * n_letters + rel[i], *S = rowmax.data() + (size_t)(3 + q) * n_letters + rel[i];
                for (int b = min_seg; b <= L - min_seg; ++b)
                    if (P[b - 1] != INT32_MIN && S[b] != INT32_MIN) one = std::max(one, (int64_t)P[b - 1] + S[b]);
            }
            if (one == INT64_MIN) { set_error("mgta_seqs_chimera: contig %u: a pair of parents and no single parent", i); return (int)MGTA_EHIP; }
            mgta_chimera_rec &r = recs[i];
            r.brk = c.brk; r.left_ref = c.pair.lref; r.left_score = c.pair.lscore; r.right_ref = c.pair.rref; r.right_score = c.pair.rscore;
            r.two = c.pair.lscore + c.pair.rscore; r.one = (int32_t)one; r.gain = r.two - r.one;
            r.status = r.gain >= min_gain ? 1 : 0;
            n_chim += r.status;
        }
        if (stats) {
            const unsigned __int128 all_cells = (unsigned __int128)n_letters * n_cols * 2;
            stats->n_chimeric = n_chim; stats->n_clean = (int64_t)n_par - n_chim; stats->n_unchecked = n - (int64_t)n_par;
            stats->n_cells = all_cells > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)all_cells;
            stats->n_parent_cells = par_cells; stats->n_items = (int64_t)n_items; stats->n_parent_items = (int64_t)n_par * 2; stats->n_segments = n_seg;
            stats->n_groups = n_groups; stats->grid_blocks = grid; stats->waves_per_block = kSweepWaves; stats->blocks_per_cu = bpc; stats->lds_bytes = kSubLdsBytes;
            stats->bound_bytes = (int64_t)((uint64_t)grid * kSweepWaves * bound_stride * sizeof(int2)); stats->peak_bytes = (int64_t)ctx->peak_bytes;
            stats->ms_top = ms_top; stats->ms_parents = ms_par;
        }
        return (int)MGTA_OK;
    });
}

}  // extern "C"
