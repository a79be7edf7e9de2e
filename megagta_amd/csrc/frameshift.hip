// frameshift.hip — the closest reference protein of every NUCLEOTIDE contig, with shifts of the reading frame by one nucleotide
// (mgta_seqs_frameshift): the place of FrameBot on the nucleotide representatives in the reference's bin/post_proc.sh:106-109.  The rule
// is this library's own (include/megagta_hip.h): rows are nucleotide positions, a match state consumes three letters (a codon), two (one
// letter missing, the residue unknown) or four (one letter too many, the first dropped), an insert state a whole codon, a delete
// state a reference residue; global in the contig, local in the reference, int32, first candidate wins a tie.
//
// The shape is nearest.hip's: a score pass over (contig, segment of the reference concatenation) items, longest contig first from one
// atomic head, one wave per item, lanes own reference columns 64 at a time (a strip), lane l computes row i = t - l + 1 at step t; a
// trace pass over the (contig, nearest reference) pairs in batches with one byte per cell; a walk with one thread per pair.  What is
// different is how far back a cell looks.  With P = max(M, X, Y) (preference M, X, Y) the lane of cell (i, j) computes
//     P  = P[i][j]                               a candidate of M[i+3][j+1], M[i+2][j+1] and M[i+4][j+1]
//     Y' = max(M[i][j] - go, Y[i][j] - ge)       Y[i][j+1]                        (taken by lane l + 1 at the next step)
//     X' = max(M[i][j] - go, X[i][j] - ge)       X[i+3][j]                        (its own, three steps later)
// P and Y' move to lane l + 1 by one DPP wave shift each, as does the class of the codon that ends at the row.  The receiving lane keeps
// the last four P it was given in h1 .. h4 (P[i-1 .. i-4][j-1] at row i) and its own last three X' in x1 .. x3, all named registers
// rotated by hand: no array, nothing indexed by a lane or a loop variable, no scratch.  What arrives is put right ON ARRIVAL, so that
// the history is exact at every depth: the row-0 value is 0 (B, against any column), rows below 0 are undefined, and a lane on the
// first column of its reference takes undefined for every row >= 1, so nothing crosses a reference boundary however old.  Lane 0 takes
// P and Y' of lane 63 of the strip before from the wave's boundary rows in LDS (one wave, LDS in program order: row t is read before
// the rows <= t - 63 are written, in place).  The class of a(i), the residue of the codon that ends at row i, is computed once per item
// into LDS, one byte per row; the cell loop translates nothing.
//   MODE 0  the score pass.   MODE 1  the score pass that also fills `scores` (atomicMax per defined cell of the last row).
//   MODE 2  the trace pass: every cell stores one byte, bits 0-1 the state P came from (0 M, 1 X, 2 Y), bits 2-3 the candidate M took
//           (0 codon, 1 short, 2 long), bit 4 Y' came from Y, bit 5 X' came from X, at ((i - 1 + l) mod L) * w + l of its strip (tb_at).
//           B is implied: a match state whose candidate leads to row 0 began the alignment.
//
// Range.  A path has at most 4096 residue-consuming states (each takes a reference column), at most 4096 insert states (each takes
// three of at most 12288 letters), at most 4096 delete states, and a shift only in a residue-consuming state: a defined value is at
// most 127 * 4096 in substitution scores and at most 1024 * (4096 + 4096 + 4096) in costs, 13 103 104 < 2^24 in magnitude.  A value
// derived from the sentinel kUndef = -2^30 is the sentinel plus the terms of a monotone path inside one strip run: at most 12288 + 4096
// cells and 128 more on lanes outside the rows, each term between -(128 + 1024 + 1024) and +127, so it stays inside
// [-2^30 - 3.6e7, -2^30 + 2.1e6]: below kDefinedFloor = -2^29, below every defined value, above INT32_MIN.
#include <algorithm>
#include <vector>

#include "frameshift_seq.hpp"
#include "seq_dp.hpp"

namespace mgta {
namespace {

constexpr int kFrameshiftMaxLen = 12288;            // nucleotides of a contig: 9 bytes of LDS per row of the wave that owns it
constexpr int kFrameshiftMaxRef = 4096;             // residues of a reference; also the stride of the caller's path slots
constexpr size_t kFrameshiftLdsBudget = 80 * 1024;  // of a workgroup while the longest contig allows it: two fit a CU
constexpr int kClassX = 24;                         // c('X')

struct FsSweepArgs {
    const uint8_t *seqs;         // the nucleotides of every contig
    const uint64_t *off;         // [n + 1] into seqs
    const uint32_t *order;       // contig numbers, longest first (MODE 2: the batch's)
    const uint8_t *rcls;         // [n_cols] class | kFirstColumn of every reference column
    const uint32_t *seg;         // MODE 0, 1: [n_seg + 1] the columns where the segments start
    const uint32_t *pair_c0;     // MODE 2: [n_items] first column of the item's reference
    const uint32_t *pair_w;      // MODE 2: [n_items] its columns
    const uint64_t *cell_base;   // MODE 2: [n_items] where the traceback bytes of the item start
    const int32_t *col_ref;      // MODE 1: [n_cols] the reference of a column
    const int8_t *sub;           // [27 * 27]
    int32_t go, ge, fs;
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

__device__ __forceinline__ unsigned long long fs_wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

template <int MODE>
__global__ __launch_bounds__(256) void frameshift_sweep_kernel(FsSweepArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    // [sub 27 x 32 B][boundary: waves x rows_lds x (P, Y')][codon classes: waves x rows_lds B]
    int8_t *s_sub = reinterpret_cast<int8_t *>(lds_raw);
    const int n_waves = blockDim.x >> 6;
    int2 *s_bound = reinterpret_cast<int2 *>(lds_raw + kSubLdsBytes) + (size_t)wave_id() * a.rows_lds;
    uint8_t *s_x = lds_raw + kSubLdsBytes + (size_t)n_waves * a.rows_lds * 8 + (size_t)wave_id() * a.rows_lds;
    stage_sub(s_sub, a.sub);
    const int lane = lane_id();
    const int32_t go = a.go, ge = a.ge, fs = a.fs;

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
        // c(a(i)) of row i at s_x[i - 1]; rows 1 and 2 end no codon (their class is never part of a defined value)
        for (int p = lane; p < L; p += 64) s_x[p] = p >= 2 ? (uint8_t)residue_class((uint8_t)codon_residue_at(a.seqs + o0, p + 1)) : (uint8_t)0;
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
            const int32_t ufs = (int32_t)s_sub[cy32 + kClassX] - fs;      // u(j) - frameshift
            const int32_t ref_id = (MODE == 1 && own) ? a.col_ref[g] : 0;
            const bool last_strip = s == n_strips - 1;
            uint8_t *tbs = MODE == 2 ? tb + (size_t)s * 64 * L : nullptr;
            // this lane starts at row 1 - lane: P of the rows before it in the column to the left is B (0) at row 0 and undefined below
            int32_t h1 = lane == 0 ? 0 : kUndef, h2 = kUndef, h3 = kUndef, h4 = kUndef;
            int32_t x1 = kUndef, x2 = kUndef, x3 = kUndef;
            int32_t p_out = kUndef, y_out = kUndef, cx_out = 0;
            const int n_steps = L + w - 1;
            int i = 1 - lane;                                             // this lane's row
            int t_mod = 0;                                                // t mod L
            for (int t = 0; t < n_steps; ++t, ++i) {
                // lane 0's row is t + 1: every lane reads its slot (one address, a broadcast) and only lane 0 keeps it
                const int r0 = min(t, L - 1);
                const int2 bd = s_bound[r0];
                const int32_t cx0 = s_x[r0];
                // what the left neighbour computed at the last step: P[i][j-1], Y[i][j], the class of a(i); put right on arrival
                int32_t p_new = from_left(p_out, bd.x), v_y = from_left(y_out, bd.y);
                const int32_t cx = from_left(cx_out, cx0);
                cx_out = cx;
                if (first) { p_new = kUndef; v_y = kUndef; }
                if (i <= 0) p_new = i == 0 ? 0 : kUndef;
                const int32_t e = (int32_t)s_sub[cy32 + cx];
                const int32_t c_codon = h3 + e, c_short = h2 + ufs, c_long = h4 + e - fs;
                const int32_t v_x = x3;
                h4 = h3; h3 = h2; h2 = h1; h1 = p_new;
                int32_t v_m = c_codon, P, Y, X;
                if (MODE == 2) {
                    uint32_t ch = 0;
                    if (c_short > v_m) { v_m = c_short; ch = 4; }
                    if (c_long > v_m) { v_m = c_long; ch = 8; }
                    const int32_t open = v_m - go, y_ext = v_y - ge, x_ext = v_x - ge;
                    P = v_m; Y = open; X = open;
                    if (v_x > P) { P = v_x; ch |= 1; }
                    if (v_y > P) { P = v_y; ch = (ch & ~3u) | 2; }
                    if (y_ext > Y) { Y = y_ext; ch |= 16; }
                    if (x_ext > X) { X = x_ext; ch |= 32; }
                    if (own && i >= 1 && i <= L) tbs[(size_t)t_mod * w + lane] = (uint8_t)ch;   // (i - 1 + lane) mod L = t mod L
                    if (++t_mod == L) t_mod = 0;
                } else {
                    v_m = max(max(c_codon, c_short), c_long);
                    const int32_t open = v_m - go;
                    P = max(max(v_m, v_x), v_y); Y = max(open, v_y - ge); X = max(open, v_x - ge);
                }
                if (own && i == L) {
                    if (v_m > best) { best = v_m; best_g = g; }           // strips ascend: an equal score keeps the lower column
                    if (MODE == 1 && v_m >= kDefinedFloor) atomicMax(a.scores + (size_t)idx * a.n_ref + (size_t)ref_id, v_m);
                }
                if (!last_strip && lane == 63 && i >= 1 && i <= L) s_bound[i - 1] = make_int2(P, Y);
                p_out = P; y_out = Y;
                x3 = x2; x2 = x1; x1 = X;
            }
            wave_lds_fence();
        }
        // the score and the lowest column that reaches it
        const unsigned long long key = fs_wave_max_u64(((unsigned long long)((uint32_t)best ^ 0x80000000u) << 32) | (uint32_t)~best_g);
        if (lane == 0) {
            if (MODE == 2) {
                a.score[k] = (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
                a.jend[k] = (int32_t)(~(uint32_t)key - c0) + 1;
            } else a.keys[k] = key;
        }
    }
}

struct FsWalkArgs {
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
    mgta_frameshift_rec *recs;   // [count]; ref is the host's to fill
    char *path;                  // or NULL
    int32_t *path_len;           // [count] (with path)
};

// One thread per pair walks the bytes back from the match state of (L, lowest end column).  A match state goes 3, 2 or 4 rows up and
// one column left, and began the alignment when that is row 0; an insert state 3 rows up; a delete state one column left.
__global__ __launch_bounds__(256) void frameshift_trace_kernel(FsWalkArgs a) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.count) return;
    const uint32_t idx = a.order[k];
    const uint64_t o0 = a.off[idx];
    const int L = (int)(a.off[idx + 1] - o0), W = (int)a.pair_w[k];
    const int32_t score = a.score[k];
    mgta_frameshift_rec r;
    r.status = 1; r.ref = -1; r.score = 0; r.ref_from = 0; r.ref_to = 0; r.n_match = 0; r.n_ident = 0; r.n_insert = 0; r.n_delete = 0; r.n_short = 0; r.n_long = 0;
    int plen = 0;
    if (L > 0 && W > 0 && score >= kDefinedFloor) {
        const uint8_t *x = a.seqs + o0;
        const uint8_t *y = a.rcls + a.pair_c0[k];
        const uint8_t *tb = a.tb + a.cell_base[k];
        char *slot = a.path ? a.path + a.path_base[k] : nullptr;
        const int slot_len = L + W;
        r.status = 0; r.score = score; r.ref_to = a.jend[k];
        int i = L, j = a.jend[k], state = 0;
        // every step consumes two letters at least or a column: fewer than L + W of them
        for (int guard = 0; guard < L + W && i >= 1 && j >= 1 && j <= W; ++guard) {
            if (state == 0) {
                const uint32_t cand = (tb_at(tb, L, W, i, j) >> 2) & 3u;
                if (slot) slot[slot_len - 1 - plen] = cand == 0 ? 'M' : cand == 1 ? '<' : '>';
                ++plen;
                if (cand == 1) ++r.n_short;
                else {
                    if (cand == 0) ++r.n_match; else ++r.n_long;
                    const uint32_t cx = residue_class((uint8_t)codon_residue_at(x, i)), cy = y[j - 1] & 31u;
                    r.n_ident += cx == cy && cx != 0;
                }
                r.ref_from = j;
                i -= cand == 0 ? 3 : cand == 1 ? 2 : 4;
                --j;
                if (i <= 0 || j == 0) break;                              // B (i == 0); the rest is not reached: such a state has no score
                state = tb_at(tb, L, W, i, j) & 3;
            } else if (state == 1) {
                if (slot) slot[slot_len - 1 - plen] = 'I';
                ++plen;
                ++r.n_insert;
                if (i <= 3) break;                                        // (not reached: rows 1 .. 3 have no insert state)
                state = (tb_at(tb, L, W, i - 3, j) & 32) ? 1 : 0;
                i -= 3;
            } else {
                if (slot) slot[slot_len - 1 - plen] = 'D';
                ++plen;
                ++r.n_delete;
                if (j == 1) break;                                        // (not reached: column 1 has no delete state)
                state = (tb_at(tb, L, W, i, j - 1) & 16) ? 2 : 0;
                --j;
            }
        }
        if (slot)
            for (int p = 0; p < plen; ++p) slot[p] = slot[slot_len - plen + p];   // forwards: the source is never behind the target
    }
    a.recs[k] = r;
    if (a.path_len) a.path_len[k] = plen;
}

}  // namespace
}  // namespace mgta

using namespace mgta;

extern "C" {

int mgta_seqs_frameshift(mgta_ctx *ctx, const char *nucl, const uint64_t *offsets, int64_t n, const char *refs, const uint64_t *ref_offsets, int64_t n_ref,
                         const int8_t *sub, int32_t gap_open, int32_t gap_extend, int32_t frameshift, mgta_frameshift_rec *recs, int32_t *scores, char *path,
                         int32_t *path_len, mgta_frameshift_stats *stats) {
    static const SeqWords kNuclContigs{"contig", "n", "offsets", "nucl"};
    if (!ctx) { set_error("mgta_seqs_frameshift: ctx must not be NULL"); return MGTA_EINVAL; }
    if (n < 0) { set_error("mgta_seqs_frameshift: n = %lld must not be negative", (long long)n); return MGTA_EINVAL; }
    if (n_ref < 0) { set_error("mgta_seqs_frameshift: n_ref = %lld must not be negative", (long long)n_ref); return MGTA_EINVAL; }
    if (!check_seq_count("mgta_seqs_frameshift", kNuclContigs, n)) return MGTA_EINVAL;
    if (!check_seq_count("mgta_seqs_frameshift", kReferences, n_ref)) return MGTA_EINVAL;
    if (gap_extend < 0 || gap_extend > gap_open || gap_open > 1024) {
        set_error("mgta_seqs_frameshift: gap_open = %d, gap_extend = %d (the rule needs 0 <= gap_extend <= gap_open <= 1024)", gap_open, gap_extend);
        return MGTA_EINVAL;
    }
    if (frameshift < 0 || frameshift > 1024) {
        set_error("mgta_seqs_frameshift: frameshift = %d (the rule needs 0 <= frameshift <= 1024)", frameshift);
        return MGTA_EINVAL;
    }
    if (n > 0 && !offsets) { set_error("mgta_seqs_frameshift: offsets must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && !recs) { set_error("mgta_seqs_frameshift: recs must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && !sub) { set_error("mgta_seqs_frameshift: sub must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && n_ref > 0 && !ref_offsets) { set_error("mgta_seqs_frameshift: ref_offsets must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && path && !path_len) { set_error("mgta_seqs_frameshift: path_len must not be NULL when path is given"); return MGTA_EINVAL; }
    if (!check_seq_offsets("mgta_seqs_frameshift", kNuclContigs, offsets, n, kFrameshiftMaxLen, "nucleotides")) return MGTA_EINVAL;
    if (!check_seq_offsets("mgta_seqs_frameshift", kReferences, ref_offsets, n > 0 ? n_ref : 0, kFrameshiftMaxRef)) return MGTA_EINVAL;
    const uint64_t n_letters = n > 0 ? offsets[n] - offsets[0] : 0, n_cols = (n > 0 && n_ref > 0) ? ref_offsets[n_ref] - ref_offsets[0] : 0;
    if (!check_ref_columns("mgta_seqs_frameshift", n_cols)) return MGTA_EINVAL;
    if (!check_seq_letters("mgta_seqs_frameshift", kNuclContigs, nucl, n_letters)) return MGTA_EINVAL;
    if (!check_seq_letters("mgta_seqs_frameshift", kReferences, refs, n_cols)) return MGTA_EINVAL;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return MGTA_OK;
    return guarded("mgta_seqs_frameshift", [&]() {
        const uint32_t nn = (uint32_t)n;
        mgta_frameshift_rec none;
        memset(&none, 0, sizeof none);
        none.status = 1; none.ref = -1;
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

        // waves of a workgroup by the longest contig: inside the budget while one wave's rows allow it, else one wave with all it needs
        const uint32_t l_max = (uint32_t)(rel[order[0] + 1] - rel[order[0]]);
        const uint32_t rows_lds = (std::max(1u, l_max) + 7u) & ~7u;
        const int waves = waves_that_fit(rows_lds, 9, kSubLdsBytes, kFrameshiftLdsBudget);
        const size_t lds = kSubLdsBytes + (size_t)waves * rows_lds * 9;

        SeqStage dev;
        dev.upload(ctx, nucl, offsets, rel, &order);
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

        FsSweepArgs sa;
        memset(&sa, 0, sizeof sa);
        sa.seqs = dev.seqs.as<uint8_t>(); sa.off = dev.off.as<uint64_t>(); sa.order = dev.order.as<uint32_t>(); sa.rcls = d_rcls.as<uint8_t>(); sa.seg = d_seg.as<uint32_t>();
        sa.col_ref = d_colref.as<int32_t>(); sa.sub = d_sub.as<int8_t>(); sa.go = gap_open; sa.ge = gap_extend; sa.fs = frameshift; sa.n_items = n_items; sa.n_seg = n_seg;
        sa.n_ref = (uint64_t)n_ref; sa.keys = d_keys.as<unsigned long long>(); sa.scores = d_scores.as<int32_t>(); sa.rows_lds = rows_lds;
        sa.head = dev.head.as<unsigned long long>();
        Timer t_score(st), t_trace(st);
        t_score.start();
        const WaveLaunch sweep = launch_waves(ctx, scores ? frameshift_sweep_kernel<1> : frameshift_sweep_kernel<0>, sa, waves, lds, n_items);
        t_score.end();
        std::vector<unsigned long long> keys((size_t)n_items);
        MGTA_HIP_CHECK(hipMemcpyAsync(keys.data(), d_keys.p, (size_t)n_items * 8, hipMemcpyDeviceToHost, st));
        if (scores) MGTA_HIP_CHECK(hipMemcpyAsync(scores, d_scores.p, (size_t)n * (size_t)n_ref * 4, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        const double ms_score = t_score.ms();
        d_keys.release(); d_scores.release(); d_colref.release(); d_seg.release();

        // the nearest reference of every contig: the largest key of its items
        std::vector<uint32_t> t_order;                                    // the aligned contigs, longest first
        std::vector<uint32_t> near_ref(nn, 0);
        for (uint32_t ci = 0; ci < nn; ++ci) {
            const uint32_t idx = order[ci];
            unsigned long long key = 0;
            for (uint32_t s = 0; s < n_seg; ++s) key = std::max(key, keys[(size_t)ci * n_seg + s]);
            const int32_t best = (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
            recs[idx] = none;
            if (path) path_len[idx] = 0;
            if (best < kDefinedFloor) continue;
            const uint32_t g = ~(uint32_t)key;
            near_ref[idx] = (uint32_t)(std::upper_bound(rstart.begin(), rstart.end(), g) - rstart.begin()) - 1;   // the last reference that starts at or before g
            t_order.push_back(idx);
        }
        const uint32_t n_al = (uint32_t)t_order.size();

        const uint64_t cap = batch_cap(ctx, ctx->nearest_batch_cells, 1);    // one traceback byte per cell
        double ms_trace = 0;
        int64_t n_batches = 0, n_trace_cells = 0, n_shifted = 0;
        if (n_al) MGTA_HIP_CHECK(hipMemcpyAsync(dev.order.p, t_order.data(), (size_t)n_al * 4, hipMemcpyHostToDevice, st));
        std::vector<uint64_t> cell_base, path_base;
        std::vector<uint32_t> pair_c0, pair_w;
        std::vector<mgta_frameshift_rec> h_recs;
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
            d_recs.alloc((size_t)count * sizeof(mgta_frameshift_rec), live, peak);
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

            FsSweepArgs fa = sa;
            fa.order = dev.order.as<uint32_t>() + b0; fa.seg = nullptr; fa.col_ref = nullptr; fa.keys = nullptr; fa.scores = nullptr; fa.n_seg = 1;
            fa.pair_c0 = d_c0.as<uint32_t>(); fa.pair_w = d_w.as<uint32_t>(); fa.cell_base = d_cbase.as<uint64_t>(); fa.n_items = count;
            fa.tb = d_tb.as<uint8_t>(); fa.score = d_score.as<int32_t>(); fa.jend = d_jend.as<int32_t>();
            t_trace.start();
            launch_waves(ctx, frameshift_sweep_kernel<2>, fa, waves, lds, count);
            FsWalkArgs wa;
            wa.seqs = fa.seqs; wa.off = fa.off; wa.order = fa.order; wa.rcls = fa.rcls; wa.pair_c0 = fa.pair_c0; wa.pair_w = fa.pair_w; wa.cell_base = fa.cell_base;
            wa.path_base = d_pbase.as<uint64_t>(); wa.count = count; wa.tb = fa.tb; wa.score = fa.score; wa.jend = fa.jend; wa.recs = d_recs.as<mgta_frameshift_rec>();
            wa.path = path ? d_path.as<char>() : nullptr; wa.path_len = path ? d_plen.as<int32_t>() : nullptr;
            hipLaunchKernelGGL(frameshift_trace_kernel, dim3((count + 255) / 256), dim3(256), 0, st, wa);
            MGTA_HIP_CHECK(hipGetLastError());
            t_trace.end();

            h_recs.resize(count);
            MGTA_HIP_CHECK(hipMemcpyAsync(h_recs.data(), d_recs.p, (size_t)count * sizeof(mgta_frameshift_rec), hipMemcpyDeviceToHost, st));
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
                    set_error("mgta_seqs_frameshift: contig %u: the trace pass found no score where the score pass found one", idx);
                    return (int)MGTA_EHIP;
                }
                recs[idx] = h_recs[k];
                recs[idx].ref = (int32_t)near_ref[idx];
                n_shifted += (h_recs[k].n_short + h_recs[k].n_long) > 0;
                if (path) {
                    path_len[idx] = h_plen[k];
                    memcpy(path + offsets[idx] + (uint64_t)idx * kFrameshiftMaxRef, h_path.data() + path_base[k], (size_t)h_plen[k]);
                }
            }
            n_trace_cells += (int64_t)cells; ++n_batches;
            b0 = b1;
        }
        if (stats) {
            stats->n_unaligned = n - (int64_t)n_al; stats->n_trace_cells = n_trace_cells; stats->n_batches = n_batches; stats->n_segments = n_seg;
            stats->blocks_per_cu = sweep.blocks_per_cu; stats->waves_per_block = waves; stats->grid_blocks = sweep.grid; stats->lds_bytes = (int64_t)lds;
            stats->peak_bytes = (int64_t)ctx->peak_bytes; stats->ms_score = ms_score; stats->ms_trace = ms_trace; stats->n_shifted = n_shifted;
        }
        return (int)MGTA_OK;
    });
}

}  // extern "C"
