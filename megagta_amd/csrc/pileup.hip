// pileup.hip — the reads placed on a gene's contigs: per-base depth, the reads that fit a contig end to end and the positions where the
// reads disagree with it (mgta_reads_pileup; the rule is this project's own and is stated in include/megagta_hip.h).
//
// Four phases.  (1) Keys: both strands of every contig (one batch of cut_batch, contig_jobs.hpp) go through share_walk_kernel into
// the edge-keyed table (walk.hpp: sample_table_alloc, stage_symbols, queue_launch), exactly as the per-library coverage does it,
// marks included: every window keeps the slot of its own edge and of the edge of its reverse complement.  (2) Occurrence index: per
// key the list of (contig, window, strand) that lie on it -- a count per key, a prefix sum (scan.hpp) and a fill through an atomic
// cursor; the order inside a key is the device's and no output depends on it.  (3) The read scan, below.  (4) One wave per contig
// over its counts for the per-contig record.
//
// The read scan.  A group of 8 lanes owns a read (32 groups per workgroup, reads from one atomic head), walks it
// as sample_scan_kernel does and leaves one word per window in the group's own scratch row: 0 = no edge, the slot of its key, or "an
// edge that is no key".  A window on a key has, per occurrence, one anchor (o, p, i, q) on the diagonal d = q - p.  Candidates are
// never listed: an anchor whose left neighbour on the diagonal is an anchor too (window p - 1 has an edge and c[q - 1] = s[p - 1]:
// one byte compare) is skipped; every other anchor -- a run start -- is verified along the whole overlap, the lanes comparing 8
// letters a step, and the same sweep counts the anchors of the diagonal (runs of k + 1 equal letters whose window has an edge) and
// finds the first of them.  Only the first anchor of a diagonal owns the candidate, so a candidate is judged once whatever the number
// of its runs.  Pass one keeps the best score, the number of candidates that have it and the lowest of them; pass two repeats the
// sweeps, leaving one as soon as its mismatches put it below that score, and commits the candidates that have it: integer atomicAdds,
// so no order matters.  Every loop is bounded by a read length, an occurrence count or the table size; no workgroup waits for
// another.
//
// The gapped scan (mgta_reads_pileup_gapped) is the same body as a template.  Its pass one also leaves every candidate in a list of
// the read's diagonals (the group's own row, sized on the host for the most a read of the call can have); gap_pass judges every
// ordered pair of them on one (contig, orient) within max_gap: the breakpoint sweep over the legal b, then one sweep per side.  Pass
// two commits the ungapped and the gapped candidates of the best score; gap records go through one atomic cursor and the host sorts
// them.  Its loops are bounded by the list and the read's length.
#include <algorithm>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "device_utils.hpp"
#include "graph.hpp"
#include "scan.hpp"
#include "walk.hpp"

namespace mgta {
namespace {

constexpr uint32_t kPileNoKey = 0xFFFFFFFFu;      // a window with an edge that is no key of the call
constexpr uint32_t kPileMaxRead = 65535;
constexpr uint64_t kPileScratchBytes = 1ull << 30;   // most bytes of per-window words of the groups in flight

enum { PC_HEAD, PC_WALKED, PC_SEARCHED, PC_HITS, PC_WINDOWS, PC_READS_CAND, PC_CAND, PC_VERIFIED, PC_PLACED, PC_MULTI, PC_PLACEMENTS, PC_PILED, PC_NUM };

struct PileArgs {
    const uint32_t *packed;
    const uint64_t *start;
    uint64_t n_reads;
    int reversed;
    uint32_t chunk;
    const uint32_t *marks;
    SampleTable t;
    const uint8_t *sym;               // the contigs' symbols as given (1..4, 0 = no base)
    const uint64_t *coff;             // [n + 1] first letter of every contig
    const uint64_t *occ_off;          // [n_keys + 2] by key number
    const uint64_t *occ;              // contig << 33 | window << 1 | strand
    uint32_t *counts, *uniq;
    unsigned long long *ctg;          // [n][3] placements, unique placements, mismatches
    mgta_read_place *per_read;        // or NULL
    uint32_t *wv;                     // one row of wv_stride words per group in flight
    uint64_t wv_stride;
    int min_anchors, min_overlap, max_permille;
    unsigned long long *counters;
};

// ---- the gapped scan (mgta_reads_pileup_gapped): what it has beyond PileArgs

struct DiagEnt {                      // one ungapped candidate of the read at hand: a diagonal with its first and last anchor
    int64_t d;
    uint32_t ci, o, first, last;
};

enum { GC_CURSOR, GC_CAND, GC_PASS, GC_READS, GC_PLACED, GC_INS, GC_DEL, GC_OVERFLOW, GC_NUM };

struct GapArgs {
    DiagEnt *list;                    // one row of list_stride entries per group in flight
    uint64_t list_stride;
    mgta_gap_place *per_read;         // or NULL (PileArgs::per_read is NULL in this scan)
    mgta_gap_rec *gaps;               // [gap_cap]; records beyond it are counted and not written
    uint64_t gap_cap;
    int max_gap, gap_open, gap_extend;
    unsigned long long *gcnt;         // [GC_NUM]
};

// the occurrences per key: a window as given lies on the key of its own edge (strand 0), and its reverse complement on the key of that
// one's edge (strand 1; only where the window itself has an edge: an anchor is a window of the contig as given)
__global__ __launch_bounds__(256) void pile_occ_count_kernel(const uint32_t *own, const uint32_t *rc, const uint32_t *dense, uint64_t n_win, uint32_t *cnt) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < n_win; w += stride) {
        const uint32_t so = own[w], sr = rc[w];
        if (!so) continue;
        atomicAdd(&cnt[dense[so]], 1u);
        if (sr) atomicAdd(&cnt[dense[sr]], 1u);
    }
}

// one wave per contig
__global__ __launch_bounds__(256) void pile_occ_fill_kernel(const uint64_t *woff, uint32_t n, const uint32_t *own, const uint32_t *rc, const uint32_t *dense,
                                                            const uint64_t *occ_off, uint32_t *cursor, uint64_t *occ) {
    const uint32_t i = blockIdx.x * 4 + (uint32_t)wave_id();
    if (i >= n) return;
    const uint64_t b = woff[i];
    const uint32_t n_win = (uint32_t)(woff[i + 1] - b);
    for (uint32_t q = lane_id(); q < n_win; q += 64) {
        const uint32_t so = own[b + q], sr = rc[b + q];
        if (!so) continue;
        const uint64_t v = ((uint64_t)i << 33) | ((uint64_t)q << 1);
        const uint32_t d0 = dense[so];
        occ[occ_off[d0] + atomicAdd(&cursor[d0], 1u)] = v;
        if (sr) {
            const uint32_t d1 = dense[sr];
            occ[occ_off[d1] + atomicAdd(&cursor[d1], 1u)] = v | 1ull;
        }
    }
}

// One pass over the anchors of a read.  COMMIT = false: the best score, its ties and the lowest of them.  COMMIT = true: the adds of
// the candidates with the best score.  All 8 lanes of the group run the same control flow on the same values.
// LIST (pass one of the gapped scan): every candidate, passing or not, is also left in the group's list with its first and last anchor.
template <bool COMMIT, bool LIST = false>
__device__ __forceinline__ void pile_pass(const PileArgs &A, int k, int a, uint64_t s0, uint32_t len, uint32_t n_win, const uint32_t *wvp, int sub, int lane,
                                          int &best, uint32_t &ties, uint32_t &lo_c, int &lo_o, int64_t &lo_d, uint32_t &lo_mm, uint32_t &n_cand, uint32_t &n_ver,
                                          unsigned long long &piled, DiagEnt *list = nullptr, uint32_t list_cap = 0, uint32_t *n_list = nullptr) {
    for (uint32_t pt = 0; pt < n_win; ++pt) {
        const uint32_t v = wvp[pt];
        if (v == 0 || v == kPileNoKey) continue;
        const uint32_t dn = A.t.dense[v];
        const uint64_t z1 = A.occ_off[dn + 1];
        for (uint64_t z = A.occ_off[dn]; z < z1; ++z) {
            const uint64_t oc = A.occ[z];
            const int strand = (int)(oc & 1ull);
            const uint32_t q = (uint32_t)(oc >> 1), ci = (uint32_t)(oc >> 33);
            const int o = strand ? 1 - a : a, same = !strand;
            const uint32_t comp = o ? 3u : 0u;
            const uint32_t p = strand ? n_win - 1 - pt : pt;                  // the window of the read in orientation o
            const uint64_t ioff = A.coff[ci];
            const int64_t clen = (int64_t)(A.coff[ci + 1] - ioff);
            // not a run start: the anchor before it on the diagonal exists, and so the candidate is not this anchor's
            if (p > 0 && q > 0 && wvp[strand ? pt + 1 : pt - 1] != 0 && (uint32_t)A.sym[ioff + q - 1] == pile_base(A.packed, s0, len, same, comp, p - 1)) continue;
            const int64_t d = (int64_t)q - (int64_t)p;
            const int64_t x0 = d > 0 ? d : 0, x1 = d + (int64_t)len < clen ? d + (int64_t)len : clen;
            const uint32_t n_ov = (uint32_t)(x1 - x0);
            uint32_t n_mm = 0, votes = 0;
            int run = 0;
            int64_t p_first = -1, p_last = -1;
            for (int64_t xb = x0; xb < x1; xb += 8) {
                if (COMMIT && (int)n_ov - 2 * (int)n_mm < best) break;        // the second pass looks for the best score only: this one is below it already
                const int64_t x = xb + sub;
                bool eq = false;
                if (x < x1) eq = (uint32_t)A.sym[ioff + (uint64_t)x] == pile_base(A.packed, s0, len, same, comp, (uint32_t)(x - d));
                const uint32_t m8 = (uint32_t)(__ballot(eq) >> (lane & 56)) & 0xFFu;
                const int nin = x1 - xb < 8 ? (int)(x1 - xb) : 8;
                n_mm += (uint32_t)nin - (uint32_t)__popc(m8);
                if (m8 == 0) { run = 0; continue; }
                for (int b = 0; b < nin; ++b) {
                    if (!((m8 >> b) & 1u)) { run = 0; continue; }
                    if (++run > k) {                                          // k + 1 equal letters end here: window xb + b - k - d of the read
                        const int64_t pw = xb + b - k - d;
                        if (wvp[same ? pw : (int64_t)n_win - 1 - pw] != 0) {
                            ++votes;
                            if (p_first < 0) p_first = pw;
                            if (LIST) p_last = pw;
                        }
                    }
                }
            }
            if (COMMIT && (int)n_ov - 2 * (int)n_mm < best) continue;
            if (!COMMIT) ++n_ver;
            if (p_first != (int64_t)p) continue;                              // an earlier anchor owns the diagonal
            if (!COMMIT) ++n_cand;
            if (LIST) {                                                       // (every lane writes the entry and reads back only what it wrote itself)
                if (*n_list < list_cap) list[*n_list] = DiagEnt{d, ci, (uint32_t)o, (uint32_t)p_first, (uint32_t)p_last};
                ++*n_list;
            }
            if ((int)votes < A.min_anchors || (int)n_ov < A.min_overlap || (uint64_t)n_mm * 1000ull > (uint64_t)A.max_permille * n_ov) continue;
            const int score = (int)n_ov - 2 * (int)n_mm;
            if (!COMMIT) {
                if (ties == 0 || score > best) { best = score; ties = 1; lo_c = ci; lo_o = o; lo_d = d; lo_mm = n_mm; }
                else if (score == best) {
                    ++ties;
                    if (ci < lo_c || (ci == lo_c && (o < lo_o || (o == lo_o && d < lo_d)))) { lo_c = ci; lo_o = o; lo_d = d; lo_mm = n_mm; }
                }
            } else if (score == best) {
                for (int64_t x = x0 + sub; x < x1; x += 8) {
                    const uint32_t b = pile_base(A.packed, s0, len, same, comp, (uint32_t)(x - d)) - 1;
                    atomicAdd(&A.counts[(ioff + (uint64_t)x) * 4 + b], 1u);
                    if (ties == 1) atomicAdd(&A.uniq[ioff + (uint64_t)x], 1u);
                }
                if (sub == 0) {
                    atomicAdd(&A.ctg[(uint64_t)ci * 3], 1ull);
                    if (ties == 1) atomicAdd(&A.ctg[(uint64_t)ci * 3 + 1], 1ull);
                    if (n_mm) atomicAdd(&A.ctg[(uint64_t)ci * 3 + 2], (unsigned long long)n_mm);
                }
                piled += n_ov;
            }
        }
    }
}

// One side of a one-gap candidate: the read letters p in [pa, pb) against x = p + d of the contig, clipped to the contig.  Adds the
// pairs, those that differ and the anchors whose k + 1 letters lie inside (runs of k + 1 equal letters whose window has an edge, as in
// pile_pass).  PILE: adds the pairs to counts / uniq instead.  All 8 lanes run the same control flow; the ballot stands outside the
// branch on the lane.
template <bool PILE>
__device__ __forceinline__ void gap_side(const PileArgs &A, int k, uint64_t s0, uint32_t len, uint32_t n_win, const uint32_t *wvp, int sub, int lane, int same,
                                         uint32_t comp, uint64_t ioff, int64_t clen, int64_t d, int64_t pa, int64_t pb, bool uniq, uint32_t &n_ov, uint32_t &n_mm,
                                         uint32_t &votes) {
    if (pa < -d) pa = -d;
    if (pb > clen - d) pb = clen - d;
    if (pb <= pa) return;
    if (PILE) {
        for (int64_t p = pa + sub; p < pb; p += 8) {
            const uint32_t b = pile_base(A.packed, s0, len, same, comp, (uint32_t)p) - 1;
            atomicAdd(&A.counts[(ioff + (uint64_t)(p + d)) * 4 + b], 1u);
            if (uniq) atomicAdd(&A.uniq[ioff + (uint64_t)(p + d)], 1u);
        }
        return;
    }
    n_ov += (uint32_t)(pb - pa);
    int run = 0;
    for (int64_t pk = pa; pk < pb; pk += 8) {
        const int64_t p = pk + sub;
        bool eq = false;
        if (p < pb) eq = (uint32_t)A.sym[ioff + (uint64_t)(p + d)] == pile_base(A.packed, s0, len, same, comp, (uint32_t)p);
        const uint32_t m8 = (uint32_t)(__ballot(eq) >> (lane & 56)) & 0xFFu;
        const int nin = pb - pk < 8 ? (int)(pb - pk) : 8;
        n_mm += (uint32_t)nin - (uint32_t)__popc(m8);
        if (m8 == 0) { run = 0; continue; }
        for (int b = 0; b < nin; ++b) {
            if (!((m8 >> b) & 1u)) { run = 0; continue; }
            if (++run > k) {
                const int64_t pw = pk + b - k;
                if (wvp[same ? pw : (int64_t)n_win - 1 - pw] != 0) ++votes;
            }
        }
    }
}

// The one-gap candidates of a read: every ordered pair (d1, d2) of the list's diagonals on one (contig, orient) within max_gap.
// COMMIT = false: judged, and the best score, its ties and the lowest of them carried on from the ungapped pass.  COMMIT = true: judged
// again, and those with the best score piled and recorded.  The breakpoint: total(b + 1) - total(b) = [c[b + d1] != s[b]] -
// [c[b + ins + d2] != s[b + ins]], so the best b is the first minimum of a running sum over the legal b, 8 of them a step: two ballots,
// popcounts below the lane, a minimum over the 8 lanes.  Every loop is bounded by the list or the read's length.
template <bool COMMIT>
__device__ __forceinline__ void gap_pass(const PileArgs &A, const GapArgs &G, int k, uint64_t r, uint64_t s0, uint32_t len, uint32_t n_win, const uint32_t *wvp, int sub,
                                         int lane, int a, const DiagEnt *list, uint32_t n_list, int &best, uint32_t &ties, uint32_t &lo_c, int &lo_o, int64_t &lo_d,
                                         int64_t &lo_d2, uint32_t &lo_b, uint32_t &lo_mm, uint32_t &n_gcand, uint32_t &n_gpass, uint32_t &n_gplaced, uint32_t &n_ins,
                                         uint32_t &n_del, unsigned long long &piled) {
    for (uint32_t ia = 0; ia < n_list; ++ia) {
        const DiagEnt e1 = list[ia];
        for (uint32_t ib = 0; ib < n_list; ++ib) {
            const DiagEnt e2 = list[ib];
            if (ib == ia || e2.ci != e1.ci || e2.o != e1.o) continue;
            const int64_t d1 = e1.d, d2 = e2.d;
            const int64_t gap = d2 > d1 ? d2 - d1 : d1 - d2;
            if (gap == 0 || gap > (int64_t)G.max_gap) continue;
            const int64_t ins = d1 > d2 ? d1 - d2 : 0;
            const int64_t lo = (int64_t)e1.first + k + 1, hi = (int64_t)e2.last - ins;     // the legal b are [lo, hi]
            if (lo > hi) continue;
            const uint32_t ci = e1.ci;
            const int o = (int)e1.o, same = o == a;
            const uint32_t comp = o ? 3u : 0u;
            const uint64_t ioff = A.coff[ci];
            const int64_t clen = (int64_t)(A.coff[ci + 1] - ioff);
            // the breakpoint.  For b in [lo, hi) both letters of the difference lie inside the read and the contig: b + d1 and
            // b + ins + d2 are at least first + k + 1 + d1 >= 0 and at most last + d2 < clen.
            int cur = 0, low = 0;
            int64_t brk = lo;
            for (int64_t bk = lo; bk < hi; bk += 8) {
                const int64_t b = bk + sub;
                bool m1 = false, m2 = false;
                if (b < hi) {
                    m1 = (uint32_t)A.sym[ioff + (uint64_t)(b + d1)] != pile_base(A.packed, s0, len, same, comp, (uint32_t)b);
                    m2 = (uint32_t)A.sym[ioff + (uint64_t)(b + ins + d2)] != pile_base(A.packed, s0, len, same, comp, (uint32_t)(b + ins));
                }
                const uint32_t w1 = (uint32_t)(__ballot(m1) >> (lane & 56)) & 0xFFu, w2 = (uint32_t)(__ballot(m2) >> (lane & 56)) & 0xFFu;
                const uint32_t upto = (2u << sub) - 1u;
                const int v = cur + (int)__popc(w1 & upto) - (int)__popc(w2 & upto);       // total(b + 1) - total(lo)
                int key = b < hi ? (((v + 65536) << 3) | sub) : 0x7FFFFFFF;
                key = min(key, __shfl_xor(key, 1, 8));
                key = min(key, __shfl_xor(key, 2, 8));
                key = min(key, __shfl_xor(key, 4, 8));
                const int mv = (key >> 3) - 65536;
                if (mv < low) { low = mv; brk = bk + (key & 7) + 1; }
                cur += (int)__popc(w1) - (int)__popc(w2);
            }
            uint32_t n_ov = 0, n_mm = 0, votes = 0;
            gap_side<false>(A, k, s0, len, n_win, wvp, sub, lane, same, comp, ioff, clen, d1, 0, brk, false, n_ov, n_mm, votes);
            gap_side<false>(A, k, s0, len, n_win, wvp, sub, lane, same, comp, ioff, clen, d2, brk + ins, (int64_t)len, false, n_ov, n_mm, votes);
            if (!COMMIT) ++n_gcand;
            if ((int)votes < A.min_anchors || (int)n_ov < A.min_overlap || (uint64_t)n_mm * 1000ull > (uint64_t)A.max_permille * n_ov) continue;
            if (!COMMIT) ++n_gpass;
            const int score = (int)n_ov - 2 * (int)n_mm - (G.gap_open + G.gap_extend * (int)gap);
            if (!COMMIT) {
                const bool first = ties == 0 || score > best, tie = !first && score == best;
                const bool lower = ci < lo_c || (ci == lo_c && (o < lo_o || (o == lo_o && (d1 < lo_d || (d1 == lo_d && d2 < lo_d2)))));
                if (first) { best = score; ties = 1; }
                if (tie) ++ties;
                if (first || (tie && lower)) { lo_c = ci; lo_o = o; lo_d = d1; lo_d2 = d2; lo_b = (uint32_t)brk; lo_mm = n_mm; }
            } else if (score == best) {
                uint32_t none = 0;
                gap_side<true>(A, k, s0, len, n_win, wvp, sub, lane, same, comp, ioff, clen, d1, 0, brk, ties == 1, none, none, none);
                gap_side<true>(A, k, s0, len, n_win, wvp, sub, lane, same, comp, ioff, clen, d2, brk + ins, (int64_t)len, ties == 1, none, none, none);
                if (sub == 0) {
                    atomicAdd(&A.ctg[(uint64_t)ci * 3], 1ull);
                    if (ties == 1) atomicAdd(&A.ctg[(uint64_t)ci * 3 + 1], 1ull);
                    if (n_mm) atomicAdd(&A.ctg[(uint64_t)ci * 3 + 2], (unsigned long long)n_mm);
                    const unsigned long long at = atomicAdd(&G.gcnt[GC_CURSOR], 1ull);
                    if (at < G.gap_cap) {
                        mgta_gap_rec rec;
                        rec.read = r; rec.contig = (int32_t)ci; rec.pos = (uint32_t)(brk + d1); rec.len = (int32_t)(d2 - d1); rec.brk = (uint32_t)brk;
                        rec.orient = o; rec.unique = ties == 1;
                        G.gaps[at] = rec;
                    }
                }
                ++n_gplaced;
                if (d1 > d2) n_ins += (uint32_t)gap; else n_del += (uint32_t)gap;
                piled += n_ov;
            }
        }
    }
}

// the scan of mgta_reads_pileup (GAPPED = false: G is not looked at) and of mgta_reads_pileup_gapped
template <bool GAPPED>
__device__ __forceinline__ void pile_scan_body(const GraphDev &g, const PileArgs &A, const GapArgs &G) {
    __shared__ uint8_t s_seq[kCovGroups][kMatchMaxWindow];
    __shared__ unsigned long long s_cnt[PC_NUM];
    if (threadIdx.x < PC_NUM) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int sub = threadIdx.x & 7, lane = lane_id();
    const int k = g.k;
    const int a = A.reversed ? 1 : 0;                                         // the stored order, complemented when reversed, is the read in orientation a
    uint8_t *seq = s_seq[threadIdx.x >> 3];
    uint32_t *wvp = A.wv + ((uint64_t)blockIdx.x * (kCovGroups) + (threadIdx.x >> 3)) * A.wv_stride;
    DiagEnt *list = GAPPED ? G.list + ((uint64_t)blockIdx.x * (kCovGroups) + (threadIdx.x >> 3)) * G.list_stride : nullptr;
    const uint32_t flip = A.reversed ? 3u : 0u;
    for (;;) {
        // every lane takes part and only the group's first counts.  (grp_next_chunk, the leader-only form of the other kernels, measured
        // 0.4 % slower here where the scan is the walk alone: profiles/walk/README.md)
        unsigned long long first = atomicAdd(&A.counters[PC_HEAD], sub == 0 ? (unsigned long long)A.chunk : 0ull);
        first = __shfl(first, 0, 8);
        if (first >= A.n_reads) break;
        const uint64_t r_end = min((unsigned long long)A.n_reads, first + A.chunk);
        for (uint64_t r = first; r < r_end; ++r) {
            const uint64_t s0 = A.start[r];
            const uint32_t len = (uint32_t)(A.start[r + 1] - s0);
            const uint32_t n_win = len > (uint32_t)k ? len - (uint32_t)k : 0;
            int64_t e = -1;                                                   // the edge of the window before, -1 = the walk has to start again
            LineR L{};
            uint32_t hits = 0, w = 0, walked = 0, searched = 0;
            for (uint32_t p = 0; p < n_win; ++p) {
                const uint64_t q = s0 + p + (uint64_t)k;                      // the window's last base
                if (p == 0 || (q & 15) == 0) w = A.packed[q >> 4];
                const int c = (int)packed_symbol(w, q, flip);
                if (e >= 0) {
                    e = cov_step(g, L, e, c, sub);
                    if (e >= 0) ++walked;
                } else {
                    // every lane writes all k + 1 symbols itself and reads back only what it wrote (the same values in every lane of the group)
                    for (int i = 0; i <= k; ++i) {
                        const uint64_t qi = s0 + p + (uint64_t)i;
                        seq[i] = (uint8_t)packed_symbol(A.packed[qi >> 4], qi, flip);
                    }
                    e = g_index_edge(g, seq);
                    ++searched;
                    if (e >= 0) L = grp_load_line(g, (uint64_t)e >> 6, sub);
                }
                uint32_t v = 0;
                if (e >= 0) {
                    v = kPileNoKey;
                    if (edge_marked(A.marks, e)) {                 // the one-bit filter in front of the table
                        const uint32_t slot = sample_table_find(A.t, e);
                        if (slot) { v = slot; ++hits; }
                    }
                }
                wvp[p] = v;                                                   // (every lane the same word: each reads back what it wrote itself)
            }
            int best = 0, lo_o = 0;
            uint32_t ties = 0, lo_c = 0, lo_mm = 0, n_cand = 0, n_ver = 0;
            int64_t lo_d = 0;
            unsigned long long piled = 0;
            int64_t lo_d2 = 0;
            uint32_t lo_b = 0, n_list = 0, n_gcand = 0, n_gpass = 0, n_gplaced = 0, n_ins = 0, n_del = 0;
            if (hits) {
                if constexpr (GAPPED) {
                    const uint32_t cap = (uint32_t)G.list_stride;
                    pile_pass<false, true>(A, k, a, s0, len, n_win, wvp, sub, lane, best, ties, lo_c, lo_o, lo_d, lo_mm, n_cand, n_ver, piled, list, cap, &n_list);
                    lo_d2 = lo_d;
                    if (n_list > cap) {                                       // (the host sized the list for the most a read can have)
                        if (sub == 0) atomicAdd(&G.gcnt[GC_OVERFLOW], 1ull);
                        n_list = cap;
                    }
                    gap_pass<false>(A, G, k, r, s0, len, n_win, wvp, sub, lane, a, list, n_list, best, ties, lo_c, lo_o, lo_d, lo_d2, lo_b, lo_mm, n_gcand, n_gpass,
                                    n_gplaced, n_ins, n_del, piled);
                    if (ties) {
                        pile_pass<true>(A, k, a, s0, len, n_win, wvp, sub, lane, best, ties, lo_c, lo_o, lo_d, lo_mm, n_cand, n_ver, piled);
                        gap_pass<true>(A, G, k, r, s0, len, n_win, wvp, sub, lane, a, list, n_list, best, ties, lo_c, lo_o, lo_d, lo_d2, lo_b, lo_mm, n_gcand, n_gpass,
                                       n_gplaced, n_ins, n_del, piled);
                    }
                } else {
                    pile_pass<false>(A, k, a, s0, len, n_win, wvp, sub, lane, best, ties, lo_c, lo_o, lo_d, lo_mm, n_cand, n_ver, piled);
                    if (ties) pile_pass<true>(A, k, a, s0, len, n_win, wvp, sub, lane, best, ties, lo_c, lo_o, lo_d, lo_mm, n_cand, n_ver, piled);
                }
            }
            if (sub == 0) {
                if constexpr (GAPPED) {
                    if (G.per_read) {
                        mgta_gap_place pr;
                        pr.score = ties ? best : 0; pr.contig = ties ? (int32_t)lo_c : -1; pr.diag = ties ? (int32_t)lo_d : 0; pr.orient = ties ? lo_o : 0;
                        pr.n_placed = ties; pr.n_mismatch = ties ? lo_mm : 0; pr.diag2 = ties ? (int32_t)lo_d2 : 0; pr.brk = lo_b;   // (set only where a gapped candidate became the lowest; no ungapped one is judged after it)
                        G.per_read[r] = pr;
                    }
                    if (n_gcand) atomicAdd(&G.gcnt[GC_CAND], (unsigned long long)n_gcand);
                    if (n_gpass) atomicAdd(&G.gcnt[GC_PASS], (unsigned long long)n_gpass);
                    if (ties && lo_d2 != lo_d) atomicAdd(&G.gcnt[GC_READS], 1ull);
                    if (n_gplaced) atomicAdd(&G.gcnt[GC_PLACED], (unsigned long long)n_gplaced);
                    if (n_ins) atomicAdd(&G.gcnt[GC_INS], (unsigned long long)n_ins);
                    if (n_del) atomicAdd(&G.gcnt[GC_DEL], (unsigned long long)n_del);
                }
                if (A.per_read) {
                    mgta_read_place pr;
                    pr.score = ties ? best : 0; pr.contig = ties ? (int32_t)lo_c : -1; pr.diag = ties ? (int32_t)lo_d : 0; pr.orient = ties ? lo_o : 0;
                    pr.n_placed = ties; pr.n_mismatch = ties ? lo_mm : 0;
                    A.per_read[r] = pr;
                }
                if (walked) atomicAdd(&s_cnt[PC_WALKED], (unsigned long long)walked);
                if (searched) atomicAdd(&s_cnt[PC_SEARCHED], (unsigned long long)searched);
                if (n_win) atomicAdd(&s_cnt[PC_WINDOWS], (unsigned long long)n_win);
                if (hits) atomicAdd(&s_cnt[PC_HITS], (unsigned long long)hits);
                if (n_cand) { atomicAdd(&s_cnt[PC_READS_CAND], 1ull); atomicAdd(&s_cnt[PC_CAND], (unsigned long long)n_cand); }
                if (n_ver) atomicAdd(&s_cnt[PC_VERIFIED], (unsigned long long)n_ver);
                if (ties) { atomicAdd(&s_cnt[PC_PLACED], 1ull); atomicAdd(&s_cnt[PC_PLACEMENTS], (unsigned long long)ties); atomicAdd(&s_cnt[PC_PILED], piled); }
                if (ties > 1) atomicAdd(&s_cnt[PC_MULTI], 1ull);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x > 0 && threadIdx.x < PC_NUM && s_cnt[threadIdx.x]) atomicAdd(&A.counters[threadIdx.x], s_cnt[threadIdx.x]);
}

__global__ __launch_bounds__(kCovThreads) void pile_scan_kernel(GraphDev g, PileArgs A) { pile_scan_body<false>(g, A, GapArgs{}); }

__global__ __launch_bounds__(kCovThreads) void pile_gapped_scan_kernel(GraphDev g, PileArgs A, GapArgs G) { pile_scan_body<true>(g, A, G); }

// the most occurrences of one key (atomicMax into *out, zeroed by the caller): it bounds the diagonals a read can lie on
__global__ __launch_bounds__(256) void pile_occ_max_kernel(const uint32_t *cnt, uint64_t n, unsigned long long *out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    unsigned long long mx = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) mx = max(mx, (unsigned long long)cnt[i]);
    if (mx) atomicMax(out, mx);
}

// one wave per contig over its counts
__global__ __launch_bounds__(256) void pile_records_kernel(const uint64_t *coff, uint32_t n, const uint32_t *counts, const unsigned long long *ctg, mgta_contig_pileup *out) {
    const int lane = lane_id();
    const uint32_t i = blockIdx.x * 4 + (uint32_t)wave_id();
    if (i >= n) return;                                                       // (whole waves leave)
    const uint64_t b = coff[i];
    const uint32_t len = (uint32_t)(coff[i + 1] - b);
    uint64_t sum = 0;
    uint32_t mn = 0xFFFFFFFFu, mx = 0, nc = 0;
    for (uint32_t x = lane; x < len; x += 64) {
        const uint4 c = reinterpret_cast<const uint4 *>(counts)[b + x];
        const uint32_t depth = c.x + c.y + c.z + c.w;
        sum += depth; mn = min(mn, depth); mx = max(mx, depth); nc += depth != 0;
    }
    mgta_contig_pileup res;
    res.len = len; res.n_covered = wave_sum(nc); res.min_depth = len ? wave_min(mn) : 0u; res.max_depth = wave_max(mx);
    res.n_placed = ctg[(uint64_t)i * 3]; res.n_unique = ctg[(uint64_t)i * 3 + 1]; res.depth_sum = wave_sum64(sum); res.mismatch_sum = ctg[(uint64_t)i * 3 + 2];
    if (lane == 0) out[i] = res;
}

// what mgta_reads_pileup_gapped has beyond mgta_reads_pileup, NULL for the latter
struct GapCall {
    int max_gap, gap_open, gap_extend;
    mgta_gap_rec *gaps;
    uint64_t gap_cap;
    mgta_gapped_stats *stats;
};

int pileup_run(const char *name, mgta_sdbg *g, const mgta_reads *reads, int reads_reversed, uint64_t n_short_reads, const char *seqs, const uint64_t *offsets, int64_t n,
               mgta_pileup_params par, uint32_t *counts, uint32_t *uniq, mgta_contig_pileup *per_contig, void *per_read, mgta_pileup_stats *stats, const GapCall *gc);

}  // namespace
}  // namespace mgta

using namespace mgta;

extern "C" {

int mgta_ctx_set_pileup_chunk(mgta_ctx *ctx, uint32_t reads) {
    if (!ctx) { set_error("mgta_ctx_set_pileup_chunk: ctx must not be NULL"); return MGTA_EINVAL; }
    ctx->pileup_chunk = reads;
    return MGTA_OK;
}

int mgta_reads_pileup(mgta_sdbg *g, const mgta_reads *reads, int reads_reversed, uint64_t n_short_reads, const char *seqs, const uint64_t *offsets, int64_t n,
                      const mgta_pileup_params *params, uint32_t *counts, uint32_t *uniq, mgta_contig_pileup *per_contig, mgta_read_place *per_read,
                      mgta_pileup_stats *stats) {
    mgta_pileup_params par{0, 0, 0};
    if (params) par = *params;
    return pileup_run("mgta_reads_pileup", g, reads, reads_reversed, n_short_reads, seqs, offsets, n, par, counts, uniq, per_contig, per_read, stats, nullptr);
}

int mgta_reads_pileup_gapped(mgta_sdbg *g, const mgta_reads *reads, int reads_reversed, uint64_t n_short_reads, const char *seqs, const uint64_t *offsets, int64_t n,
                             const mgta_gapped_params *params, uint32_t *counts, uint32_t *uniq, mgta_contig_pileup *per_contig, mgta_gap_place *per_read,
                             mgta_gap_rec *gaps, uint64_t gap_cap, mgta_gapped_stats *stats) {
    mgta_gapped_params p{0, 0, 0, 0, 0, 0};
    if (params) p = *params;
    GapCall gc{p.max_gap, p.gap_open, p.gap_extend, gaps, gap_cap, stats};
    return pileup_run("mgta_reads_pileup_gapped", g, reads, reads_reversed, n_short_reads, seqs, offsets, n, mgta_pileup_params{p.min_anchors, p.min_overlap, p.max_mismatch_permille},
                      counts, uniq, per_contig, per_read, nullptr, &gc);
}

}  // extern "C"

namespace mgta {
namespace {

int pileup_run(const char *name, mgta_sdbg *g, const mgta_reads *reads, int reads_reversed, uint64_t n_short_reads, const char *seqs, const uint64_t *offsets, int64_t n,
               mgta_pileup_params par, uint32_t *counts, uint32_t *uniq, mgta_contig_pileup *per_contig, void *per_read, mgta_pileup_stats *stats, const GapCall *gc) {
    if (!g || !reads) { set_error("%s: the graph and the reads must not be NULL", name); return MGTA_EINVAL; }
    if (g->ctx != reads->ctx) { set_error("%s: the graph and the reads belong to different contexts", name); return MGTA_EINVAL; }
    if (n_short_reads > reads->n_reads) {
        set_error("%s: n_short_reads = %llu, the library holds %llu reads", name, (unsigned long long)n_short_reads, (unsigned long long)reads->n_reads);
        return MGTA_EINVAL;
    }
    if (n < 0 || (n > 0 && !offsets)) { set_error("%s: bad contig count or offsets", name); return MGTA_EINVAL; }
    if (n > 0x7FFFFFFFll) { set_error("%s: %lld contigs (n < 2^31 is supported)", name, (long long)n); return MGTA_EINVAL; }
    if (g->dev.k + 1 > kMatchMaxWindow) { set_error("%s: k = %d (k + 1 <= %d is supported)", name, g->dev.k, kMatchMaxWindow); return MGTA_EINVAL; }
    const uint64_t k = (uint64_t)g->dev.k;
    if (par.min_anchors < 0 || par.min_overlap < 0 || par.max_mismatch_permille < 0 || par.max_mismatch_permille > 1000) {
        set_error("%s: min_anchors = %d, min_overlap = %d, max_mismatch_permille = %d (none negative, permille <= 1000)", name, par.min_anchors, par.min_overlap,
                  par.max_mismatch_permille);
        return MGTA_EINVAL;
    }
    if (par.min_anchors == 0) par.min_anchors = 1;
    if (par.min_overlap == 0) par.min_overlap = (int32_t)k + 1;
    if (par.max_mismatch_permille == 0) par.max_mismatch_permille = 50;
    GapCall gp{0, 0, 0, nullptr, 0, nullptr};
    if (gc) {
        gp = *gc;
        if (gp.max_gap == 0) gp.max_gap = 32;
        if (gp.gap_open == 0) gp.gap_open = 4;
        if (gp.gap_extend == 0) gp.gap_extend = 1;
        if (gp.max_gap < 0 || gp.max_gap > 255) { set_error("%s: max_gap = %d (0 <= max_gap <= 255 is supported)", name, gc->max_gap); return MGTA_EINVAL; }
        if (gp.gap_open < 0 || gp.gap_open > 255) { set_error("%s: gap_open = %d (0 <= gap_open <= 255 is supported)", name, gc->gap_open); return MGTA_EINVAL; }
        if (gp.gap_extend < 0 || gp.gap_extend > gp.gap_open) {
            set_error("%s: gap_extend = %d with gap_open = %d (0 <= gap_extend <= gap_open is supported)", name, gp.gap_extend, gp.gap_open);
            return MGTA_EINVAL;
        }
        if (gp.gap_cap > 0 && !gp.gaps) { set_error("%s: gaps must not be NULL with gap_cap = %llu", name, (unsigned long long)gp.gap_cap); return MGTA_EINVAL; }
    }
    uint64_t total_win = 0;
    if (!check_contigs(name, seqs, offsets, n, k, 0, 0, &total_win, nullptr)) return MGTA_EINVAL;   // (no cap per contig: offsets[n] is checked below)
    if (n > 0 && offsets[0] != 0) { set_error("%s: offsets[0] = %llu (the counts are indexed by the offsets: 0 is expected)", name, (unsigned long long)offsets[0]); return MGTA_EINVAL; }
    const uint64_t n_sym = n > 0 ? offsets[n] : 0;
    if (n_sym > 0xFFFFFFFFull) { set_error("%s: %llu letters in the call (offsets[n] < 2^32 is supported)", name, (unsigned long long)n_sym); return MGTA_EINVAL; }
    if (n_sym > 0 && !counts) { set_error("%s: counts must not be NULL", name); return MGTA_EINVAL; }
    // the table holds the edges of both strands: at most half full; a slot number is 32 bits and its highest value is taken
    const uint64_t most_keys = std::min<uint64_t>(2 * total_win, (uint64_t)std::max<int64_t>(g->dev.size, 0));
    if (2 * most_keys + 2 > (1ull << 31)) {
        set_error("%s: %llu keys need a table of more than 2^31 slots", name, (unsigned long long)most_keys);
        return MGTA_ENOMEM;
    }
    auto zero_outputs = [&]() {
        if (stats) memset(stats, 0, sizeof(*stats));
        if (gc && gp.stats) memset(gp.stats, 0, sizeof(*gp.stats));
        if (n_sym) memset(counts, 0, n_sym * 16);
        if (uniq && n_sym) memset(uniq, 0, n_sym * 4);
        if (per_contig)
            for (int64_t i = 0; i < n; ++i) { memset(&per_contig[i], 0, sizeof(per_contig[i])); per_contig[i].len = (uint32_t)(offsets[i + 1] - offsets[i]); }
        if (per_read && !gc)
            for (uint64_t r = 0; r < n_short_reads; ++r) static_cast<mgta_read_place *>(per_read)[r] = mgta_read_place{0, -1, 0, 0, 0, 0};
        if (per_read && gc)
            for (uint64_t r = 0; r < n_short_reads; ++r) static_cast<mgta_gap_place *>(per_read)[r] = mgta_gap_place{0, -1, 0, 0, 0, 0, 0, 0};
    };
    if (n == 0 || n_short_reads == 0) { zero_outputs(); return MGTA_OK; }
    return guarded(name, [&]() {
        mgta_ctx *ctx = g->ctx;
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        uint64_t live = 0, peak = 0;                                          // the buffers of this call
        DevBuf d_cnt;
        d_cnt.alloc(256, &live, &peak);
        MGTA_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 256, st));
        unsigned long long *cnt_mark = d_cnt.as<unsigned long long>(), *cnt_scan = cnt_mark + 8, *cnt_len = cnt_mark + 24;
        hipLaunchKernelGGL(pile_maxlen_kernel, dim3((unsigned)std::min<uint64_t>((n_short_reads + 255) / 256, (uint64_t)ctx->num_cus * 8)), dim3(256), 0, st, reads->d_start,
                           n_short_reads, cnt_len);
        MGTA_HIP_CHECK(hipGetLastError());
        unsigned long long max_len = 0;
        MGTA_HIP_CHECK(hipMemcpyAsync(&max_len, cnt_len, 8, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        if (max_len > kPileMaxRead) {
            set_error("%s: a read of %llu bases (reads of at most %u bases are supported)", name, max_len, kPileMaxRead);
            return (int)MGTA_EINVAL;
        }
        if (!gc) zero_outputs();                                              // (the gapped call writes nothing before it knows that its records fit)
        Timer t_keys(st), t_index(st), t_scan(st), t_rec(st);
        uint32_t *d_marks = marks_reset(g, st);
        DevBuf d_sym, d_jobs, d_own, d_rc, d_coff, d_woff, d_occ_cnt, d_occ_off, d_occ, d_tmp, d_counts, d_uniq, d_ctg, d_wv, d_pr, d_out, d_gcnt, d_list, d_gaps;
        SampleTableMem tm;
        sample_table_alloc(ctx, st, most_keys, &live, &peak, tm);
        const SampleTable &tab = tm.t;
        d_own.alloc(total_win * 4 + 16, &live, &peak);
        d_rc.alloc(total_win * 4 + 16, &live, &peak);
        // ---- phase 1: the keys.  All contigs are one batch: the best-hit rule needs them all
        std::vector<CovJob> jobs;
        uint64_t n_win = 0;
        cut_batch(offsets, n, k, 0, ~0ull, true, jobs, &n_win);
        const std::vector<uint64_t> woff = window_offsets(offsets, n, k);
        const uint32_t nj = (uint32_t)jobs.size();
        const uint64_t longest = contig_windows(jobs[0].len, k);
        d_sym.alloc(2 * n_sym + 16, &live, &peak);
        d_jobs.alloc((size_t)nj * sizeof(CovJob), &live, &peak);
        d_coff.alloc(((size_t)n + 1) * 8, &live, &peak);
        d_woff.alloc(((size_t)n + 1) * 8, &live, &peak);
        int64_t *d_ids = reinterpret_cast<int64_t *>(window_scratch(ctx, 2 * total_win * 8 + 64));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)nj * sizeof(CovJob), hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_coff.p, offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_woff.p, woff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
        stage_symbols(ctx, st, d_sym, seqs, n_sym, true);
        const QueueLaunch q_walk = queue_launch(ctx, queue_per_cu(share_walk_kernel), nj, 64, 4);
        t_keys.start();
        if (g->dev.size > 0)
            hipLaunchKernelGGL(share_walk_kernel, dim3(q_walk.blocks), dim3(kCovThreads), 0, st, g->dev, d_sym.as<uint8_t>(), d_jobs.as<CovJob>(), nj, q_walk.chunk, d_ids,
                               cnt_mark);
        else
            MGTA_HIP_CHECK(hipMemsetAsync(d_ids, 0xFF, 2 * total_win * 8 + 64, st));   // no edge anywhere
        MGTA_HIP_CHECK(hipGetLastError());
        if (longest) {
            const unsigned gy = (unsigned)std::min<uint64_t>((longest + 255) / 256, 1024);
            hipLaunchKernelGGL(sample_count_kernel, dim3((nj + 63) / 64, gy), dim3(256), 0, st, tab, d_jobs.as<CovJob>(), nj, (int)k, d_ids, total_win, (uint64_t)0,
                               d_own.as<uint32_t>(), d_rc.as<uint32_t>(), d_marks, cnt_mark);
        }
        hipLaunchKernelGGL(sample_dense_kernel, dim3((unsigned)std::min<uint64_t>(tab.n_slots / 256, (uint64_t)ctx->num_cus * 16)), dim3(256), 0, st, tab, cnt_mark);
        MGTA_HIP_CHECK(hipGetLastError());
        t_keys.end();
        unsigned long long cnt[32] = {0};
        MGTA_HIP_CHECK(hipMemcpyAsync(cnt, d_cnt.p, 64, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        if (cnt[5]) { set_error("%s: the key table of %llu slots ran full", name, (unsigned long long)tab.n_slots); return (int)MGTA_EHIP; }
        const uint64_t n_keys = cnt[3];
        // ---- phase 2: the occurrence index
        d_occ_cnt.alloc((n_keys + 2) * 4 * 2, &live, &peak);                  // the counts, and behind them the cursors
        d_occ_off.alloc((n_keys + 2) * 8, &live, &peak);
        d_tmp.alloc((scan_tmp_elems(n_keys + 2) + 1) * 8, &live, &peak);
        MGTA_HIP_CHECK(hipMemsetAsync(d_occ_cnt.p, 0, (n_keys + 2) * 4 * 2, st));
        uint32_t *occ_cnt = d_occ_cnt.as<uint32_t>(), *occ_cur = occ_cnt + (n_keys + 2);
        uint64_t *d_total = d_tmp.as<uint64_t>() + scan_tmp_elems(n_keys + 2);
        t_index.start();
        if (total_win)
            hipLaunchKernelGGL(pile_occ_count_kernel, dim3((unsigned)std::min<uint64_t>((total_win + 255) / 256, (uint64_t)ctx->num_cus * 16)), dim3(256), 0, st,
                               d_own.as<uint32_t>(), d_rc.as<uint32_t>(), tab.dense, total_win, occ_cnt);
        exclusive_scan_u32(st, occ_cnt, n_keys + 2, d_occ_off.as<uint64_t>(), d_tmp.as<uint64_t>(), d_total);
        MGTA_HIP_CHECK(hipGetLastError());
        uint64_t n_occ = 0;
        MGTA_HIP_CHECK(hipMemcpyAsync(&n_occ, d_total, 8, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        d_occ.alloc(n_occ * 8 + 16, &live, &peak);
        if (total_win)
            hipLaunchKernelGGL(pile_occ_fill_kernel, dim3((unsigned)(((uint64_t)n + 3) / 4)), dim3(256), 0, st, d_woff.as<uint64_t>(), (uint32_t)n, d_own.as<uint32_t>(),
                               d_rc.as<uint32_t>(), tab.dense, d_occ_off.as<uint64_t>(), occ_cur, d_occ.as<uint64_t>());
        MGTA_HIP_CHECK(hipGetLastError());
        t_index.end();
        // ---- phase 3: the read scan
        d_counts.alloc(n_sym * 16 + 16, &live, &peak);
        d_uniq.alloc(n_sym * 4 + 16, &live, &peak);
        d_ctg.alloc((size_t)n * 24, &live, &peak);
        d_out.alloc((size_t)n * sizeof(mgta_contig_pileup), &live, &peak);
        const size_t pr_bytes = gc ? sizeof(mgta_gap_place) : sizeof(mgta_read_place);
        if (per_read) d_pr.alloc(n_short_reads * pr_bytes, &live, &peak);
        MGTA_HIP_CHECK(hipMemsetAsync(d_counts.p, 0, n_sym * 16 + 16, st));
        MGTA_HIP_CHECK(hipMemsetAsync(d_uniq.p, 0, n_sym * 4 + 16, st));
        MGTA_HIP_CHECK(hipMemsetAsync(d_ctg.p, 0, (size_t)n * 24, st));
        const uint64_t max_win = max_len > k ? max_len - k : 0;
        const uint64_t wv_stride = std::max<uint64_t>(16, (max_win + 15) & ~15ull);
        QueueLaunch q_scan = queue_launch(ctx, gc ? queue_per_cu(pile_gapped_scan_kernel) : queue_per_cu(pile_scan_kernel), n_short_reads, 256, 16, ctx->pileup_chunk);
        q_scan.blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(q_scan.blocks, kPileScratchBytes / (wv_stride * 4 * kCovGroups)));   // the scratch rows of the groups in flight
        uint64_t list_entries = 0;
        if (gc) {
            // the diagonal list of a group: a read has at most one candidate per anchor, a window at most the occurrences of one key
            unsigned long long max_occ = 0;
            hipLaunchKernelGGL(pile_occ_max_kernel, dim3((unsigned)std::min<uint64_t>((n_keys + 2 + 255) / 256, (uint64_t)ctx->num_cus * 8)), dim3(256), 0, st, occ_cnt,
                               n_keys + 2, cnt_len + 1);
            MGTA_HIP_CHECK(hipGetLastError());
            MGTA_HIP_CHECK(hipMemcpyAsync(&max_occ, cnt_len + 1, 8, hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
            list_entries = std::max<uint64_t>(1, max_win * max_occ);
            if (list_entries > 0xFFFFFFFFull) { set_error("%s: a list of %llu diagonals per read does not fit", name, (unsigned long long)list_entries); return (int)MGTA_ENOMEM; }
            q_scan.blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(q_scan.blocks, kPileScratchBytes / (list_entries * sizeof(DiagEnt) * kCovGroups)));
            d_list.alloc((uint64_t)q_scan.blocks * kCovGroups * list_entries * sizeof(DiagEnt), &live, &peak);
            d_gcnt.alloc(GC_NUM * 8, &live, &peak);
            MGTA_HIP_CHECK(hipMemsetAsync(d_gcnt.p, 0, GC_NUM * 8, st));
            if (gp.gap_cap) d_gaps.alloc(gp.gap_cap * sizeof(mgta_gap_rec), &live, &peak);
        }
        d_wv.alloc((uint64_t)q_scan.blocks * kCovGroups * wv_stride * 4, &live, &peak);
        t_scan.start();
        if (g->dev.size > 0 && gc) {
            PileArgs A;
            A.packed = reads->d_packed; A.start = reads->d_start; A.n_reads = n_short_reads; A.reversed = reads_reversed ? 1 : 0; A.chunk = q_scan.chunk;
            A.marks = d_marks; A.t = tab; A.sym = d_sym.as<uint8_t>(); A.coff = d_coff.as<uint64_t>(); A.occ_off = d_occ_off.as<uint64_t>();
            A.occ = d_occ.as<uint64_t>(); A.counts = d_counts.as<uint32_t>(); A.uniq = d_uniq.as<uint32_t>(); A.ctg = d_ctg.as<unsigned long long>();
            A.per_read = nullptr; A.wv = d_wv.as<uint32_t>(); A.wv_stride = wv_stride;
            A.min_anchors = par.min_anchors; A.min_overlap = par.min_overlap; A.max_permille = par.max_mismatch_permille; A.counters = cnt_scan;
            GapArgs G;
            G.list = d_list.as<DiagEnt>(); G.list_stride = list_entries; G.per_read = per_read ? d_pr.as<mgta_gap_place>() : nullptr;
            G.gaps = gp.gap_cap ? d_gaps.as<mgta_gap_rec>() : nullptr; G.gap_cap = gp.gap_cap; G.max_gap = gp.max_gap; G.gap_open = gp.gap_open;
            G.gap_extend = gp.gap_extend; G.gcnt = d_gcnt.as<unsigned long long>();
            hipLaunchKernelGGL(pile_gapped_scan_kernel, dim3(q_scan.blocks), dim3(kCovThreads), 0, st, g->dev, A, G);
        } else if (g->dev.size > 0) {
            PileArgs A;
            A.packed = reads->d_packed; A.start = reads->d_start; A.n_reads = n_short_reads; A.reversed = reads_reversed ? 1 : 0; A.chunk = q_scan.chunk;
            A.marks = d_marks; A.t = tab; A.sym = d_sym.as<uint8_t>(); A.coff = d_coff.as<uint64_t>(); A.occ_off = d_occ_off.as<uint64_t>();
            A.occ = d_occ.as<uint64_t>(); A.counts = d_counts.as<uint32_t>(); A.uniq = d_uniq.as<uint32_t>(); A.ctg = d_ctg.as<unsigned long long>();
            A.per_read = per_read ? d_pr.as<mgta_read_place>() : nullptr; A.wv = d_wv.as<uint32_t>(); A.wv_stride = wv_stride;
            A.min_anchors = par.min_anchors; A.min_overlap = par.min_overlap; A.max_permille = par.max_mismatch_permille; A.counters = cnt_scan;
            hipLaunchKernelGGL(pile_scan_kernel, dim3(q_scan.blocks), dim3(kCovThreads), 0, st, g->dev, A);
        }
        MGTA_HIP_CHECK(hipGetLastError());
        t_scan.end();
        // ---- phase 4: the per-contig records
        t_rec.start();
        hipLaunchKernelGGL(pile_records_kernel, dim3((unsigned)(((uint64_t)n + 3) / 4)), dim3(256), 0, st, d_coff.as<uint64_t>(), (uint32_t)n, d_counts.as<uint32_t>(),
                           d_ctg.as<unsigned long long>(), d_out.as<mgta_contig_pileup>());
        MGTA_HIP_CHECK(hipGetLastError());
        t_rec.end();
        unsigned long long gcnt[GC_NUM] = {0};
        std::vector<mgta_gap_rec> recs;
        if (gc) {
            MGTA_HIP_CHECK(hipMemcpyAsync(gcnt, d_gcnt.p, GC_NUM * 8, hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
            if (gcnt[GC_OVERFLOW]) { set_error("%s: the diagonal list of %llu entries ran full", name, (unsigned long long)list_entries); return (int)MGTA_EHIP; }
            if (gcnt[GC_CURSOR] > gp.gap_cap) {
                set_error("%s: %llu gap records, gap_cap = %llu (call again with gap_cap >= %llu)", name, gcnt[GC_CURSOR], (unsigned long long)gp.gap_cap, gcnt[GC_CURSOR]);
                if (gp.stats) gp.stats->n_gap_placements = (int64_t)gcnt[GC_CURSOR];
                return (int)MGTA_EINVAL;
            }
            recs.resize(gcnt[GC_CURSOR]);
            if (!recs.empty()) MGTA_HIP_CHECK(hipMemcpyAsync(recs.data(), d_gaps.p, recs.size() * sizeof(mgta_gap_rec), hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
            zero_outputs();
            std::sort(recs.begin(), recs.end(), [](const mgta_gap_rec &x, const mgta_gap_rec &y) {
                if (x.contig != y.contig) return x.contig < y.contig;
                if (x.pos != y.pos) return x.pos < y.pos;
                if (x.len != y.len) return x.len < y.len;
                if (x.read != y.read) return x.read < y.read;
                if (x.orient != y.orient) return x.orient < y.orient;
                return (int64_t)x.pos - (int64_t)x.brk < (int64_t)y.pos - (int64_t)y.brk;
            });
            if (!recs.empty()) memcpy(gp.gaps, recs.data(), recs.size() * sizeof(mgta_gap_rec));
        }
        if (n_sym) MGTA_HIP_CHECK(hipMemcpyAsync(counts, d_counts.p, n_sym * 16, hipMemcpyDeviceToHost, st));
        if (uniq && n_sym) MGTA_HIP_CHECK(hipMemcpyAsync(uniq, d_uniq.p, n_sym * 4, hipMemcpyDeviceToHost, st));
        if (per_contig) MGTA_HIP_CHECK(hipMemcpyAsync(per_contig, d_out.p, (size_t)n * sizeof(mgta_contig_pileup), hipMemcpyDeviceToHost, st));
        if (per_read && g->dev.size > 0) MGTA_HIP_CHECK(hipMemcpyAsync(per_read, d_pr.p, n_short_reads * pr_bytes, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(cnt, d_cnt.p, 192, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        if (ctx->live_bytes + peak > ctx->peak_bytes) ctx->peak_bytes = ctx->live_bytes + peak;
        mgta_pileup_stats own;
        if (gc && gp.stats) stats = &own;
        if (stats) {
            const unsigned long long *c = cnt + 8;
            stats->n_contigs = n; stats->n_contig_letters = (int64_t)n_sym; stats->n_contig_windows = (int64_t)total_win; stats->n_keys = (int64_t)n_keys;
            stats->n_occurrences = (int64_t)n_occ; stats->n_reads = (int64_t)n_short_reads; stats->n_read_windows = (int64_t)c[PC_WINDOWS];
            stats->n_hit_windows = (int64_t)c[PC_HITS]; stats->n_read_walked = (int64_t)c[PC_WALKED]; stats->n_read_index_searches = (int64_t)c[PC_SEARCHED];
            stats->n_reads_with_candidate = (int64_t)c[PC_READS_CAND]; stats->n_candidates = (int64_t)c[PC_CAND]; stats->n_verified = (int64_t)c[PC_VERIFIED];
            stats->n_reads_placed = (int64_t)c[PC_PLACED]; stats->n_reads_multi = (int64_t)c[PC_MULTI]; stats->n_placements = (int64_t)c[PC_PLACEMENTS];
            stats->n_bases_piled = (int64_t)c[PC_PILED]; stats->groups_per_cu = q_scan.groups_per_cu(); stats->peak_bytes = peak;
            stats->ms_keys = t_keys.ms(); stats->ms_index = t_index.ms(); stats->ms_scan = t_scan.ms(); stats->ms_records = t_rec.ms();
            stats->ms_total = stats->ms_keys + stats->ms_index + stats->ms_scan + stats->ms_records;
        }
        if (gc && gp.stats) {
            mgta_gapped_stats *gs = gp.stats;
            memcpy(gs, &own, sizeof(own));                                    // (the first fields are mgta_pileup_stats)
            gs->n_gap_candidates = (int64_t)gcnt[GC_CAND]; gs->n_gap_passing = (int64_t)gcnt[GC_PASS]; gs->n_reads_gapped = (int64_t)gcnt[GC_READS];
            gs->n_gap_placements = (int64_t)gcnt[GC_PLACED]; gs->n_inserted = (int64_t)gcnt[GC_INS]; gs->n_deleted = (int64_t)gcnt[GC_DEL];
            gs->diag_list_entries = (int64_t)list_entries;
        }
        return (int)MGTA_OK;
    });
}

}  // namespace
}  // namespace mgta
