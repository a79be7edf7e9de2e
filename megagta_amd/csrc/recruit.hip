// recruit.hip — which reads of the resident library the gene's profile HMM places in one of six frames (mgta_reads_recruit).  The
// rule is this library's own (include/megagta_hip.h): per frame the longest run of residues without a stop, scored exactly as
// mgta_seqs_align scores that run as a protein (fp64, every + one IEEE add, the maximum first and then + e, first candidate wins a
// tie), the best frame per read, a threshold in nats.
//
// One kernel.  A wave takes `chunk` reads from one atomic head; lane r of the wave keeps the record of the chunk's read r.  The
// wave translates frame after frame straight from the 2-bit words (pile_base, walk.hpp; the 64 codon letters in LDS): a first pass
// finds the stops by ballot and the longest run between them with scalar work, a second writes the run's residues into the wave's
// rows in LDS, bit 7 on the run's first residue and bit 5 (the lower-case bit, free in an upper-case letter) on its last.  When the
// rows or the stretch slots are full, and at the end of the chunk, the rows are swept.
//
// The sweep is align.hip's strip sweep with three differences.  (1) All T residues in the rows go through a strip of 64 columns back
// to back, T + w - 1 steps instead of L + w - 1 per stretch: a first residue resets its cell to row 1 of the recurrence (B = 0, no
// insert, no delete), and nothing else crosses from one stretch to the next, because X and I are the only values that move down a
// row and both are replaced there.  (2) No cell is stored.  Every X, Y and I carries the column of the first match state of the
// candidate that won it, chosen by the same comparisons, so the column that arrives with the best cell of a last row is the one the
// traceback of mgta_seqs_align would reach.  (3) A last residue offers its match value to its stretch's slot in LDS; columns are
// offered in ascending order (strips ascend, and within a strip lane l is a step behind lane l - 1), so a strict > keeps the lowest.
// The rows at a strip's edge are 24 bytes per residue: X, Y and their two columns.
//
// Local mode (MGTA_RECRUIT_LOCAL, the kernel's second template parameter; the global instantiation is the code above, unchanged).
// The first pass gives every run of at least min_aa residues between two stops its rows and its slot, not only the longest, so the
// rows are swept whenever 64 slots are full.  In the sweep the match state of every row takes B = 0 as its first candidate, the delete
// state is fed by the match value without that candidate (one more add), and what is carried with X, Y and I is the entry column in
// the low 20 bits and the entry row (of the wave's rows) in the 12 above them: still one register per value, six cross-lane moves a
// step and 24 bytes per edge row.  A lane keeps the best match value of its column over the rows of the stretch it is in (strict >:
// the lowest row) and offers it to the stretch's slot when it passes the stretch's last residue; a lane passes that residue a step
// behind its left neighbour and strips ascend, so the slot's strict > still keeps the lowest column.  The slot holds the end row
// above the end column in the same packing, and the stretch's first row beside the read and the frame.
#include <algorithm>
#include <cmath>
#include <vector>

#include "seq_dp.hpp"
#include "walk.hpp"

namespace mgta {
namespace {

constexpr uint32_t kRecruitMaxBases = 3 * 4096 + 2;    // of one read: 4096 residues in every frame
constexpr uint32_t kRecruitRows = 256;                 // residues a wave sweeps at once, where no read needs more
#ifdef MGTA_RECRUIT_ONE_AT_A_TIME                      // the experiment of profiles/recruit/README.md: a sweep per stretch, align.hip's shape
constexpr uint32_t kRecruitSlots = 1;
#else
constexpr uint32_t kRecruitSlots = 64;                 // stretches a wave sweeps at once
#endif
constexpr uint32_t kRecruitMaxChunk = 64;              // reads per queue grab: one lane each
constexpr size_t kRecruitLdsBudget = 80 * 1024;        // of a workgroup while the longest read allows it: two fit a CU
constexpr size_t kRecruitLdsMax = 160 * 1024;          // of a workgroup at all
constexpr uint32_t kFirstResidue = 0x80u, kLastResidue = 0x20u;
constexpr int kLocalColBits = 20;                      // local mode: a column below, a row of the wave (< 4096) above, in one register
constexpr int kLocalColMask = (1 << kLocalColBits) - 1;

__constant__ char kRecruitCodon[65] = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF";   // codon = 16 b0 + 4 b1 + b2, A C G T = 0 .. 3

enum { RC_HEAD, RC_FRAMES, RC_RESIDUES, RC_UNALIGNED, RC_UNSCORED, RC_RECRUITED, RC_FRAME0, RC_NUM = RC_FRAME0 + 6 };

struct RecruitArgs {
    const uint32_t *packed;
    const uint64_t *start;
    uint64_t n_reads;
    int reversed;
    uint32_t chunk;
    int M, A;
    const double *tab;
    const int8_t *alpha;
    uint32_t rows;                   // residues of a wave's rows (a multiple of 8, >= the longest stretch)
    uint32_t min_aa;
    double min_score;
    unsigned long long *hit_bits;
    mgta_recruit_rec *recs;          // or NULL
    unsigned long long *col_diff;    // [M + 1]: + 1 at model_from - 1, - 1 at model_to; or NULL
    unsigned long long *counters;    // [RC_NUM]
};

struct StretchSlot {                 // 24 bytes
    double score;
    int32_t jend, entry;             // local mode: | end row << 20, | entry row << 20
    uint32_t read_frame;             // read of the chunk | frame << 8; local mode: | the stretch's first row << 12
    uint32_t aa;                     // aa_from | aa_len << 16, of the stretch
};

// what a wave has in LDS beside the profile's
struct RecruitLds {
    double *bxy;                     // [2 * rows] X and Y of the strip's last lane, per row
    int32_t *bent;                   // [2 * rows] their columns
    volatile StretchSlot *slot;      // [kRecruitSlots]
    uint8_t *res;                    // [rows]
    const char *codon;               // [64], the workgroup's
};

__host__ __device__ constexpr size_t recruit_wave_bytes(uint32_t rows) { return (size_t)kRecruitSlots * sizeof(StretchSlot) + rows; }

// the residue of codon c of a frame: the bases off + 3c .. off + 3c + 2 of the read in orientation o
__device__ __forceinline__ char frame_residue(const RecruitArgs &a, const char *codon, uint64_t s0, uint32_t len, int same, uint32_t comp, uint32_t off, uint32_t c) {
    const uint32_t p = off + 3u * c;
    const uint32_t b0 = pile_base(a.packed, s0, len, same, comp, p) - 1, b1 = pile_base(a.packed, s0, len, same, comp, p + 1) - 1,
                   b2 = pile_base(a.packed, s0, len, same, comp, p + 2) - 1;
    return codon[16u * b0 + 4u * b1 + b2];
}

// All T residues of the wave's rows over the M nodes: the slots' score, end column and entry column (LOCAL: the best cell of any row,
// end and entry as column | row << 20).
template <bool LOCAL>
__device__ __forceinline__ void recruit_sweep(const RecruitLds &w, int T, int M, int A, const double *tsc, const ProfileLds &lds) {
    const size_t M1 = (size_t)M + 1;
    const int lane = lane_id();
    const double NINF = neg_inf();
    const int n_strips = (M + 63) / 64;
    for (int s = 0; s < n_strips; ++s) {
        const int wd = min(64, M - 64 * s);
        const int j = 64 * s + lane + 1;
        const bool own = lane < wd;
        const Node nd = load_node(tsc, lds.msc, M1, A, own ? j : M);        // (idle lanes read a valid node and offer nothing)
        const bool last_strip = s == n_strips - 1;
        double x_out = NINF, y_out = NINF, x_held = NINF, v_i = NINF;
        int ex_out = 0, ey_out = 0, ex_held = 0, e_i = 0;
        int q = 0;                                                        // the stretch of this lane's row
        double run = NINF;                                                // LOCAL: the best match value of this column in stretch q,
        int run_row = 0, run_ent = 0;                                     // its row (the lowest) and its entry
        const int n_steps = T + wd - 1;
        for (int t = 0; t < n_steps; ++t) {
            const int i = t - lane;                                       // this lane's row, from 0
            const bool valid = own && i >= 0 && i < T;
            // what the left neighbour computed at the last step: X of its row i - 1 (for this lane's row i), Y = the delete state of (i, j)
            const double x_new = __shfl_up(x_out, 1, 64);
            const int ex_new = __shfl_up(ex_out, 1, 64);
            double v_d = __shfl_up(y_out, 1, 64);
            int e_d = __shfl_up(ey_out, 1, 64);
            double x_use = x_held;
            int e_m = ex_held;
            const int r = min(max(i, 0), T - 1);
            if (lane == 0) {
                const bool have = s > 0 && i < T;
                x_use = have ? w.bxy[2 * r] : NINF;
                v_d = have ? w.bxy[2 * r + 1] : NINF;
                e_m = have ? w.bent[2 * r] : 0;
                e_d = have ? w.bent[2 * r + 1] : 0;
            }
            x_held = x_new; ex_held = ex_new;
            const uint32_t c = w.res[r];
            const bool first = (c & kFirstResidue) != 0;                  // (row 0 is always one: the rows before it reset too)
            const double e = emission(lds.alpha, nd.mrow, c & 0x5Fu);
            double v_c = NINF;                                            // LOCAL: the match value without its B candidate
            int e_c = 0;
            if (LOCAL) {
                if (first) { x_use = NINF; v_i = NINF; v_d = NINF; }      // row 1 of a stretch: nothing continues into it
                v_c = x_use + e; e_c = e_m;
                if (!(x_use > 0.0)) { x_use = 0.0; e_m = (int)((uint32_t)j | (uint32_t)r << kLocalColBits); }   // B first: it wins an equality
            } else if (first) { x_use = 0.0; e_m = j; v_i = NINF; v_d = NINF; }        // row 1 of a stretch: B, no insert and no delete state
            const double v_m = x_use + e;
            const double c0 = v_m + nd.mm, c1 = v_i + nd.im, c2 = v_d + nd.dm;
            double X = c0; int eX = e_m;
            if (c1 > X) { X = c1; eX = e_i; }
            if (c2 > X) { X = c2; eX = e_d; }
            const double d0 = (LOCAL ? v_c : v_m) + nd.md, d1 = v_d + nd.dd;    // (LOCAL: no delete straight after the first match)
            double Y = d0; int eY = LOCAL ? e_c : e_m;
            if (d1 > Y) { Y = d1; eY = e_d; }
            if (first) Y = NINF;                                          // row 1 has no delete state
            const double i0 = v_m + nd.mi, i1 = v_i + nd.ii;
            double I = i0; int eI = e_m;
            if (i1 > I) { I = i1; eI = e_i; }
            if (j >= M) I = NINF;                                         // node M has no insert state
            x_out = X; y_out = Y; ex_out = eX; ey_out = eY;
            if (valid) {
                v_i = I; e_i = eI;
                if (!last_strip && lane == 63) {
                    w.bxy[2 * i + 1] = Y; w.bent[2 * i + 1] = eY;         // the delete state of (i, j + 1)
                    if (i + 1 < T) { w.bxy[2 * i + 2] = X; w.bent[2 * i + 2] = eX; }   // the candidate of the match state of (i + 1, j + 1)
                }
                if (LOCAL && v_m > run) { run = v_m; run_row = i; run_ent = e_m; }
                if (c & kLastResidue) {
                    if (LOCAL) {
                        if (run > w.slot[q].score) { w.slot[q].score = run; w.slot[q].jend = (int)((uint32_t)j | (uint32_t)run_row << kLocalColBits); w.slot[q].entry = run_ent; }
                        run = NINF;
                    } else if (v_m > w.slot[q].score) { w.slot[q].score = v_m; w.slot[q].jend = j; w.slot[q].entry = e_m; }
                    ++q;
                }
            }
        }
        wave_lds_fence();
    }
}

// the best frame of one read, as lane r of the wave that took it keeps it
struct ReadBest {
    double score;
    int32_t from, to;
    uint32_t aa, frame;              // of the best frame; of the lowest scored frame while none has a score
    uint32_t n_scored, residues;
};

// the longest reads [0, n_reads) hold, and the first of them longer than `limit`
__global__ __launch_bounds__(256) void recruit_lengths_kernel(const uint64_t *start, uint64_t n_reads, uint64_t limit, unsigned long long *out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    unsigned long long mx = 0, first = ~0ull;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_reads; r += stride) {
        const unsigned long long len = start[r + 1] - start[r];
        mx = max(mx, len);
        if (len > limit) first = min(first, (unsigned long long)r);
    }
    if (mx) atomicMax(&out[0], mx);
    if (first != ~0ull) atomicMin(&out[1], first);
}

template <bool MSC_LDS, bool LOCAL>
__global__ __launch_bounds__(256) void recruit_kernel(RecruitArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const size_t n_msc = ((size_t)a.M + 1) * a.A;
    const ProfileLds lds = profile_lds<MSC_LDS>(lds_raw, a.rows / 2 * 3, a.tab, a.alpha, n_msc);     // 24 bytes per row
    char *s_codon = reinterpret_cast<char *>(lds.past);
    for (int c = threadIdx.x; c < 64; c += blockDim.x) s_codon[c] = kRecruitCodon[c];
    __syncthreads();
    unsigned char *mine = lds.past + 64 + (size_t)wave_id() * recruit_wave_bytes(a.rows);
    const RecruitLds w{lds.bound, reinterpret_cast<int32_t *>(lds.bound + 2 * (size_t)a.rows), reinterpret_cast<volatile StretchSlot *>(mine),
                       mine + kRecruitSlots * sizeof(StretchSlot), s_codon};
    const int lane = lane_id();
    const double NINF = neg_inf();
    const double *tsc = a.tab + n_msc;

    for (;;) {
        const unsigned long long k = atomicAdd(&a.counters[RC_HEAD], lane == 0 ? (unsigned long long)a.chunk : 0ull);
        const uint64_t first = wave_uniform((uint64_t)k);
        if (first >= a.n_reads) break;
        const uint32_t cnt = (uint32_t)min((uint64_t)a.chunk, a.n_reads - first);
        ReadBest best{NINF, 0, 0, 0u, 0u, 0u, 0u};
        uint32_t T = 0, ns = 0;

        // the rows swept, and every stretch's result taken by the lane of its read, frames ascending: a later frame has to be better
        const auto flush = [&]() {
            if (ns == 0) return;
            wave_lds_fence();
            recruit_sweep<LOCAL>(w, (int)T, a.M, a.A, tsc, lds);
            for (uint32_t q = 0; q < ns; ++q) {
                const uint32_t rf = w.slot[q].read_frame, aa = w.slot[q].aa;
                const double sc = w.slot[q].score;
                if ((uint32_t)lane == (rf & 0xFFu)) {
                    const uint32_t frame = LOCAL ? (rf >> 8) & 7u : rf >> 8;
                    if (best.n_scored == 0) { best.frame = frame; best.aa = aa; }
                    ++best.n_scored;
                    best.residues += aa >> 16;
                    if (sc > best.score) {                                // stretches ascend by frame and position: the earlier keeps an equal score
                        const int32_t entry = w.slot[q].entry, jend = w.slot[q].jend;
                        best.score = sc; best.frame = frame;
                        if (LOCAL) {                                      // the aligned span: entry row .. end row of the stretch's rows
                            const uint32_t row_in = (uint32_t)entry >> kLocalColBits, row_out = (uint32_t)jend >> kLocalColBits;
                            best.from = entry & kLocalColMask; best.to = jend & kLocalColMask;
                            best.aa = ((aa & 0xFFFFu) + (row_in - (rf >> 12))) | ((row_out - row_in + 1u) << 16);
                        } else { best.from = entry; best.to = jend; best.aa = aa; }
                    }
                }
            }
            wave_lds_fence();
            T = 0; ns = 0;
        };

        for (uint32_t rl = 0; rl < cnt; ++rl) {
            const uint64_t s0 = a.start[first + rl];
            const uint32_t len = (uint32_t)(a.start[first + rl + 1] - s0);
            for (uint32_t f = 0; f < 6; ++f) {
                const int o = f >= 3 ? 1 : 0, same = o == a.reversed;     // the stored order, complemented when reversed, is orientation `reversed`
                const uint32_t comp = o ? 3u : 0u, off = f % 3;
                const uint32_t ncod = len >= off ? (len - off) / 3 : 0;
                // the residues [aa_from, aa_from + aa_len) of the frame into the rows, and their slot
                const auto take = [&](uint32_t aa_from, uint32_t aa_len) {
                    if (T + aa_len > a.rows || ns == kRecruitSlots) flush();
                    for (uint32_t c = (uint32_t)lane; c < aa_len; c += 64) {
                        const uint32_t ch = (uint32_t)(uint8_t)frame_residue(a, w.codon, s0, len, same, comp, off, aa_from + c);
                        w.res[T + c] = (uint8_t)(ch | (c == 0 ? kFirstResidue : 0u) | (c == aa_len - 1 ? kLastResidue : 0u));
                    }
                    if (lane == 0) {
                        w.slot[ns].score = NINF; w.slot[ns].jend = 0x7FFFFFFF; w.slot[ns].entry = 0;
                        w.slot[ns].read_frame = rl | (f << 8) | (LOCAL ? T << 12 : 0u); w.slot[ns].aa = aa_from | (aa_len << 16);
                    }
                    T += aa_len; ++ns;
                };
                // the longest run without a stop, the first of equally long ones; LOCAL: every run of min_aa residues, as it is found
                uint32_t run_start = 0, aa_len = 0, aa_from = 0;
                const uint32_t n_look = LOCAL ? ncod + 1 : ncod;           // (LOCAL: the frame's end closes its last run like a stop)
                for (uint32_t c0 = 0; c0 < n_look; c0 += 64) {
                    const uint32_t c = c0 + (uint32_t)lane;
                    bool stop = LOCAL && c == ncod;
                    if (c < ncod) stop = frame_residue(a, w.codon, s0, len, same, comp, off, c) == '*';
                    uint64_t m = __ballot(stop);
                    while (m) {
                        const uint32_t p = c0 + (uint32_t)__builtin_ctzll(m);
                        if (LOCAL) {
                            if (p - run_start >= a.min_aa) take(run_start, p - run_start);
                        } else if (p - run_start > aa_len) { aa_len = p - run_start; aa_from = run_start; }
                        run_start = p + 1;
                        m &= m - 1;
                    }
                }
                if (LOCAL) continue;
                if (ncod - run_start > aa_len) { aa_len = ncod - run_start; aa_from = run_start; }
                if (aa_len == 0 || aa_len < a.min_aa) continue;
                take(aa_from, aa_len);
            }
        }
        flush();

        // one writer per record: lane r the chunk's read r
        const bool mine_read = (uint32_t)lane < cnt;
        const bool unscored = mine_read && best.n_scored == 0;
        const bool unaligned = mine_read && best.n_scored > 0 && !(best.score > NINF);
        const bool hit = mine_read && best.n_scored > 0 && best.score > NINF && best.score >= a.min_score;
        if (mine_read && a.recs) {
            mgta_recruit_rec rec;
            rec.score = best.score; rec.model_from = unaligned ? 0 : best.from; rec.model_to = unaligned ? 0 : best.to;
            rec.aa_from = (uint16_t)(best.aa & 0xFFFFu); rec.aa_len = (uint16_t)(best.aa >> 16);
            rec.frame = (uint8_t)best.frame; rec.status = (uint8_t)(unscored ? 2 : unaligned ? 1 : 0); rec.pad[0] = 0; rec.pad[1] = 0;
            a.recs[first + (uint64_t)lane] = rec;
        }
        if (hit && a.col_diff) {
            atomicAdd(&a.col_diff[best.from - 1], 1ull);
            atomicAdd(&a.col_diff[best.to], ~0ull);
        }
        const uint64_t hits = __ballot(hit);
        const uint32_t n_frames = wave_sum(mine_read ? best.n_scored : 0u), n_res = wave_sum(mine_read ? best.residues : 0u);
        const uint64_t m_unal = __ballot(unaligned), m_unsc = __ballot(unscored);
        uint64_t m_frame[6];
#pragma unroll
        for (uint32_t f = 0; f < 6; ++f) m_frame[f] = __ballot(hit && best.frame == f);
        if (lane == 0) {
            const int sh = (int)(first & 63);
            if (hits) {
                atomicOr(&a.hit_bits[first >> 6], (unsigned long long)(hits << sh));
                if (sh && (hits >> (64 - sh))) atomicOr(&a.hit_bits[(first >> 6) + 1], (unsigned long long)(hits >> (64 - sh)));
                atomicAdd(&a.counters[RC_RECRUITED], (unsigned long long)__popcll(hits));
            }
            if (n_frames) atomicAdd(&a.counters[RC_FRAMES], (unsigned long long)n_frames);
            if (n_res) atomicAdd(&a.counters[RC_RESIDUES], (unsigned long long)n_res);
            if (m_unal) atomicAdd(&a.counters[RC_UNALIGNED], (unsigned long long)__popcll(m_unal));
            if (m_unsc) atomicAdd(&a.counters[RC_UNSCORED], (unsigned long long)__popcll(m_unsc));
#pragma unroll
            for (uint32_t f = 0; f < 6; ++f)
                if (m_frame[f]) atomicAdd(&a.counters[RC_FRAME0 + f], (unsigned long long)__popcll(m_frame[f]));
        }
    }
}

}  // namespace
}  // namespace mgta

using namespace mgta;

extern "C" {

int mgta_ctx_set_recruit_chunk(mgta_ctx *ctx, uint32_t reads) {
    if (!ctx) { set_error("mgta_ctx_set_recruit_chunk: ctx must not be NULL"); return MGTA_EINVAL; }
    ctx->recruit_chunk = reads;
    return MGTA_OK;
}

int mgta_reads_recruit(mgta_ctx *ctx, const mgta_hmm *hmm, const mgta_reads *reads, int reads_reversed, uint64_t n_short_reads, const mgta_recruit_params *params,
                       uint64_t *hit_bits, mgta_recruit_rec *recs, uint64_t *col_depth, mgta_recruit_stats *stats) {
    if (!ctx) { set_error("mgta_reads_recruit: ctx must not be NULL"); return MGTA_EINVAL; }
    if (!hmm || !reads) { set_error("mgta_reads_recruit: the model and the reads must not be NULL"); return MGTA_EINVAL; }
    if (hmm->ctx != ctx) { set_error("mgta_reads_recruit: the model belongs to another context"); return MGTA_EINVAL; }
    if (reads->ctx != ctx) { set_error("mgta_reads_recruit: the reads belong to another context"); return MGTA_EINVAL; }
    if (n_short_reads > reads->n_reads) {
        set_error("mgta_reads_recruit: n_short_reads = %llu, the library holds %llu reads", (unsigned long long)n_short_reads, (unsigned long long)reads->n_reads);
        return MGTA_EINVAL;
    }
    if (n_short_reads > 0 && !hit_bits) { set_error("mgta_reads_recruit: hit_bits must not be NULL"); return MGTA_EINVAL; }
    mgta_recruit_params par{20, 0, 20.0 * 0.6931471805599453};
    if (params) par = *params;
    if (par.min_aa < 1) { set_error("mgta_reads_recruit: min_aa = %d (>= 1 is required)", (int)par.min_aa); return MGTA_EINVAL; }
    if (std::isnan(par.min_score)) { set_error("mgta_reads_recruit: min_score must not be NaN"); return MGTA_EINVAL; }
    if (par.mode != MGTA_RECRUIT_GLOBAL && par.mode != MGTA_RECRUIT_LOCAL) {
        set_error("mgta_reads_recruit: mode = %d (0 = MGTA_RECRUIT_GLOBAL or 1 = MGTA_RECRUIT_LOCAL is required)", (int)par.mode);
        return MGTA_EINVAL;
    }
    const int M = hmm->M, A = hmm->A;
    const bool local = par.mode == MGTA_RECRUIT_LOCAL;
    if (local && M > kLocalColMask) {
        set_error("mgta_reads_recruit: local mode takes a model of at most %d columns, this one has %d", kLocalColMask, M);
        return MGTA_EINVAL;
    }
    if (n_short_reads == 0) {
        if (col_depth) memset(col_depth, 0, (size_t)M * 8);
        if (stats) memset(stats, 0, sizeof(*stats));
        return MGTA_OK;
    }
    return guarded("mgta_reads_recruit", [&]() {
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        uint64_t *live = &ctx->live_bytes, *peak = &ctx->peak_bytes;
        const uint64_t n = n_short_reads, n_words = (n + 63) / 64;

        // the longest read sizes the rows; a read beyond the limit ends the call before anything is written
        DevBuf d_len;
        d_len.alloc(16, live, peak);
        const unsigned long long len_init[2] = {0ull, ~0ull};
        MGTA_HIP_CHECK(hipMemcpyAsync(d_len.p, len_init, 16, hipMemcpyHostToDevice, st));
        Timer t_scan(st), t_fill(st);
        t_scan.start();
        hipLaunchKernelGGL(recruit_lengths_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->num_cus * 8)), dim3(256), 0, st, reads->d_start, n,
                           (uint64_t)kRecruitMaxBases, d_len.as<unsigned long long>());
        MGTA_HIP_CHECK(hipGetLastError());
        t_scan.end();
        unsigned long long len_out[2];
        MGTA_HIP_CHECK(hipMemcpyAsync(len_out, d_len.p, 16, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        if (len_out[1] != ~0ull) {
            set_error("mgta_reads_recruit: read %llu holds more than %u bases (4096 residues per frame is the limit)", len_out[1], kRecruitMaxBases);
            return (int)MGTA_EINVAL;
        }

        const uint32_t rows = std::max<uint32_t>(kRecruitRows, ((uint32_t)(len_out[0] / 3) + 7u) & ~7u);
        const size_t per_wave = (size_t)rows * 24 + recruit_wave_bytes(rows), fixed = kAlphaLdsBytes + 64;
        const size_t msc_bytes = ((size_t)M + 1) * A * 8;
        const size_t budget = fixed + per_wave <= kRecruitLdsBudget ? kRecruitLdsBudget : kRecruitLdsMax;
        const int waves = waves_that_fit(1, per_wave, fixed, budget);
        size_t lds = fixed + (size_t)waves * per_wave;
        const bool msc_lds = lds + msc_bytes <= budget;
        if (msc_lds) lds += msc_bytes;
        const auto kernel = local ? (msc_lds ? recruit_kernel<true, true> : recruit_kernel<false, true>) : (msc_lds ? recruit_kernel<true, false> : recruit_kernel<false, false>);
        const int blocks_per_cu = blocks_per_cu_of(kernel, waves, lds);
        // reads per grab: the switch, else 4 where every wave in flight still gets several grabs (400 k reads of 150 bases, M = 300:
        // 97.2 ms at 1, 94.4 at 4, 95.7 at 16, 112.6 at 64, where the last grabs leave waves idle; profiles/recruit/README.md)
        const uint64_t in_flight = (uint64_t)ctx->num_cus * (uint64_t)blocks_per_cu * (uint64_t)waves;
        uint32_t chunk = ctx->recruit_chunk ? ctx->recruit_chunk : (uint32_t)std::min<uint64_t>(4, std::max<uint64_t>(1, n / (in_flight * 4)));
        chunk = std::min(chunk, kRecruitMaxChunk);

        DevBuf d_bits, d_recs, d_diff, d_cnt;
        d_bits.alloc(n_words * 8, live, peak);
        d_diff.alloc(((size_t)M + 1) * 8, live, peak);
        d_cnt.alloc(RC_NUM * 8, live, peak);
        if (recs) d_recs.alloc(n * sizeof(mgta_recruit_rec), live, peak);
        MGTA_HIP_CHECK(hipMemsetAsync(d_bits.p, 0, n_words * 8, st));
        MGTA_HIP_CHECK(hipMemsetAsync(d_diff.p, 0, ((size_t)M + 1) * 8, st));
        MGTA_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, RC_NUM * 8, st));

        RecruitArgs ra;
        ra.packed = reads->d_packed; ra.start = reads->d_start; ra.n_reads = n; ra.reversed = reads_reversed ? 1 : 0; ra.chunk = chunk;
        ra.M = M; ra.A = A; ra.tab = hmm->tab.as<double>(); ra.alpha = hmm->d_alpha.as<int8_t>(); ra.rows = rows; ra.min_aa = (uint32_t)par.min_aa;
        ra.min_score = par.min_score; ra.hit_bits = d_bits.as<unsigned long long>(); ra.recs = recs ? d_recs.as<mgta_recruit_rec>() : nullptr;
        ra.col_diff = col_depth ? d_diff.as<unsigned long long>() : nullptr; ra.counters = d_cnt.as<unsigned long long>();
        t_fill.start();
        const unsigned grid = launch_waves(ctx, kernel, ra, waves, lds, (n + chunk - 1) / chunk, blocks_per_cu).grid;
        t_fill.end();

        std::vector<unsigned long long> diff((size_t)M + 1), cnt(RC_NUM);
        MGTA_HIP_CHECK(hipMemcpyAsync(hit_bits, d_bits.p, n_words * 8, hipMemcpyDeviceToHost, st));
        if (recs) MGTA_HIP_CHECK(hipMemcpyAsync(recs, d_recs.p, n * sizeof(mgta_recruit_rec), hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(diff.data(), d_diff.p, ((size_t)M + 1) * 8, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(cnt.data(), d_cnt.p, RC_NUM * 8, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        if (col_depth) {
            unsigned long long run = 0;
            for (int j = 0; j < M; ++j) { run += diff[(size_t)j]; col_depth[j] = run; }
        }
        if (stats) {
            memset(stats, 0, sizeof(*stats));
            stats->n_reads = (int64_t)n; stats->n_frames_scored = (int64_t)cnt[RC_FRAMES]; stats->n_cells = (int64_t)cnt[RC_RESIDUES] * M;
            stats->n_unaligned = (int64_t)cnt[RC_UNALIGNED]; stats->n_unscored = (int64_t)cnt[RC_UNSCORED]; stats->n_recruited = (int64_t)cnt[RC_RECRUITED];
            for (int f = 0; f < 6; ++f) stats->n_recruited_frame[f] = (int64_t)cnt[RC_FRAME0 + f];
            stats->blocks_per_cu = blocks_per_cu; stats->waves_per_block = waves; stats->grid_blocks = grid; stats->lds_bytes = (int64_t)lds;
            stats->msc_in_lds = msc_lds ? 1 : 0; stats->rows_per_wave = rows; stats->chunk = chunk;
            stats->ms_scan = t_scan.ms(); stats->ms_fill = t_fill.ms();
        }
        return (int)MGTA_OK;
    });
}

}  // extern "C"
