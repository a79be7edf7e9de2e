// posterior.hip — Forward score and per-residue posteriors of protein sequences on a profile HMM (mgta_seqs_posterior): how far the
// placement of mgta_seqs_align can be trusted.  The rule is this library's own (include/megagta_hip.h): mgta_seqs_align's cells with
// every max replaced by log-sum-exp, fp64, a backward sweep over the same cells, posterior = exp(forward + backward - F).
//
// Forward.  align_fill_kernel's scheme: one wave owns a sequence; waves take sequences longest first from one atomic head.  Lanes own
// model columns, 64 at a time (a strip); at step t of a strip lane l computes row i = t - l + 1 of its column j.  Written from the
// cell outwards: the lane of cell (i, j) holds the seven transitions out of node j and computes what its neighbours need,
//     X = lse(FM + MM, FI + IM, FD + DM)   the sum into FM[i+1][j+1]  (taken by lane l + 1 two steps later)
//     Y = lse(FM + MD, FD + DD)            FD[i][j+1]                 (taken by lane l + 1 at the next step)
//     I = lse(FM + MI, FI + II)            FI[i+1][j]                 (its own next step)
// X and Y move to lane l + 1 by a cross-lane move; the last lane of a strip leaves them per row in LDS for lane 0 of the next strip
// (one wave, LDS in program order: row i is read before the rows <= i - 62 are written, in place).  FM and FI of every cell are
// stored, two planes of doubles, a strip of width w at ((i - 1 + l) mod L) * w + l: a step's lanes write one run.  FD is not kept.
//
// Backward.  The mirror: strips from the last to the first, at step t lane l computes row i = L - t + (w - 1 - l), the neighbour is
// column j + 1 (lane l + 1, or LDS across a strip edge: lane 0 writes row i while lane 63 reads the rows <= i - 62).  Every
// transition of the backward recurrence leaves node j, so the lane of (i, j) again needs only its own seven.  It hands
//     N = e(j, x_i) + BM[i][j]             to cell (i-1, j-1)  (taken by lane l - 1 two steps later)
//     BD[i][j]                             to cell (i, j-1)    (taken by lane l - 1 at the next step)
//     BI[i][j]                             to cell (i-1, j)    (its own next step)
// reads FM and FI of its cell back, adds the two posteriors into two registers (rows descend: one fixed order per column) and
// writes pp of a residue whose label names this cell (the labels of the sequence sit in LDS).  No atomics on floating-point values:
// every output has one writer.
//
// lse.  lse(a, b, c) = m + log(exp(a - m) + exp(b - m) + exp(c - m)), m the maximum; the term of the maximum is exp(0) = 1, so two
// exponentials and one logarithm are evaluated.  m = -inf gives -inf and -inf - -inf is never evaluated.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "device_utils.hpp"

namespace mgta {
namespace {

constexpr int kPostMaxLen = 4096;                  // residues of one sequence: 20 bytes of LDS per row of the wave that owns it
constexpr size_t kPostLdsBudget = 82 * 1024;       // of a workgroup: the longest sequence alone (4096 * 20 + 128 bytes) still fits
constexpr int kPostAlphaBytes = 128;
constexpr uint64_t kPostCellBytes = 16;            // FM and FI of a cell

__device__ __forceinline__ double neg_inf() { return -__builtin_huge_val(); }

__device__ __forceinline__ double lse2(double a, double b) {
    const double m = fmax(a, b), lo = fmin(a, b);
    const double mm = m == neg_inf() ? 0.0 : m;                           // (lo is -inf too then: no -inf - -inf)
    const double r = mm + log(1.0 + exp(lo - mm));
    return m == neg_inf() ? neg_inf() : r;
}

__device__ __forceinline__ double lse3(double a, double b, double c) {
    const double hi = fmax(a, b), lo = fmin(a, b);
    const double m = fmax(hi, c), mid = fmin(hi, c);
    const double mm = m == neg_inf() ? 0.0 : m;
    const double r = mm + log(1.0 + (exp(lo - mm) + exp(mid - mm)));
    return m == neg_inf() ? neg_inf() : r;
}

__device__ __forceinline__ double wave_lse(double v) {                    // the same value in every lane: lse2 is symmetric
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = lse2(v, __shfl_xor(v, d, 64));
    return v;
}

struct PostArgs {
    const uint8_t *seqs;         // the letters of every sequence
    const uint64_t *off;         // [n + 1] into seqs
    const uint32_t *order;       // the batch: sequence numbers, longest first
    const uint64_t *cell_base;   // [count] where the cells of a batch item start in fm / fi
    uint32_t count;
    int M, A;
    const double *tab;           // [msc (M+1)*A][tsc 7*(M+1)] ...
    const int8_t *alpha;         // [128]
    double *fm, *fi;             // FM and FI of every cell of the batch
    double *fwd, *bwd;           // [count] F, Bt
    const int32_t *labels;       // [letters] or NULL (backward)
    double *pp;                  // [letters] or NULL, zero before the launch (backward)
    double *col_m, *col_i;       // [count * M] or NULL, zero before the launch (backward)
    uint32_t rows_lds;           // rows a wave has in LDS (>= the longest sequence of the batch)
    unsigned long long *head;
};

template <bool MSC_LDS>
__global__ __launch_bounds__(256) void post_forward_kernel(PostArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    // [alpha 128 B][boundary: waves x rows_lds x (X, Y)][msc (M+1)*A doubles when MSC_LDS]
    int8_t *s_alpha = reinterpret_cast<int8_t *>(lds_raw);
    const int n_waves = blockDim.x >> 6;
    double *s_bound = reinterpret_cast<double *>(lds_raw + kPostAlphaBytes) + (size_t)wave_id() * a.rows_lds * 2;
    double *s_msc = reinterpret_cast<double *>(lds_raw + kPostAlphaBytes) + (size_t)n_waves * a.rows_lds * 2;
    const int M = a.M, A = a.A;
    const size_t M1 = (size_t)M + 1;
    for (int c = threadIdx.x; c < kPostAlphaBytes; c += blockDim.x) s_alpha[c] = a.alpha[c];
    if (MSC_LDS)
        for (size_t c = threadIdx.x; c < M1 * A; c += blockDim.x) s_msc[c] = a.tab[c];
    __syncthreads();
    const double *msc = MSC_LDS ? s_msc : a.tab;
    const double *tsc = a.tab + M1 * A;
    const int lane = lane_id();
    const double NINF = neg_inf();
    const int n_strips = (M + 63) / 64;

    for (;;) {
        // every lane takes part and only lane 0 counts (align_fill_kernel: no branch on the lane in front of the wave-wide read)
        unsigned long long k = atomicAdd(a.head, lane == 0 ? 1ull : 0ull);
        k = wave_uniform((uint64_t)k);
        if (k >= a.count) break;
        const uint32_t idx = a.order[k];
        const uint64_t o0 = a.off[idx];
        const int L = (int)(a.off[idx + 1] - o0);
        if (L == 0) {
            if (lane == 0) a.fwd[k] = NINF;
            continue;
        }
        const uint8_t *x = a.seqs + o0;
        double *pm = a.fm + a.cell_base[k], *pi = a.fi + a.cell_base[k];
        double f_acc = NINF;                                              // lse of this lane's FM[L][.] over the strips
        for (int s = 0; s < n_strips; ++s) {
            const int w = min(64, M - 64 * s);
            const int j = 64 * s + lane + 1;
            const bool own = lane < w;
            const int jc = own ? j : M;                                   // (idle lanes read a valid node and store nothing)
            const double tMM = tsc[0 * M1 + jc], tMI = tsc[1 * M1 + jc], tMD = tsc[2 * M1 + jc], tIM = tsc[3 * M1 + jc], tII = tsc[4 * M1 + jc],
                         tDM = tsc[5 * M1 + jc], tDD = tsc[6 * M1 + jc];
            const double *mrow = msc + (size_t)jc * A;
            double *pms = pm + (size_t)s * 64 * L, *pis = pi + (size_t)s * 64 * L;
            const bool last_strip = s == n_strips - 1;
            double x_out = NINF, y_out = NINF, x_held = NINF, v_i = NINF;
            const int n_steps = L + w - 1;
            int t_mod = 0;                                                // t mod L
            for (int t = 0; t < n_steps; ++t) {
                const int i = t - lane + 1;                               // this lane's row
                const bool valid = own && i >= 1 && i <= L;
                // what the left neighbour computed at the last step: X of its row i (for this lane's row i + 1), Y = FD[i][j]
                double x_new = __shfl_up(x_out, 1, 64), v_d = __shfl_up(y_out, 1, 64);
                double x_use = x_held;
                if (lane == 0) {
                    const int r = min(max(i, 1), L) - 1;                  // = i - 1: lane 0 is valid at every step t < L
                    const bool have = s > 0 && i <= L;
                    x_use = have ? s_bound[2 * r] : NINF;
                    v_d = have ? s_bound[2 * r + 1] : NINF;
                }
                x_held = x_new;
                const int ii = min(max(i, 1), L);
                const uint32_t c = x[ii - 1];
                const int col = c < 127 ? (int)s_alpha[c] : -1;
                const double e = col < 0 ? 0.0 : mrow[col];
                if (i <= 1) { x_use = 0.0; v_i = NINF; v_d = NINF; }      // row 1: FM = e, no insert and no delete state
                const double v_m = x_use + e;
                const double X = lse3(v_m + tMM, v_i + tIM, v_d + tDM);
                double Y = lse2(v_m + tMD, v_d + tDD);
                if (i <= 1) Y = NINF;                                     // FD[1][.] does not exist
                double I = lse2(v_m + tMI, v_i + tII);
                if (j >= M) I = NINF;                                     // node M has no insert state
                x_out = X; y_out = Y;
                if (valid) {
                    const size_t at = (size_t)t_mod * w + lane;           // (i - 1 + lane) mod L = t mod L
                    pms[at] = v_m;
                    pis[at] = v_i;
                    v_i = I;
                    if (i == L) f_acc = lse2(f_acc, v_m);
                    if (!last_strip && lane == 63) {
                        s_bound[2 * (i - 1) + 1] = Y;                     // FD[i][j + 1]
                        if (i < L) s_bound[2 * i] = X;                    // the sum into FM[i + 1][j + 1]
                    }
                }
                if (++t_mod == L) t_mod = 0;
            }
            wave_lds_fence();
        }
        const double F = wave_lse(f_acc);
        if (lane == 0) a.fwd[k] = F;
    }
}

template <bool MSC_LDS>
__global__ __launch_bounds__(256) void post_backward_kernel(PostArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    // [alpha 128 B][boundary: waves x rows_lds x (N, BD)][msc (M+1)*A doubles when MSC_LDS][labels: waves x rows_lds x int32]
    int8_t *s_alpha = reinterpret_cast<int8_t *>(lds_raw);
    const int n_waves = blockDim.x >> 6;
    const int M = a.M, A = a.A;
    const size_t M1 = (size_t)M + 1;
    double *s_bound = reinterpret_cast<double *>(lds_raw + kPostAlphaBytes) + (size_t)wave_id() * a.rows_lds * 2;
    double *s_msc = reinterpret_cast<double *>(lds_raw + kPostAlphaBytes) + (size_t)n_waves * a.rows_lds * 2;
    int32_t *s_lab = reinterpret_cast<int32_t *>(s_msc + (MSC_LDS ? M1 * A : 0)) + (size_t)wave_id() * a.rows_lds;
    for (int c = threadIdx.x; c < kPostAlphaBytes; c += blockDim.x) s_alpha[c] = a.alpha[c];
    if (MSC_LDS)
        for (size_t c = threadIdx.x; c < M1 * A; c += blockDim.x) s_msc[c] = a.tab[c];
    __syncthreads();
    const double *msc = MSC_LDS ? s_msc : a.tab;
    const double *tsc = a.tab + M1 * A;
    const int lane = lane_id();
    const double NINF = neg_inf();
    const int n_strips = (M + 63) / 64;
    const bool want_pp = a.labels != nullptr && a.pp != nullptr;

    for (;;) {
        unsigned long long k = atomicAdd(a.head, lane == 0 ? 1ull : 0ull);
        k = wave_uniform((uint64_t)k);
        if (k >= a.count) break;
        const uint32_t idx = a.order[k];
        const uint64_t o0 = a.off[idx];
        const int L = (int)(a.off[idx + 1] - o0);
        const double F = L > 0 ? a.fwd[k] : NINF;
        if (L == 0 || F == NINF) {                                        // unaligned: pp and the column sums stay zero
            if (lane == 0) a.bwd[k] = NINF;
            continue;
        }
        const uint8_t *x = a.seqs + o0;
        const double *pm = a.fm + a.cell_base[k], *pi = a.fi + a.cell_base[k];
        if (want_pp) {
            for (int r = lane; r < L; r += 64) s_lab[r] = a.labels[o0 + r];
            wave_lds_fence();
        }
        double bt_acc = NINF;                                             // lse of this lane's e(j, x_1) + BM[1][j] over the strips
        for (int s = n_strips - 1; s >= 0; --s) {
            const int w = min(64, M - 64 * s);
            const int j = 64 * s + lane + 1;
            const bool own = lane < w;
            const int jc = own ? j : M;
            const double tMM = tsc[0 * M1 + jc], tMI = tsc[1 * M1 + jc], tMD = tsc[2 * M1 + jc], tIM = tsc[3 * M1 + jc], tII = tsc[4 * M1 + jc],
                         tDM = tsc[5 * M1 + jc], tDD = tsc[6 * M1 + jc];
            const double *mrow = msc + (size_t)jc * A;
            const double *pms = pm + (size_t)s * 64 * L, *pis = pi + (size_t)s * 64 * L;
            const bool rightmost = s == n_strips - 1;                     // no column behind this strip
            double n_out = NINF, d_out = NINF, n_held = NINF, b_i = NINF, sum_m = 0.0, sum_i = 0.0;
            const int n_steps = L + w - 1;
            int r_mod = (L + w - 2) % L;                                  // (i - 1 + lane) mod L = (L + w - 2 - t) mod L
            for (int t = 0; t < n_steps; ++t) {
                const int i = L - t + (w - 1 - lane);                     // this lane's row
                const bool valid = own && i >= 1 && i <= L;
                // what the right neighbour computed at the last step: N of its row i (for this lane's row i - 1), BD[i][j + 1]
                double n_new = __shfl_down(n_out, 1, 64), b_d = __shfl_down(d_out, 1, 64);
                double n_use = n_held;
                if (lane == w - 1) {                                      // valid at every step t < L
                    const int ii = min(max(i, 1), L);
                    const bool have = !rightmost && i >= 1;
                    n_use = have && i < L ? s_bound[2 * ii] : NINF;       // N of row i + 1
                    b_d = have ? s_bound[2 * (ii - 1) + 1] : NINF;        // BD[i][j + 1]
                }
                n_held = n_new;
                const int ii = min(max(i, 1), L);
                const uint32_t c = x[ii - 1];
                const int col = c < 127 ? (int)s_alpha[c] : -1;
                const double e = col < 0 ? 0.0 : mrow[col];
                double BM = lse3(tMM + n_use, tMI + b_i, tMD + b_d);      // (b_i is -inf at j = M, b_d at j = M and from row 1)
                double BI = lse2(tIM + n_use, tII + b_i);
                double BD = lse2(tDM + n_use, tDD + b_d);
                if (i >= L) { BM = 0.0; BI = NINF; BD = NINF; }           // row L: the alignment ends in a match state
                if (i <= 1) { BI = NINF; BD = NINF; }                     // row 1 has no insert and no delete state
                if (j >= M) { BI = NINF; BD = NINF; }                     // node M has no insert state, and nothing behind it
                if (j <= 1) BD = NINF;                                    // FD[.][1] does not exist
                const double N = e + BM;
                n_out = N; d_out = BD; b_i = BI;
                if (valid) {
                    const size_t at = (size_t)r_mod * w + lane;
                    const double f_m = pms[at], f_i = pis[at];
                    const double p_m = (f_m == NINF || BM == NINF) ? 0.0 : exp(f_m + BM - F);
                    const double p_i = (f_i == NINF || BI == NINF) ? 0.0 : exp(f_i + BI - F);
                    sum_m += p_m; sum_i += p_i;
                    if (want_pp) {
                        const int lab = s_lab[i - 1];
                        if (lab == j) a.pp[o0 + i - 1] = p_m;
                        else if (lab == -j) a.pp[o0 + i - 1] = p_i;
                    }
                    if (i == 1) bt_acc = lse2(bt_acc, N);
                    if (s > 0 && lane == 0) {
                        s_bound[2 * (i - 1)] = N;
                        s_bound[2 * (i - 1) + 1] = BD;
                    }
                }
                r_mod = r_mod == 0 ? L - 1 : r_mod - 1;
            }
            if (own) {
                if (a.col_m) a.col_m[(size_t)k * M + j - 1] = sum_m;
                if (a.col_i) a.col_i[(size_t)k * M + j - 1] = sum_i;
            }
            wave_lds_fence();
        }
        const double Bt = wave_lse(bt_acc);
        if (lane == 0) a.bwd[k] = Bt;
    }
}

}  // namespace
}  // namespace mgta

using namespace mgta;

extern "C" {

int mgta_ctx_set_posterior_batch(mgta_ctx *ctx, int64_t cells) {
    if (!ctx) { set_error("mgta_ctx_set_posterior_batch: ctx must not be NULL"); return MGTA_EINVAL; }
    if (cells < 0) { set_error("mgta_ctx_set_posterior_batch: cells = %lld must not be negative", (long long)cells); return MGTA_EINVAL; }
    ctx->posterior_batch_cells = (uint64_t)cells;
    return MGTA_OK;
}

int mgta_seqs_posterior(mgta_ctx *ctx, const mgta_hmm *hmm, const char *seqs, const uint64_t *offsets, int64_t n, const int32_t *labels, mgta_post_rec *recs,
                        double *pp, double *col_match, double *col_insert, mgta_post_stats *stats) {
    if (!ctx) { set_error("mgta_seqs_posterior: ctx must not be NULL"); return MGTA_EINVAL; }
    if (!hmm) { set_error("mgta_seqs_posterior: the model must not be NULL"); return MGTA_EINVAL; }
    if (hmm->ctx != ctx) { set_error("mgta_seqs_posterior: the model belongs to another context"); return MGTA_EINVAL; }
    if (n < 0) { set_error("mgta_seqs_posterior: n = %lld must not be negative", (long long)n); return MGTA_EINVAL; }
    if (n >= (1ll << 31)) { set_error("mgta_seqs_posterior: n = %lld (the limit is n < 2^31 sequences)", (long long)n); return MGTA_EINVAL; }
    if (n > 0 && !offsets) { set_error("mgta_seqs_posterior: offsets must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && !recs) { set_error("mgta_seqs_posterior: recs must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && pp && !labels) { set_error("mgta_seqs_posterior: labels must not be NULL when pp is given"); return MGTA_EINVAL; }
    for (int64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) { set_error("mgta_seqs_posterior: sequence %lld: offsets must ascend", (long long)i); return MGTA_EINVAL; }
        if (offsets[i + 1] - offsets[i] > (uint64_t)kPostMaxLen) {
            set_error("mgta_seqs_posterior: sequence %lld holds %llu residues (the limit is %d residues per sequence)", (long long)i,
                      (unsigned long long)(offsets[i + 1] - offsets[i]), kPostMaxLen);
            return MGTA_EINVAL;
        }
    }
    if (n > 0 && offsets[n] > offsets[0] && !seqs) { set_error("mgta_seqs_posterior: seqs must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && labels) {
        const int64_t M = hmm->M;
        for (int64_t i = 0; i < n; ++i)
            for (uint64_t r = offsets[i]; r < offsets[i + 1]; ++r)
                if (labels[r] > M || labels[r] <= -M) {
                    set_error("mgta_seqs_posterior: sequence %lld, residue %llu: label %d (a match state is 1 .. %lld, an insert state -1 .. -%lld, none is 0)",
                              (long long)i, (unsigned long long)(r - offsets[i]), labels[r], (long long)M, (long long)(M - 1));
                    return MGTA_EINVAL;
                }
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return MGTA_OK;
    return guarded("mgta_seqs_posterior", [&]() {
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        uint64_t *live = &ctx->live_bytes, *peak = &ctx->peak_bytes;
        struct PeakOfCall {                                               // peak_bytes is this call's while it runs, the context's again on every way out
            uint64_t *peak, before;
            ~PeakOfCall() { *peak = std::max(*peak, before); }
        } peak_of_call{peak, *peak};
        *peak = *live;
        const uint32_t nn = (uint32_t)n;
        const int M = hmm->M, A = hmm->A;
        const uint64_t n_letters = offsets[n] - offsets[0];
        const size_t msc_bytes = ((size_t)M + 1) * A * 8;
        const bool want_pp = labels && pp;

        // the letters, the labels and where they start, once; the sequences longest first
        std::vector<uint64_t> rel((size_t)nn + 1);
        for (uint32_t i = 0; i <= nn; ++i) rel[i] = offsets[i] - offsets[0];
        std::vector<uint32_t> order(nn);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return rel[x + 1] - rel[x] > rel[y + 1] - rel[y]; });
        DevBuf d_seqs, d_off, d_order, d_head, d_labels, d_pp;
        d_seqs.alloc(n_letters + 16, live, peak);
        d_off.alloc((size_t)(nn + 1) * 8, live, peak);
        d_order.alloc((size_t)nn * 4, live, peak);
        d_head.alloc(64, live, peak);
        if (n_letters) MGTA_HIP_CHECK(hipMemcpyAsync(d_seqs.p, seqs + offsets[0], n_letters, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_off.p, rel.data(), (size_t)(nn + 1) * 8, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_order.p, order.data(), (size_t)nn * 4, hipMemcpyHostToDevice, st));
        if (want_pp) {
            d_labels.alloc((size_t)n_letters * 4 + 16, live, peak);
            d_pp.alloc((size_t)n_letters * 8 + 16, live, peak);
            if (n_letters) MGTA_HIP_CHECK(hipMemcpyAsync(d_labels.p, labels + offsets[0], (size_t)n_letters * 4, hipMemcpyHostToDevice, st));
            MGTA_HIP_CHECK(hipMemsetAsync(d_pp.p, 0, (size_t)n_letters * 8 + 16, st));
        }

        // cells of a batch: the switch, or what half of the memory the context may still take holds (16 bytes per cell; the rest of
        // a batch's buffers are far smaller)
        uint64_t avail = 0;
        {
            size_t free_b = 0, total_b = 0;
            MGTA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            avail = free_b;
            if (ctx->mem_limit) avail = std::min<uint64_t>(avail, ctx->mem_limit > ctx->live_bytes ? ctx->mem_limit - ctx->live_bytes : 0);
        }
        uint64_t cap = ctx->posterior_batch_cells;
        if (!cap) cap = std::max<uint64_t>(avail / 2 / kPostCellBytes, 1);

        Timer t_fwd(st), t_bwd(st);
        double ms_fwd = 0, ms_bwd = 0;
        int64_t n_batches = 0, n_scored = 0, n_cells = 0, max_bpc = 0, min_wpb = 4, max_grid = 0, max_lds = 0, all_msc_lds = 1;
        std::vector<uint64_t> cell_base;
        std::vector<double> h_fwd, h_bwd, h_cm, h_ci;
        for (uint32_t b0 = 0; b0 < nn;) {
            // the batch [b0, b1): at least one sequence
            uint32_t b1 = b0;
            uint64_t cells = 0;
            cell_base.clear();
            while (b1 < nn) {
                const uint64_t L = rel[order[b1] + 1] - rel[order[b1]];
                if (b1 > b0 && cells + L * (uint64_t)M > cap) break;
                cell_base.push_back(cells);
                cells += L * (uint64_t)M;
                ++b1;
            }
            const uint32_t count = b1 - b0;
            const uint64_t plane_bytes = cells * 8 + 16;
            if (2 * plane_bytes > avail) {                                // (one sequence alone may be more than the device has left)
                set_error("mgta_seqs_posterior: a batch of %llu cells needs %llu bytes of device memory and %llu are left", (unsigned long long)cells,
                          (unsigned long long)(2 * plane_bytes), (unsigned long long)avail);
                return (int)MGTA_ENOMEM;
            }
            const uint32_t l_max = (uint32_t)(rel[order[b0] + 1] - rel[order[b0]]);
            const uint32_t rows_lds = std::max(1u, l_max);
            // one geometry for both kernels: the backward one needs 4 more bytes per row, for the labels
            int waves = 4;
            while (waves > 1 && kPostAlphaBytes + (size_t)waves * rows_lds * 20 > kPostLdsBudget) waves >>= 1;
            size_t lds_f = kPostAlphaBytes + (size_t)waves * rows_lds * 16, lds_b = kPostAlphaBytes + (size_t)waves * rows_lds * 20;
            const bool msc_lds = lds_b + msc_bytes <= kPostLdsBudget;
            if (msc_lds) { lds_f += msc_bytes; lds_b += msc_bytes; }

            DevBuf d_fm, d_fi, d_cbase, d_fwd, d_bwd, d_cm, d_ci;
            d_fm.alloc(plane_bytes, live, peak);
            d_fi.alloc(plane_bytes, live, peak);
            d_cbase.alloc((size_t)count * 8, live, peak);
            d_fwd.alloc((size_t)count * 8, live, peak);
            d_bwd.alloc((size_t)count * 8, live, peak);
            MGTA_HIP_CHECK(hipMemcpyAsync(d_cbase.p, cell_base.data(), (size_t)count * 8, hipMemcpyHostToDevice, st));
            if (col_match) {
                d_cm.alloc((size_t)count * M * 8, live, peak);
                MGTA_HIP_CHECK(hipMemsetAsync(d_cm.p, 0, (size_t)count * M * 8, st));
            }
            if (col_insert) {
                d_ci.alloc((size_t)count * M * 8, live, peak);
                MGTA_HIP_CHECK(hipMemsetAsync(d_ci.p, 0, (size_t)count * M * 8, st));
            }

            PostArgs pa;
            pa.seqs = d_seqs.as<uint8_t>(); pa.off = d_off.as<uint64_t>(); pa.order = d_order.as<uint32_t>() + b0; pa.cell_base = d_cbase.as<uint64_t>();
            pa.count = count; pa.M = M; pa.A = A; pa.tab = hmm->tab.as<double>(); pa.alpha = hmm->d_alpha.as<int8_t>();
            pa.fm = d_fm.as<double>(); pa.fi = d_fi.as<double>(); pa.fwd = d_fwd.as<double>(); pa.bwd = d_bwd.as<double>();
            pa.labels = want_pp ? d_labels.as<int32_t>() : nullptr; pa.pp = want_pp ? d_pp.as<double>() : nullptr;
            pa.col_m = col_match ? d_cm.as<double>() : nullptr; pa.col_i = col_insert ? d_ci.as<double>() : nullptr;
            pa.rows_lds = rows_lds; pa.head = d_head.as<unsigned long long>();
            // workgroups a CU holds at once: what the runtime answers for these registers and this LDS (never assumed)
            const void *fn_f = msc_lds ? reinterpret_cast<const void *>(post_forward_kernel<true>) : reinterpret_cast<const void *>(post_forward_kernel<false>);
            const void *fn_b = msc_lds ? reinterpret_cast<const void *>(post_backward_kernel<true>) : reinterpret_cast<const void *>(post_backward_kernel<false>);
            MGTA_HIP_CHECK(hipFuncSetAttribute(fn_f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_f));
            MGTA_HIP_CHECK(hipFuncSetAttribute(fn_b, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
            int bpc_f = 0, bpc_b = 0;
            if (msc_lds) {
                MGTA_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc_f, post_forward_kernel<true>, waves * 64, lds_f));
                MGTA_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc_b, post_backward_kernel<true>, waves * 64, lds_b));
            } else {
                MGTA_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc_f, post_forward_kernel<false>, waves * 64, lds_f));
                MGTA_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc_b, post_backward_kernel<false>, waves * 64, lds_b));
            }
            const int blocks_per_cu = std::max(1, std::min(bpc_f, bpc_b));
            const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)ctx->num_cus * (uint64_t)blocks_per_cu, ((uint64_t)count + waves - 1) / waves);
            MGTA_HIP_CHECK(hipMemsetAsync(d_head.p, 0, 64, st));
            t_fwd.start();
            if (msc_lds) hipLaunchKernelGGL(post_forward_kernel<true>, dim3(grid), dim3(waves * 64), lds_f, st, pa);
            else hipLaunchKernelGGL(post_forward_kernel<false>, dim3(grid), dim3(waves * 64), lds_f, st, pa);
            MGTA_HIP_CHECK(hipGetLastError());
            t_fwd.end();
            MGTA_HIP_CHECK(hipMemsetAsync(d_head.p, 0, 64, st));
            t_bwd.start();
            if (msc_lds) hipLaunchKernelGGL(post_backward_kernel<true>, dim3(grid), dim3(waves * 64), lds_b, st, pa);
            else hipLaunchKernelGGL(post_backward_kernel<false>, dim3(grid), dim3(waves * 64), lds_b, st, pa);
            MGTA_HIP_CHECK(hipGetLastError());
            t_bwd.end();

            h_fwd.resize(count); h_bwd.resize(count);
            MGTA_HIP_CHECK(hipMemcpyAsync(h_fwd.data(), d_fwd.p, (size_t)count * 8, hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipMemcpyAsync(h_bwd.data(), d_bwd.p, (size_t)count * 8, hipMemcpyDeviceToHost, st));
            if (col_match) {
                h_cm.resize((size_t)count * M);
                MGTA_HIP_CHECK(hipMemcpyAsync(h_cm.data(), d_cm.p, (size_t)count * M * 8, hipMemcpyDeviceToHost, st));
            }
            if (col_insert) {
                h_ci.resize((size_t)count * M);
                MGTA_HIP_CHECK(hipMemcpyAsync(h_ci.data(), d_ci.p, (size_t)count * M * 8, hipMemcpyDeviceToHost, st));
            }
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
            ms_fwd += t_fwd.ms(); ms_bwd += t_bwd.ms();
            for (uint32_t k = 0; k < count; ++k) {
                const uint32_t idx = order[b0 + k];
                mgta_post_rec r;
                r.fwd = h_fwd[k]; r.bwd = h_bwd[k]; r.status = h_fwd[k] == -HUGE_VAL ? 1 : 0; r.pad = 0;
                recs[idx] = r;
                n_scored += r.status == 0;
                if (col_match) memcpy(col_match + (size_t)idx * M, h_cm.data() + (size_t)k * M, (size_t)M * 8);
                if (col_insert) memcpy(col_insert + (size_t)idx * M, h_ci.data() + (size_t)k * M, (size_t)M * 8);
            }
            n_cells += (int64_t)cells; ++n_batches;
            max_bpc = std::max<int64_t>(max_bpc, blocks_per_cu); min_wpb = std::min<int64_t>(min_wpb, waves);
            max_grid = std::max<int64_t>(max_grid, grid); max_lds = std::max<int64_t>(max_lds, (int64_t)lds_b);
            if (!msc_lds) all_msc_lds = 0;
            b0 = b1;
        }
        if (want_pp && n_letters) MGTA_HIP_CHECK(hipMemcpy(pp + offsets[0], d_pp.p, (size_t)n_letters * 8, hipMemcpyDeviceToHost));
        if (stats) {
            stats->n_seqs = n; stats->n_scored = n_scored; stats->n_unaligned = n - n_scored; stats->n_cells = n_cells; stats->n_batches = n_batches;
            stats->workgroups = max_grid; stats->waves_per_block = min_wpb; stats->blocks_per_cu = max_bpc; stats->lds_bytes = max_lds;
            stats->msc_in_lds = all_msc_lds; stats->peak_bytes = (int64_t)ctx->peak_bytes; stats->ms_forward = ms_fwd; stats->ms_backward = ms_bwd;
        }
        return (int)MGTA_OK;
    });
}

}  // extern "C"
