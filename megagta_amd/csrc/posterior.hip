// posterior.hip — Forward score and per-residue posteriors of protein sequences on a profile HMM (mgta_seqs_posterior): how far the
// placement of mgta_seqs_align can be trusted.  The rule is this library's own (include/megagta_hip.h): mgta_seqs_align's cells with
// every max replaced by log-sum-exp, fp64, a backward sweep over the same cells, posterior = exp(forward + backward - F).
//
// Forward.  align_fill_kernel's scheme on the same sweep (profile_forward, seq_dp.hpp) with ForwardCell: X, Y and I are log-sum-exps,
// and FM and FI of every cell are stored, two planes of doubles, a strip of width w at ((i - 1 + l) mod L) * w + l: a step's lanes
// write one run.  FD is not kept.
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
#include <vector>

#include "seq_dp.hpp"

namespace mgta {
namespace {

constexpr int kPostMaxLen = 4096;                  // residues of one sequence: 20 bytes of LDS per row of the wave that owns it
constexpr size_t kPostLdsBudget = 82 * 1024;       // of a workgroup: the longest sequence alone (4096 * 20 + 128 bytes) still fits
constexpr uint64_t kPostCellBytes = 16;            // FM and FI of a cell

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

// the cell of profile_forward (seq_dp.hpp): log-sum-exp, FM and FI of every cell stored in two planes of doubles
struct ForwardCell {
    double *pm, *pi, *pms, *pis;
    int L;
    double f_acc;                                                         // lse of this lane's FM[L][.] over the strips
    __device__ __forceinline__ void strip(int s) { pms = pm + (size_t)s * 64 * L; pis = pi + (size_t)s * 64 * L; }
    __device__ __forceinline__ double three(double a, double b, double c, uint32_t &) const { return lse3(a, b, c); }
    __device__ __forceinline__ double two(double a, double b, uint32_t &, uint32_t) const { return lse2(a, b); }
    __device__ __forceinline__ void store(size_t at, double v_m, double v_i, uint32_t) const { pms[at] = v_m; pis[at] = v_i; }
    __device__ __forceinline__ void last_row(double v_m, int) { f_acc = lse2(f_acc, v_m); }
};

template <bool MSC_LDS>
__global__ __launch_bounds__(256) void post_forward_kernel(PostArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const size_t n_msc = ((size_t)a.M + 1) * a.A;
    const ProfileLds lds = profile_lds<MSC_LDS>(lds_raw, a.rows_lds, a.tab, a.alpha, n_msc);
    const int lane = lane_id();
    const double NINF = neg_inf();

    for (;;) {
        const unsigned long long k = next_item(a.head);
        if (k >= a.count) break;
        const uint32_t idx = a.order[k];
        const uint64_t o0 = a.off[idx];
        const int L = (int)(a.off[idx + 1] - o0);
        if (L == 0) {
            if (lane == 0) a.fwd[k] = NINF;
            continue;
        }
        ForwardCell cell{a.fm + a.cell_base[k], a.fi + a.cell_base[k], nullptr, nullptr, L, NINF};
        profile_forward(a.seqs + o0, L, a.M, a.A, a.tab + n_msc, lds, cell);
        const double F = wave_lse(cell.f_acc);
        if (lane == 0) a.fwd[k] = F;
    }
}

template <bool MSC_LDS>
__global__ __launch_bounds__(256) void post_backward_kernel(PostArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    // profile_lds' carve-up with (N, BD) in the boundary rows, and behind it [labels: waves x rows_lds x int32]
    const int M = a.M, A = a.A;
    const size_t M1 = (size_t)M + 1;
    const ProfileLds lds = profile_lds<MSC_LDS>(lds_raw, a.rows_lds, a.tab, a.alpha, M1 * A);
    double *s_bound = lds.bound;
    int32_t *s_lab = reinterpret_cast<int32_t *>(lds.past) + (size_t)wave_id() * a.rows_lds;
    const double *tsc = a.tab + M1 * A;
    const int lane = lane_id();
    const double NINF = neg_inf();
    const int n_strips = (M + 63) / 64;
    const bool want_pp = a.labels != nullptr && a.pp != nullptr;

    for (;;) {
        const unsigned long long k = next_item(a.head);
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
            const Node nd = load_node(tsc, lds.msc, M1, A, own ? j : M);
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
                const double e = emission(lds.alpha, nd.mrow, x[ii - 1]);
                double BM = lse3(nd.mm + n_use, nd.mi + b_i, nd.md + b_d);      // (b_i is -inf at j = M, b_d at j = M and from row 1)
                double BI = lse2(nd.im + n_use, nd.ii + b_i);
                double BD = lse2(nd.dm + n_use, nd.dd + b_d);
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
    if (!check_seq_count("mgta_seqs_posterior", kSequences, n)) return MGTA_EINVAL;
    if (n > 0 && !offsets) { set_error("mgta_seqs_posterior: offsets must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && !recs) { set_error("mgta_seqs_posterior: recs must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && pp && !labels) { set_error("mgta_seqs_posterior: labels must not be NULL when pp is given"); return MGTA_EINVAL; }
    if (!check_seq_offsets("mgta_seqs_posterior", kSequences, offsets, n, kPostMaxLen)) return MGTA_EINVAL;
    if (!check_seq_letters("mgta_seqs_posterior", kSequences, seqs, n > 0 ? offsets[n] - offsets[0] : 0)) return MGTA_EINVAL;
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
        PeakOfCall peak_of_call(ctx);
        const uint32_t nn = (uint32_t)n;
        const int M = hmm->M, A = hmm->A;
        const uint64_t n_letters = offsets[n] - offsets[0];
        const size_t msc_bytes = ((size_t)M + 1) * A * 8;
        const bool want_pp = labels && pp;

        // the letters, the labels and where they start, once; the sequences longest first
        const std::vector<uint64_t> rel = rel_offsets(offsets, n);
        const std::vector<uint32_t> order = longest_first(rel);
        const auto len_of = [&](uint32_t k) { return rel[order[k] + 1] - rel[order[k]]; };
        SeqStage dev;
        dev.upload(ctx, seqs, offsets, rel, &order);
        DevBuf d_labels, d_pp;
        if (want_pp) {
            d_labels.alloc((size_t)n_letters * 4 + 16, live, peak);
            d_pp.alloc((size_t)n_letters * 8 + 16, live, peak);
            if (n_letters) MGTA_HIP_CHECK(hipMemcpyAsync(d_labels.p, labels + offsets[0], (size_t)n_letters * 4, hipMemcpyHostToDevice, st));
            MGTA_HIP_CHECK(hipMemsetAsync(d_pp.p, 0, (size_t)n_letters * 8 + 16, st));
        }

        uint64_t avail = 0;
        const uint64_t cap = batch_cap(ctx, ctx->posterior_batch_cells, kPostCellBytes, &avail);

        Timer t_fwd(st), t_bwd(st);
        double ms_fwd = 0, ms_bwd = 0;
        int64_t n_batches = 0, n_scored = 0, n_cells = 0, max_bpc = 0, min_wpb = 4, max_grid = 0, max_lds = 0, all_msc_lds = 1;
        std::vector<uint64_t> cell_base;
        std::vector<double> h_fwd, h_bwd, h_cm, h_ci;
        for (uint32_t b0 = 0; b0 < nn;) {
            uint64_t cells = 0;
            const uint32_t b1 = cut_cells(b0, nn, cap, len_of, [&](uint32_t) { return (uint64_t)M; }, cell_base, nullptr, &cells);
            const uint32_t count = b1 - b0;
            const uint64_t plane_bytes = cells * 8 + 16;
            if (2 * plane_bytes > avail) {                                // (one sequence alone may be more than the device has left)
                set_error("mgta_seqs_posterior: a batch of %llu cells needs %llu bytes of device memory and %llu are left", (unsigned long long)cells,
                          (unsigned long long)(2 * plane_bytes), (unsigned long long)avail);
                return (int)MGTA_ENOMEM;
            }
            const uint32_t rows_lds = std::max(1u, (uint32_t)len_of(b0));
            // one geometry for both kernels: the backward one needs 4 more bytes per row, for the labels
            const int waves = waves_that_fit(rows_lds, 20, kAlphaLdsBytes, kPostLdsBudget);
            size_t lds_f = kAlphaLdsBytes + (size_t)waves * rows_lds * 16, lds_b = kAlphaLdsBytes + (size_t)waves * rows_lds * 20;
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
            pa.seqs = dev.seqs.as<uint8_t>(); pa.off = dev.off.as<uint64_t>(); pa.order = dev.order.as<uint32_t>() + b0; pa.cell_base = d_cbase.as<uint64_t>();
            pa.count = count; pa.M = M; pa.A = A; pa.tab = hmm->tab.as<double>(); pa.alpha = hmm->d_alpha.as<int8_t>();
            pa.fm = d_fm.as<double>(); pa.fi = d_fi.as<double>(); pa.fwd = d_fwd.as<double>(); pa.bwd = d_bwd.as<double>();
            pa.labels = want_pp ? d_labels.as<int32_t>() : nullptr; pa.pp = want_pp ? d_pp.as<double>() : nullptr;
            pa.col_m = col_match ? d_cm.as<double>() : nullptr; pa.col_i = col_insert ? d_ci.as<double>() : nullptr;
            pa.rows_lds = rows_lds; pa.head = dev.head.as<unsigned long long>();
            // one grid for both kernels: the workgroups a CU holds of the one that needs more
            const auto forward = msc_lds ? post_forward_kernel<true> : post_forward_kernel<false>;
            const auto backward = msc_lds ? post_backward_kernel<true> : post_backward_kernel<false>;
            const int blocks_per_cu = std::min(blocks_per_cu_of(forward, waves, lds_f), blocks_per_cu_of(backward, waves, lds_b));
            dev.reset_head(st);
            t_fwd.start();
            const unsigned grid = launch_waves(ctx, forward, pa, waves, lds_f, count, blocks_per_cu).grid;
            t_fwd.end();
            dev.reset_head(st);
            t_bwd.start();
            launch_waves(ctx, backward, pa, waves, lds_b, count, blocks_per_cu);
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
