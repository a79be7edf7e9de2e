// align.hip — protein sequences placed on the columns of a profile HMM (mgta_seqs_align): the place of `hmmalign` in the reference's
// bin/post_proc.sh:65.  The rule is this library's own (include/megagta_hip.h): Viterbi over match / insert / delete states, global in
// the sequence, local in the model, fp64, every + one IEEE add (-ffp-contract=off), first candidate wins a tie.
//
// Fill.  One wave owns a sequence; waves take sequences longest first from one atomic head.  The sweep over the model in strips of 64
// columns, anti-diagonal by anti-diagonal, is profile_forward (seq_dp.hpp); its cell here is ViterbiCell: X, Y and I are maxima, and
// the three choices are one byte per cell: bits 0-1 the state of (i, j) that X came from (0 M, 1 I, 2 D), bit 2 Y came from D, bit 3
// I came from I.  The traceback bytes of a strip of width w are stored at ((i - 1 + l) mod L) * w + l: a step's lanes write one run of
// bytes, and a sequence takes exactly L * M bytes.
//
// Trace.  One thread per sequence walks the bytes back from (L, lowest end column) (trace_walk, seq_dp.hpp) and writes the record, the
// column row and the path.
#include <algorithm>
#include <cmath>
#include <vector>

#include "seq_dp.hpp"

namespace mgta {
namespace {

constexpr int kAlignMaxLen = 4096;                 // residues of one sequence: 16 bytes of LDS per row of the wave that owns it
constexpr size_t kAlignLdsBudget = 80 * 1024;      // of a workgroup: two fit a CU

struct AlignArgs {
    const uint8_t *seqs;         // the letters of every sequence
    const uint64_t *off;         // [n + 1] into seqs
    const uint32_t *order;       // the batch: sequence numbers, longest first
    const uint64_t *cell_base;   // [count] where the traceback bytes of a batch item start
    uint32_t count;
    int M, A;
    const double *tab;           // [msc (M+1)*A][tsc 7*(M+1)] ...
    const int8_t *alpha;         // [128]
    uint8_t *tb;                 // traceback bytes of the batch
    double *score;               // [count]
    int32_t *jend;               // [count]
    uint32_t rows_lds;           // rows of boundary a wave has in LDS (>= the longest sequence of the batch)
    unsigned long long *head;
};

// the cell of profile_forward (seq_dp.hpp): the maximum, the first candidate wins a tie, the choices in one byte per cell
struct ViterbiCell {
    uint8_t *tb, *tbs;
    int L;
    double best;
    int best_j;
    __device__ __forceinline__ void strip(int s) { tbs = tb + (size_t)s * 64 * L; }
    __device__ __forceinline__ double three(double c0, double c1, double c2, uint32_t &ch) const {
        double X = c0;
        if (c1 > X) { X = c1; ch = 1; }
        if (c2 > X) { X = c2; ch = 2; }
        return X;
    }
    __device__ __forceinline__ double two(double d0, double d1, uint32_t &ch, uint32_t bit) const {
        double Y = d0;
        if (d1 > Y) { Y = d1; ch |= bit; }
        return Y;
    }
    __device__ __forceinline__ void store(size_t at, double, double, uint32_t ch) const { tbs[at] = (uint8_t)ch; }
    __device__ __forceinline__ void last_row(double v_m, int j) {
        if (v_m > best) { best = v_m; best_j = j; }                       // strips ascend: an equal score keeps the lower column
    }
};

template <bool MSC_LDS>
__global__ __launch_bounds__(256) void align_fill_kernel(AlignArgs a) {
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
            if (lane == 0) { a.score[k] = NINF; a.jend[k] = 0; }
            continue;
        }
        ViterbiCell cell{a.tb + a.cell_base[k], nullptr, L, NINF, 0x7FFFFFFF};
        profile_forward(a.seqs + o0, L, a.M, a.A, a.tab + n_msc, lds, cell);
        double best = cell.best;
        int best_j = cell.best_j;
        // the score and the lowest column that reaches it
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const double ob = __shfl_xor(best, d, 64);
            const int oj = __shfl_xor(best_j, d, 64);
            if (ob > best || (ob == best && oj < best_j)) { best = ob; best_j = oj; }
        }
        if (lane == 0) { a.score[k] = best; a.jend[k] = best_j; }
    }
}

struct TraceArgs {
    const uint8_t *seqs;
    const uint64_t *off;
    const uint32_t *order;
    const uint64_t *cell_base;
    const uint64_t *path_base;   // [count] where the path slot (L + M bytes) of a batch item starts
    uint32_t count;
    int M;
    const uint8_t *tb;
    const double *score;
    const int32_t *jend;
    mgta_align_rec *recs;        // [count]
    uint8_t *cols;               // [count * M], filled with '-' before the launch; or NULL
    char *path;                  // or NULL
    int32_t *path_len;           // [count] (with path)
};

__global__ __launch_bounds__(256) void align_trace_kernel(TraceArgs a) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.count) return;
    const uint32_t idx = a.order[k];
    const uint64_t o0 = a.off[idx];
    const int L = (int)(a.off[idx + 1] - o0), M = a.M;
    const double score = a.score[k];
    mgta_align_rec r;
    r.score = neg_inf(); r.status = 1; r.model_from = 0; r.model_to = 0; r.n_match = 0; r.n_insert = 0; r.n_delete = 0;
    int plen = 0;
    if (L > 0 && score > neg_inf()) {
        const uint8_t *x = a.seqs + o0;
        uint8_t *cols = a.cols ? a.cols + (size_t)k * M : nullptr;
        const Walked w = trace_walk(a.tb + a.cell_base[k], L, M, a.jend[k], a.path ? a.path + a.path_base[k] : nullptr, [&](int i, int j) {
            if (cols) {
                const uint8_t c = x[i - 1];
                cols[j - 1] = (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
            }
        });
        r.score = score; r.status = 0; r.model_to = a.jend[k]; r.model_from = w.from; r.n_match = w.n_match; r.n_insert = w.n_insert; r.n_delete = w.n_delete;
        plen = w.plen;
    }
    a.recs[k] = r;
    if (a.path_len) a.path_len[k] = plen;
}

}  // namespace
}  // namespace mgta

using namespace mgta;

extern "C" {

int mgta_ctx_set_align_batch(mgta_ctx *ctx, int64_t cells) {
    if (!ctx) { set_error("mgta_ctx_set_align_batch: ctx must not be NULL"); return MGTA_EINVAL; }
    if (cells < 0) { set_error("mgta_ctx_set_align_batch: cells = %lld must not be negative", (long long)cells); return MGTA_EINVAL; }
    ctx->align_batch_cells = (uint64_t)cells;
    return MGTA_OK;
}

int mgta_seqs_align(mgta_ctx *ctx, const mgta_hmm *hmm, const char *seqs, const uint64_t *offsets, int64_t n, mgta_align_rec *recs, uint8_t *cols, char *path,
                    int32_t *path_len, mgta_align_stats *stats) {
    if (!ctx) { set_error("mgta_seqs_align: ctx must not be NULL"); return MGTA_EINVAL; }
    if (!hmm) { set_error("mgta_seqs_align: the model must not be NULL"); return MGTA_EINVAL; }
    if (hmm->ctx != ctx) { set_error("mgta_seqs_align: the model belongs to another context"); return MGTA_EINVAL; }
    if (n < 0) { set_error("mgta_seqs_align: n = %lld must not be negative", (long long)n); return MGTA_EINVAL; }
    if (!check_seq_count("mgta_seqs_align", kSequences, n)) return MGTA_EINVAL;
    if (n > 0 && !offsets) { set_error("mgta_seqs_align: offsets must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && !recs) { set_error("mgta_seqs_align: recs must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && path && !path_len) { set_error("mgta_seqs_align: path_len must not be NULL when path is given"); return MGTA_EINVAL; }
    if (!check_seq_offsets("mgta_seqs_align", kSequences, offsets, n, kAlignMaxLen)) return MGTA_EINVAL;
    if (!check_seq_letters("mgta_seqs_align", kSequences, seqs, n > 0 ? offsets[n] - offsets[0] : 0)) return MGTA_EINVAL;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return MGTA_OK;
    return guarded("mgta_seqs_align", [&]() {
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        uint64_t *live = &ctx->live_bytes, *peak = &ctx->peak_bytes;
        const uint32_t nn = (uint32_t)n;
        const int M = hmm->M, A = hmm->A;
        const size_t msc_bytes = ((size_t)M + 1) * A * 8;

        // the letters and where they start, once; the sequences longest first
        const std::vector<uint64_t> rel = rel_offsets(offsets, n);
        const std::vector<uint32_t> order = longest_first(rel);
        const auto len_of = [&](uint32_t k) { return rel[order[k] + 1] - rel[order[k]]; };
        SeqStage dev;
        dev.upload(ctx, seqs, offsets, rel, &order);
        const uint64_t cap = batch_cap(ctx, ctx->align_batch_cells, 1);   // the traceback is one byte per cell

        Timer t_fill(st), t_trace(st);
        double ms_fill = 0, ms_trace = 0;
        int64_t n_batches = 0, n_aligned = 0, n_cells = 0, max_bpc = 0, min_wpb = 4, max_grid = 0, max_lds = 0, all_msc_lds = 1;
        std::vector<uint64_t> cell_base, path_base;
        std::vector<mgta_align_rec> h_recs;
        std::vector<uint8_t> h_cols;
        std::vector<char> h_path;
        std::vector<int32_t> h_plen;
        for (uint32_t b0 = 0; b0 < nn;) {
            uint64_t cells = 0, path_bytes = 0;
            const uint32_t b1 = cut_cells(b0, nn, cap, len_of, [&](uint32_t) { return (uint64_t)M; }, cell_base, &path_base, &cells, &path_bytes);
            const uint32_t count = b1 - b0;
            const uint32_t rows_lds = std::max(1u, (uint32_t)len_of(b0));
            const int waves = waves_that_fit(rows_lds, 16, kAlphaLdsBytes, kAlignLdsBudget);
            size_t lds = kAlphaLdsBytes + (size_t)waves * rows_lds * 16;
            const bool msc_lds = lds + msc_bytes <= kAlignLdsBudget;
            if (msc_lds) lds += msc_bytes;

            DevBuf d_tb, d_cbase, d_pbase, d_score, d_jend, d_recs, d_cols, d_path, d_plen;
            d_tb.alloc(cells + 16, live, peak);
            d_cbase.alloc((size_t)count * 8, live, peak);
            d_score.alloc((size_t)count * 8, live, peak);
            d_jend.alloc((size_t)count * 4, live, peak);
            d_recs.alloc((size_t)count * sizeof(mgta_align_rec), live, peak);
            MGTA_HIP_CHECK(hipMemcpyAsync(d_cbase.p, cell_base.data(), (size_t)count * 8, hipMemcpyHostToDevice, st));
            if (cols) {
                d_cols.alloc((size_t)count * M, live, peak);
                MGTA_HIP_CHECK(hipMemsetAsync(d_cols.p, '-', (size_t)count * M, st));
            }
            if (path) {
                d_pbase.alloc((size_t)count * 8, live, peak);
                d_path.alloc(path_bytes, live, peak);
                d_plen.alloc((size_t)count * 4, live, peak);
                MGTA_HIP_CHECK(hipMemcpyAsync(d_pbase.p, path_base.data(), (size_t)count * 8, hipMemcpyHostToDevice, st));
            }
            dev.reset_head(st);

            AlignArgs fa;
            fa.seqs = dev.seqs.as<uint8_t>(); fa.off = dev.off.as<uint64_t>(); fa.order = dev.order.as<uint32_t>() + b0; fa.cell_base = d_cbase.as<uint64_t>();
            fa.count = count; fa.M = M; fa.A = A; fa.tab = hmm->tab.as<double>(); fa.alpha = hmm->d_alpha.as<int8_t>(); fa.tb = d_tb.as<uint8_t>();
            fa.score = d_score.as<double>(); fa.jend = d_jend.as<int32_t>(); fa.rows_lds = rows_lds; fa.head = dev.head.as<unsigned long long>();
            const auto fill = msc_lds ? align_fill_kernel<true> : align_fill_kernel<false>;
            const int blocks_per_cu = blocks_per_cu_of(fill, waves, lds);
            t_fill.start();
            const unsigned grid = launch_waves(ctx, fill, fa, waves, lds, count, blocks_per_cu).grid;
            t_fill.end();

            TraceArgs ta;
            ta.seqs = fa.seqs; ta.off = fa.off; ta.order = fa.order; ta.cell_base = fa.cell_base; ta.path_base = d_pbase.as<uint64_t>(); ta.count = count; ta.M = M;
            ta.tb = fa.tb; ta.score = fa.score; ta.jend = fa.jend; ta.recs = d_recs.as<mgta_align_rec>(); ta.cols = cols ? d_cols.as<uint8_t>() : nullptr;
            ta.path = path ? d_path.as<char>() : nullptr; ta.path_len = path ? d_plen.as<int32_t>() : nullptr;
            t_trace.start();
            hipLaunchKernelGGL(align_trace_kernel, dim3((count + 255) / 256), dim3(256), 0, st, ta);
            MGTA_HIP_CHECK(hipGetLastError());
            t_trace.end();

            h_recs.resize(count);
            MGTA_HIP_CHECK(hipMemcpyAsync(h_recs.data(), d_recs.p, (size_t)count * sizeof(mgta_align_rec), hipMemcpyDeviceToHost, st));
            if (cols) {
                h_cols.resize((size_t)count * M);
                MGTA_HIP_CHECK(hipMemcpyAsync(h_cols.data(), d_cols.p, (size_t)count * M, hipMemcpyDeviceToHost, st));
            }
            if (path) {
                h_path.resize(path_bytes);
                h_plen.resize(count);
                MGTA_HIP_CHECK(hipMemcpyAsync(h_path.data(), d_path.p, path_bytes, hipMemcpyDeviceToHost, st));
                MGTA_HIP_CHECK(hipMemcpyAsync(h_plen.data(), d_plen.p, (size_t)count * 4, hipMemcpyDeviceToHost, st));
            }
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
            ms_fill += t_fill.ms(); ms_trace += t_trace.ms();
            for (uint32_t k = 0; k < count; ++k) {
                const uint32_t idx = order[b0 + k];
                recs[idx] = h_recs[k];
                n_aligned += h_recs[k].status == 0;
                if (cols) memcpy(cols + (size_t)idx * M, h_cols.data() + (size_t)k * M, (size_t)M);
                if (path) {
                    path_len[idx] = h_plen[k];
                    memcpy(path + offsets[idx] + (uint64_t)idx * M, h_path.data() + path_base[k], (size_t)h_plen[k]);
                }
            }
            n_cells += (int64_t)cells; ++n_batches;
            max_bpc = std::max<int64_t>(max_bpc, blocks_per_cu); min_wpb = std::min<int64_t>(min_wpb, waves);
            max_grid = std::max<int64_t>(max_grid, grid); max_lds = std::max<int64_t>(max_lds, (int64_t)lds);
            if (!msc_lds) all_msc_lds = 0;
            b0 = b1;
        }
        if (stats) {
            stats->n_seqs = n; stats->n_aligned = n_aligned; stats->n_unaligned = n - n_aligned; stats->n_cells = n_cells; stats->n_batches = n_batches;
            stats->blocks_per_cu = max_bpc; stats->waves_per_block = min_wpb; stats->grid_blocks = max_grid; stats->lds_bytes = max_lds;
            stats->msc_in_lds = all_msc_lds; stats->ms_fill = ms_fill; stats->ms_trace = ms_trace;
        }
        return (int)MGTA_OK;
    });
}

}  // extern "C"
