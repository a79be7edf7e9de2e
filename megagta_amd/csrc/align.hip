// align.hip — protein sequences placed on the columns of a profile HMM (mgta_seqs_align): the place of `hmmalign` in the reference's
// bin/post_proc.sh:65.  The rule is this library's own (include/megagta_hip.h): Viterbi over match / insert / delete states, global in
// the sequence, local in the model, fp64, every + one IEEE add (-ffp-contract=off), first candidate wins a tie.
//
// Fill.  One wave owns a sequence; waves take sequences longest first from one atomic head.  Lanes own model columns, 64 at a time
// (a strip); at step t of a strip lane l computes row i = t - l + 1 of its column j, so the cells of one anti-diagonal are computed
// together and nothing inside a row is re-associated.  The recurrence is written from the cell outwards: the lane of cell (i, j) holds
// the seven transitions out of node j in registers and computes what its neighbours need,
//     X = max(VM + MM, VI + IM, VD + DM)   the candidate of VM[i+1][j+1]  (taken by lane l + 1 two steps later)
//     Y = max(VM + MD, VD + DD)            VD[i][j+1]                     (taken by lane l + 1 at the next step)
//     I = max(VM + MI, VI + II)            VI[i+1][j]                     (its own next step)
// and the three choices, one byte per cell: bits 0-1 the state of (i, j) that X came from (0 M, 1 I, 2 D), bit 2 Y came from D, bit 3
// I came from I.  X and Y move to lane l + 1 by a cross-lane move; the last lane of a strip leaves them per row in LDS, where lane 0 of
// the next strip finds them (one wave, LDS in program order: row i is read before the rows <= i - 62 are written, in place).
// The traceback bytes of a strip of width w are stored at ((i - 1 + l) mod L) * w + l: a step's lanes write one run of bytes, and a
// sequence takes exactly L * M bytes.
//
// Trace.  One thread per sequence walks the bytes back from (L, lowest end column) and writes the record, the column row and the path.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "device_utils.hpp"

namespace mgta {
namespace {

constexpr int kAlignMaxLen = 4096;                 // residues of one sequence: 16 bytes of LDS per row of the wave that owns it
constexpr size_t kAlignLdsBudget = 80 * 1024;      // of a workgroup: two fit a CU
constexpr int kAlignAlphaBytes = 128;

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

__device__ __forceinline__ double neg_inf() { return -__builtin_huge_val(); }

template <bool MSC_LDS>
__global__ __launch_bounds__(256) void align_fill_kernel(AlignArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    // [alpha 128 B][boundary: waves x rows_lds x (X, Y)][msc (M+1)*A doubles when MSC_LDS]
    int8_t *s_alpha = reinterpret_cast<int8_t *>(lds_raw);
    const int n_waves = blockDim.x >> 6;
    double *s_bound = reinterpret_cast<double *>(lds_raw + kAlignAlphaBytes) + (size_t)wave_id() * a.rows_lds * 2;
    double *s_msc = reinterpret_cast<double *>(lds_raw + kAlignAlphaBytes) + (size_t)n_waves * a.rows_lds * 2;
    const int M = a.M, A = a.A;
    const size_t M1 = (size_t)M + 1;
    for (int c = threadIdx.x; c < kAlignAlphaBytes; c += blockDim.x) s_alpha[c] = a.alpha[c];
    if (MSC_LDS)
        for (size_t c = threadIdx.x; c < M1 * A; c += blockDim.x) s_msc[c] = a.tab[c];
    __syncthreads();
    const double *msc = MSC_LDS ? s_msc : a.tab;
    const double *tsc = a.tab + M1 * A;
    const int lane = lane_id();
    const double NINF = neg_inf();
    const int n_strips = (M + 63) / 64;

    for (;;) {
        // every lane takes part and only lane 0 counts: no branch on the lane stands in front of the wave-wide read, so the compiler
        // has nothing to thread round the loop (a leader-only branch here was split per lane, and lanes 1 .. 63 then read a zero)
        unsigned long long k = atomicAdd(a.head, lane == 0 ? 1ull : 0ull);
        k = wave_uniform((uint64_t)k);
        if (k >= a.count) break;
        const uint32_t idx = a.order[k];
        const uint64_t o0 = a.off[idx];
        const int L = (int)(a.off[idx + 1] - o0);
        if (L == 0) {
            if (lane == 0) { a.score[k] = NINF; a.jend[k] = 0; }
            continue;
        }
        const uint8_t *x = a.seqs + o0;
        uint8_t *tb = a.tb + a.cell_base[k];
        double best = NINF;
        int best_j = 0x7FFFFFFF;
        for (int s = 0; s < n_strips; ++s) {
            const int w = min(64, M - 64 * s);
            const int j = 64 * s + lane + 1;
            const bool own = lane < w;
            const int jc = own ? j : M;                                   // (idle lanes read a valid node and store nothing)
            const double tMM = tsc[0 * M1 + jc], tMI = tsc[1 * M1 + jc], tMD = tsc[2 * M1 + jc], tIM = tsc[3 * M1 + jc], tII = tsc[4 * M1 + jc],
                         tDM = tsc[5 * M1 + jc], tDD = tsc[6 * M1 + jc];
            const double *mrow = msc + (size_t)jc * A;
            uint8_t *tbs = tb + (size_t)s * 64 * L;
            const bool last_strip = s == n_strips - 1;
            double x_out = NINF, y_out = NINF, x_held = NINF, v_i = NINF;
            const int n_steps = L + w - 1;
            int t_mod = 0;                                                // t mod L
            for (int t = 0; t < n_steps; ++t) {
                const int i = t - lane + 1;                               // this lane's row
                const bool valid = own && i >= 1 && i <= L;
                // what the left neighbour computed at the last step: X of its row i (for this lane's row i + 1), Y = VD[i][j]
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
                if (i <= 1) { x_use = 0.0; v_i = NINF; v_d = NINF; }      // row 1: B, no insert and no delete state
                const double v_m = x_use + e;
                const double c0 = v_m + tMM, c1 = v_i + tIM, c2 = v_d + tDM;
                double X = c0;
                uint32_t ch = 0;
                if (c1 > X) { X = c1; ch = 1; }
                if (c2 > X) { X = c2; ch = 2; }
                const double d0 = v_m + tMD, d1 = v_d + tDD;
                double Y = d0;
                if (d1 > Y) { Y = d1; ch |= 4; }
                if (i <= 1) Y = NINF;                                     // VD[1][.] does not exist
                const double i0 = v_m + tMI, i1 = v_i + tII;
                double I = i0;
                if (i1 > I) { I = i1; ch |= 8; }
                if (j >= M) I = NINF;                                     // node M has no insert state
                x_out = X; y_out = Y;
                if (valid) {
                    v_i = I;
                    tbs[(size_t)t_mod * w + lane] = (uint8_t)ch;           // (i - 1 + lane) mod L = t mod L
                    if (i == L && v_m > best) { best = v_m; best_j = j; }  // strips ascend: an equal score keeps the lower column
                    if (!last_strip && lane == 63) {
                        s_bound[2 * (i - 1) + 1] = Y;                     // VD[i][j + 1]
                        if (i < L) s_bound[2 * i] = X;                    // the candidate of VM[i + 1][j + 1]
                    }
                }
                if (++t_mod == L) t_mod = 0;
            }
            wave_lds_fence();
        }
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

__device__ __forceinline__ uint8_t tb_at(const uint8_t *tb, int L, int M, int i, int j) {
    const int s = (j - 1) >> 6, l = (j - 1) & 63, w = min(64, M - 64 * s);
    return tb[(size_t)s * 64 * L + (size_t)((i - 1 + l) % L) * w + l];
}

__global__ __launch_bounds__(256) void align_trace_kernel(TraceArgs a) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.count) return;
    const uint32_t idx = a.order[k];
    const uint64_t o0 = a.off[idx];
    const int L = (int)(a.off[idx + 1] - o0), M = a.M;
    const double score = a.score[k];
    mgta_align_rec r;
    r.score = -__builtin_huge_val(); r.status = 1; r.model_from = 0; r.model_to = 0; r.n_match = 0; r.n_insert = 0; r.n_delete = 0;
    int plen = 0;
    if (L > 0 && score > -__builtin_huge_val()) {
        const uint8_t *x = a.seqs + o0;
        const uint8_t *tb = a.tb + a.cell_base[k];
        uint8_t *cols = a.cols ? a.cols + (size_t)k * M : nullptr;
        char *slot = a.path ? a.path + a.path_base[k] : nullptr;
        const int slot_len = L + M;
        int i = L, j = a.jend[k], state = 0;
        r.score = score; r.status = 0; r.model_to = j;
        // every step consumes a residue or a column: at most L + M of them
        for (int guard = 0; guard < L + M && i >= 1 && j >= 1 && j <= M; ++guard) {
            if (slot) slot[slot_len - 1 - plen] = state == 0 ? 'M' : state == 1 ? 'I' : 'D';
            ++plen;
            if (state == 0) {
                ++r.n_match;
                if (cols) {
                    const uint8_t c = x[i - 1];
                    cols[j - 1] = (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
                }
                r.model_from = j;
                if (i == 1) break;
                if (j == 1) break;                                        // (not reached: VM[i > 1][1] is -inf)
                state = tb_at(tb, L, M, i - 1, j - 1) & 3;
                --i; --j;
            } else if (state == 1) {
                ++r.n_insert;
                if (i == 1) break;                                        // (not reached: VI[1][.] is -inf)
                state = (tb_at(tb, L, M, i - 1, j) & 8) ? 1 : 0;
                --i;
            } else {
                ++r.n_delete;
                if (j == 1) break;                                        // (not reached: VD[.][1] is -inf)
                state = (tb_at(tb, L, M, i, j - 1) & 4) ? 2 : 0;
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
    if (n >= (1ll << 31)) { set_error("mgta_seqs_align: n = %lld (the limit is n < 2^31 sequences)", (long long)n); return MGTA_EINVAL; }
    if (n > 0 && !offsets) { set_error("mgta_seqs_align: offsets must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && !recs) { set_error("mgta_seqs_align: recs must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && path && !path_len) { set_error("mgta_seqs_align: path_len must not be NULL when path is given"); return MGTA_EINVAL; }
    for (int64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) { set_error("mgta_seqs_align: sequence %lld: offsets must ascend", (long long)i); return MGTA_EINVAL; }
        if (offsets[i + 1] - offsets[i] > (uint64_t)kAlignMaxLen) {
            set_error("mgta_seqs_align: sequence %lld holds %llu residues (the limit is %d residues per sequence)", (long long)i,
                      (unsigned long long)(offsets[i + 1] - offsets[i]), kAlignMaxLen);
            return MGTA_EINVAL;
        }
    }
    if (n > 0 && offsets[n] > offsets[0] && !seqs) { set_error("mgta_seqs_align: seqs must not be NULL"); return MGTA_EINVAL; }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return MGTA_OK;
    return guarded("mgta_seqs_align", [&]() {
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        uint64_t *live = &ctx->live_bytes, *peak = &ctx->peak_bytes;
        const uint32_t nn = (uint32_t)n;
        const int M = hmm->M, A = hmm->A;
        const uint64_t n_letters = offsets[n] - offsets[0];
        const size_t msc_bytes = ((size_t)M + 1) * A * 8;

        // the letters and where they start, once; the sequences longest first
        std::vector<uint64_t> rel((size_t)nn + 1);
        for (uint32_t i = 0; i <= nn; ++i) rel[i] = offsets[i] - offsets[0];
        std::vector<uint32_t> order(nn);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return rel[x + 1] - rel[x] > rel[y + 1] - rel[y]; });
        DevBuf d_seqs, d_off, d_order, d_head;
        d_seqs.alloc(n_letters + 16, live, peak);
        d_off.alloc((size_t)(nn + 1) * 8, live, peak);
        d_order.alloc((size_t)nn * 4, live, peak);
        d_head.alloc(64, live, peak);
        if (n_letters) MGTA_HIP_CHECK(hipMemcpyAsync(d_seqs.p, seqs + offsets[0], n_letters, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_off.p, rel.data(), (size_t)(nn + 1) * 8, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_order.p, order.data(), (size_t)nn * 4, hipMemcpyHostToDevice, st));

        // cells of a batch: the switch, or half of what the context may still take (the traceback is one byte per cell; the rest of
        // a batch's buffers are far smaller)
        uint64_t cap = ctx->align_batch_cells;
        if (!cap) {
            size_t free_b = 0, total_b = 0;
            MGTA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            uint64_t avail = free_b;
            if (ctx->mem_limit) avail = std::min<uint64_t>(avail, ctx->mem_limit > ctx->live_bytes ? ctx->mem_limit - ctx->live_bytes : 0);
            cap = std::max<uint64_t>(avail / 2, 1);
        }

        Timer t_fill(st), t_trace(st);
        double ms_fill = 0, ms_trace = 0;
        int64_t n_batches = 0, n_aligned = 0, n_cells = 0, max_bpc = 0, min_wpb = 4, max_grid = 0, max_lds = 0, all_msc_lds = 1;
        std::vector<uint64_t> cell_base, path_base;
        std::vector<mgta_align_rec> h_recs;
        std::vector<uint8_t> h_cols;
        std::vector<char> h_path;
        std::vector<int32_t> h_plen;
        for (uint32_t b0 = 0; b0 < nn;) {
            // the batch [b0, b1): at least one sequence
            uint32_t b1 = b0;
            uint64_t cells = 0, path_bytes = 0;
            cell_base.clear(); path_base.clear();
            while (b1 < nn) {
                const uint64_t L = rel[order[b1] + 1] - rel[order[b1]];
                if (b1 > b0 && cells + L * (uint64_t)M > cap) break;
                cell_base.push_back(cells); path_base.push_back(path_bytes);
                cells += L * (uint64_t)M; path_bytes += L + (uint64_t)M;
                ++b1;
            }
            const uint32_t count = b1 - b0;
            const uint32_t l_max = (uint32_t)(rel[order[b0] + 1] - rel[order[b0]]);
            const uint32_t rows_lds = std::max(1u, l_max);
            int waves = 4;
            while (waves > 1 && kAlignAlphaBytes + (size_t)waves * rows_lds * 16 > kAlignLdsBudget) waves >>= 1;
            size_t lds = kAlignAlphaBytes + (size_t)waves * rows_lds * 16;
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
            MGTA_HIP_CHECK(hipMemsetAsync(d_head.p, 0, 64, st));

            AlignArgs fa;
            fa.seqs = d_seqs.as<uint8_t>(); fa.off = d_off.as<uint64_t>(); fa.order = d_order.as<uint32_t>() + b0; fa.cell_base = d_cbase.as<uint64_t>();
            fa.count = count; fa.M = M; fa.A = A; fa.tab = hmm->tab.as<double>(); fa.alpha = hmm->d_alpha.as<int8_t>(); fa.tb = d_tb.as<uint8_t>();
            fa.score = d_score.as<double>(); fa.jend = d_jend.as<int32_t>(); fa.rows_lds = rows_lds; fa.head = d_head.as<unsigned long long>();
            // workgroups a CU holds at once: what the runtime answers for these registers and this LDS (never assumed)
            const void *fn = msc_lds ? reinterpret_cast<const void *>(align_fill_kernel<true>) : reinterpret_cast<const void *>(align_fill_kernel<false>);
            MGTA_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            int blocks_per_cu = 0;
            if (msc_lds) MGTA_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, align_fill_kernel<true>, waves * 64, lds));
            else MGTA_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, align_fill_kernel<false>, waves * 64, lds));
            blocks_per_cu = std::max(1, blocks_per_cu);
            const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)ctx->num_cus * (uint64_t)blocks_per_cu, ((uint64_t)count + waves - 1) / waves);
            t_fill.start();
            if (msc_lds) hipLaunchKernelGGL(align_fill_kernel<true>, dim3(grid), dim3(waves * 64), lds, st, fa);
            else hipLaunchKernelGGL(align_fill_kernel<false>, dim3(grid), dim3(waves * 64), lds, st, fa);
            MGTA_HIP_CHECK(hipGetLastError());
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
