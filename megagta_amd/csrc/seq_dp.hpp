// seq_dp.hpp — what the dynamic-programming stages over protein sequences share on the HIP side (derep.hip, align.hip, posterior.hip,
// nearest.hip, chimera.hip; the host side without HIP is seq_jobs.hpp).
//
// Host.  PeakOfCall (peak_bytes per call), batch_cap (cells of a batch from the switch or the free memory), SeqStage (letters, offsets,
// order and queue head on the device) and the launch of a "one wave per queue item" kernel: blocks_per_cu_of sets the kernel's dynamic
// LDS and asks the runtime how many workgroups a CU holds, launch_waves sizes the grid by it and launches.
//
// Device.  The queue: waves take items from one atomic head (next_item).  The profile kernels (align_fill_kernel, post_forward_kernel,
// post_backward_kernel) carve their LDS as [alpha 128 B][boundary: waves x rows_lds x 2 doubles][msc (M+1)*A doubles when MSC_LDS]
// (profile_lds), hold the seven transitions out of a node in registers (load_node) and look an emission up by the residue's letter
// (emission).  The forward sweep of a sequence over the model in strips of 64 columns is profile_forward: lane l of a strip computes
// row i = t - l + 1 of its column at step t, X and Y move to lane l + 1 by a cross-lane move and across a strip edge through the
// boundary rows in LDS; the caller's cell says how candidates combine (maximum with choice bits, or log-sum-exp) and what a cell
// stores.  The pairwise kernels (nearest_sweep_kernel, chimera_sweep_kernel) share the sentinels, `sub` in LDS (stage_sub) and the DPP
// shift from_left.  The traceback bytes of a strip of width w lie at ((i - 1 + l) mod L) * w + l (tb_at), and trace_walk follows
// them back from (L, end column) for align_trace_kernel and nearest_trace_kernel.
#pragma once
#include "common.hpp"
#include "device_utils.hpp"
#include "seq_jobs.hpp"

namespace mgta {

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct PeakOfCall {                       // peak_bytes is this call's while it runs, the context's again on every way out
    uint64_t *peak, before;
    explicit PeakOfCall(mgta_ctx *ctx) : peak(&ctx->peak_bytes), before(ctx->peak_bytes) { *peak = ctx->live_bytes; }
    PeakOfCall(const PeakOfCall &) = delete;
    ~PeakOfCall() { *peak = std::max(*peak, before); }
};

// bytes the context may still take: the device's free memory, under the context's limit
inline uint64_t context_avail(mgta_ctx *ctx) {
    size_t free_b = 0, total_b = 0;
    MGTA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    uint64_t avail = free_b;
    if (ctx->mem_limit) avail = std::min<uint64_t>(avail, ctx->mem_limit > ctx->live_bytes ? ctx->mem_limit - ctx->live_bytes : 0);
    return avail;
}

// cells of a batch: the switch, else half of what the context may still take at cell_bytes per cell (the rest of a batch's buffers
// are far smaller).  avail_out (or NULL): those bytes, for a caller that checks its batches against them.
inline uint64_t batch_cap(mgta_ctx *ctx, uint64_t switch_cells, uint64_t cell_bytes, uint64_t *avail_out = nullptr) {
    const uint64_t avail = (!switch_cells || avail_out) ? context_avail(ctx) : 0;
    if (avail_out) *avail_out = avail;
    return switch_cells ? switch_cells : std::max<uint64_t>(avail / 2 / cell_bytes, 1);
}

// the letters of a call (16 bytes of pad), their offsets from the first letter, the order (or none) and the 64-byte queue head
struct SeqStage {
    DevBuf seqs, off, order, head;
    void upload(mgta_ctx *ctx, const char *letters, const uint64_t *offsets, const std::vector<uint64_t> &rel, const std::vector<uint32_t> *ord) {
        uint64_t *live = &ctx->live_bytes, *peak = &ctx->peak_bytes;
        const size_t n = rel.size() - 1;
        const uint64_t n_letters = rel[n];
        seqs.alloc(n_letters + 16, live, peak);
        off.alloc((n + 1) * 8, live, peak);
        if (ord) order.alloc(n * 4, live, peak);
        head.alloc(64, live, peak);
        if (n_letters) MGTA_HIP_CHECK(hipMemcpyAsync(seqs.p, letters + offsets[0], n_letters, hipMemcpyHostToDevice, ctx->stream));
        MGTA_HIP_CHECK(hipMemcpyAsync(off.p, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (ord) MGTA_HIP_CHECK(hipMemcpyAsync(order.p, ord->data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    void reset_head(hipStream_t st) { MGTA_HIP_CHECK(hipMemsetAsync(head.p, 0, 64, st)); }
};

// workgroups of `waves` waves and `lds` bytes a CU holds at once: what the runtime answers for the kernel's registers and this LDS
// (never assumed), one at least
template <class Args> int blocks_per_cu_of(void (*kernel)(Args), int waves, size_t lds) {
    MGTA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int bpc = 0;
    MGTA_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, kernel, waves * 64, lds));
    return std::max(1, bpc);
}

struct WaveLaunch { int blocks_per_cu; unsigned grid; };

// a kernel whose waves each take items from a queue: as many workgroups as the device holds at once, never more than the items need.
// blocks_per_cu = 0: asked here; a caller that launches two kernels on one grid asks for both first and passes the smaller.
template <class Args> WaveLaunch launch_waves(mgta_ctx *ctx, void (*kernel)(Args), const Args &a, int waves, size_t lds, uint64_t n_items, int blocks_per_cu = 0) {
    if (!blocks_per_cu) blocks_per_cu = blocks_per_cu_of(kernel, waves, lds);
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ctx->num_cus * (uint64_t)blocks_per_cu, (n_items + waves - 1) / waves));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(waves * 64), lds, ctx->stream, a);
    MGTA_HIP_CHECK(hipGetLastError());
    return WaveLaunch{blocks_per_cu, grid};
}

// ---- device: leaf pieces ------------------------------------------------------------------------------------------------------------
constexpr int kAlphaLdsBytes = 128;                 // residue letter -> emission column
constexpr int kSubLdsBytes = 27 * 32;               // sub[reference class][contig class], rows padded to 32
constexpr int32_t kUndef = -(1 << 30);              // "undefined" of the int32 recurrences (nearest.hip says why it is safe)
constexpr int32_t kDefinedFloor = -(1 << 29);       // every defined value lies above it, everything derived from kUndef below

__device__ __forceinline__ double neg_inf() { return -__builtin_huge_val(); }

// lane l takes v of lane l - 1, lane 0 keeps `first`: one v_mov_b32 with the DPP control wave_shr:1
__device__ __forceinline__ int32_t from_left(int32_t v, int32_t first) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xF, 0xF, false); }

// The next item of the queue, the same in every lane.  Every lane takes part and only lane 0 counts: no branch on the lane stands in
// front of the wave-wide read, so the compiler has nothing to thread round the loop (a leader-only branch here was split per lane, and
// lanes 1 .. 63 then read a zero).  Not walk.hpp's grp_next_chunk, which is leader-only on purpose.
__device__ __forceinline__ unsigned long long next_item(unsigned long long *head) {
    const unsigned long long k = atomicAdd(head, lane_id() == 0 ? 1ull : 0ull);
    return wave_uniform((uint64_t)k);
}

// sub [27 x 27, contig class major] into LDS as [reference class][contig class], 32 bytes per reference class; ends with a barrier
__device__ __forceinline__ void stage_sub(int8_t *s_sub, const int8_t *sub) {
    for (int c = threadIdx.x; c < kSubLdsBytes; c += blockDim.x) {
        const int cy = c >> 5, cx = c & 31;
        s_sub[c] = cx < 27 ? sub[cx * 27 + cy] : (int8_t)0;
    }
    __syncthreads();
}

// the LDS of a profile kernel, carved and staged; ends with a barrier.  msc is the staged copy when MSC_LDS, else tab itself; past
// points behind the last byte used, where a kernel may keep rows of its own.
struct ProfileLds {
    const int8_t *alpha;
    double *bound;               // this wave's rows_lds rows of two doubles
    const double *msc;
    unsigned char *past;
};
template <bool MSC_LDS>
__device__ __forceinline__ ProfileLds profile_lds(unsigned char *lds_raw, uint32_t rows_lds, const double *tab, const int8_t *alpha, size_t n_msc) {
    int8_t *s_alpha = reinterpret_cast<int8_t *>(lds_raw);
    const int n_waves = blockDim.x >> 6;
    double *s_msc = reinterpret_cast<double *>(lds_raw + kAlphaLdsBytes) + (size_t)n_waves * rows_lds * 2;
    for (int c = threadIdx.x; c < kAlphaLdsBytes; c += blockDim.x) s_alpha[c] = alpha[c];
    if (MSC_LDS)
        for (size_t c = threadIdx.x; c < n_msc; c += blockDim.x) s_msc[c] = tab[c];
    __syncthreads();
    return ProfileLds{s_alpha, reinterpret_cast<double *>(lds_raw + kAlphaLdsBytes) + (size_t)wave_id() * rows_lds * 2, MSC_LDS ? s_msc : tab,
                      reinterpret_cast<unsigned char *>(s_msc + (MSC_LDS ? n_msc : 0))};
}

// the seven transitions out of node j and its row of match emissions
struct Node {
    double mm, mi, md, im, ii, dm, dd;
    const double *mrow;
};
__device__ __forceinline__ Node load_node(const double *tsc, const double *msc, size_t M1, int A, int j) {
    return Node{tsc[0 * M1 + j], tsc[1 * M1 + j], tsc[2 * M1 + j], tsc[3 * M1 + j], tsc[4 * M1 + j], tsc[5 * M1 + j], tsc[6 * M1 + j], msc + (size_t)j * A};
}

// the match emission of letter c at a node: 0 for a letter the alphabet does not know
__device__ __forceinline__ double emission(const int8_t *s_alpha, const double *mrow, uint32_t c) {
    const int col = c < 127 ? (int)s_alpha[c] : -1;
    return col < 0 ? 0.0 : mrow[col];
}

// the traceback byte of cell (i, j) of an L x W table stored strip by strip
__device__ __forceinline__ uint8_t tb_at(const uint8_t *tb, int L, int W, int i, int j) {
    const int s = (j - 1) >> 6, l = (j - 1) & 63, w = min(64, W - 64 * s);
    return tb[(size_t)s * 64 * L + (size_t)((i - 1 + l) % L) * w + l];
}

// The walk back through the bytes of an L x W table from the match state of (L, jend): byte bits 0-1 the state the match candidate
// of the cell below-right came from (0 match, 1 insert, 2 delete), bit 2 delete from delete, bit 3 insert from insert.  on_match(i, j)
// at every match step; the path, if a slot of L + W bytes is given, is written backwards and then moved to the slot's front.
struct Walked { int from, n_match, n_insert, n_delete, plen; };
template <class OnMatch> __device__ __forceinline__ Walked trace_walk(const uint8_t *tb, int L, int W, int jend, char *slot, OnMatch on_match) {
    Walked r{0, 0, 0, 0, 0};
    const int slot_len = L + W;
    int i = L, j = jend, state = 0;
    // every step consumes a residue or a column: at most L + W of them
    for (int guard = 0; guard < L + W && i >= 1 && j >= 1 && j <= W; ++guard) {
        if (slot) slot[slot_len - 1 - r.plen] = state == 0 ? 'M' : state == 1 ? 'I' : 'D';
        ++r.plen;
        if (state == 0) {
            ++r.n_match;
            on_match(i, j);
            r.from = j;
            if (i == 1) break;
            if (j == 1) break;                                            // (not reached: the match state of (i > 1, 1) has no score)
            state = tb_at(tb, L, W, i - 1, j - 1) & 3;
            --i; --j;
        } else if (state == 1) {
            ++r.n_insert;
            if (i == 1) break;                                            // (not reached: row 1 has no insert state)
            state = (tb_at(tb, L, W, i - 1, j) & 8) ? 1 : 0;
            --i;
        } else {
            ++r.n_delete;
            if (j == 1) break;                                            // (not reached: column 1 has no delete state)
            state = (tb_at(tb, L, W, i, j - 1) & 4) ? 2 : 0;
            --j;
        }
    }
    if (slot)
        for (int p = 0; p < r.plen; ++p) slot[p] = slot[slot_len - r.plen + p];   // forwards: the source is never behind the target
    return r;
}

// ---- device: the forward sweep of the profile kernels -----------------------------------------------------------------------------
// One sequence x[0 .. L) over the M nodes, by one wave.  Written from the cell outwards: the lane of cell (i, j) computes
//     X = three(M + MM, I + IM, D + DM)   the candidate of the match state of (i+1, j+1)  (taken by lane l + 1 two steps later)
//     Y = two(M + MD, D + DD)             the delete state of (i, j+1)                    (taken by lane l + 1 at the next step)
//     I = two(M + MI, I + II)             the insert state of (i+1, j)                    (its own next step)
// with every + one IEEE add in this operand order, and nothing inside a row re-associated.  The last lane of a strip leaves X and Y per
// row in the wave's boundary rows, where lane 0 of the next strip finds them (one wave, LDS in program order: row i is read before the
// rows <= i - 62 are written, in place).  The cell:
//     strip(s)                      a strip starts (its stores go to s * 64 * L of the sequence's planes)
//     three(a, b, c, ch), two(a, b, ch, bit)   combine candidates; may note its choice in ch
//     store(at, v_m, v_i, ch)       a cell of the table: its match and insert values, its choices, at `at` of the strip
//     last_row(v_m, j)              the match value of (L, j)
template <class Cell>
__device__ __forceinline__ void profile_forward(const uint8_t *x, int L, int M, int A, const double *tsc, const ProfileLds &lds, Cell &cell) {
    const size_t M1 = (size_t)M + 1;
    const int lane = lane_id();
    const double NINF = neg_inf();
    const int n_strips = (M + 63) / 64;
    double *s_bound = lds.bound;
    for (int s = 0; s < n_strips; ++s) {
        const int w = min(64, M - 64 * s);
        const int j = 64 * s + lane + 1;
        const bool own = lane < w;
        const Node nd = load_node(tsc, lds.msc, M1, A, own ? j : M);      // (idle lanes read a valid node and store nothing)
        cell.strip(s);
        const bool last_strip = s == n_strips - 1;
        double x_out = NINF, y_out = NINF, x_held = NINF, v_i = NINF;
        const int n_steps = L + w - 1;
        int t_mod = 0;                                                    // t mod L
        for (int t = 0; t < n_steps; ++t) {
            const int i = t - lane + 1;                                   // this lane's row
            const bool valid = own && i >= 1 && i <= L;
            // what the left neighbour computed at the last step: X of its row i (for this lane's row i + 1), Y = the delete state of (i, j)
            double x_new = __shfl_up(x_out, 1, 64), v_d = __shfl_up(y_out, 1, 64);
            double x_use = x_held;
            if (lane == 0) {
                const int r = min(max(i, 1), L) - 1;                      // = i - 1: lane 0 is valid at every step t < L
                const bool have = s > 0 && i <= L;
                x_use = have ? s_bound[2 * r] : NINF;
                v_d = have ? s_bound[2 * r + 1] : NINF;
            }
            x_held = x_new;
            const int ii = min(max(i, 1), L);
            const double e = emission(lds.alpha, nd.mrow, x[ii - 1]);
            if (i <= 1) { x_use = 0.0; v_i = NINF; v_d = NINF; }          // row 1: B, no insert and no delete state
            const double v_m = x_use + e;
            uint32_t ch = 0;
            const double X = cell.three(v_m + nd.mm, v_i + nd.im, v_d + nd.dm, ch);
            double Y = cell.two(v_m + nd.md, v_d + nd.dd, ch, 4u);
            if (i <= 1) Y = NINF;                                         // row 1 has no delete state
            double I = cell.two(v_m + nd.mi, v_i + nd.ii, ch, 8u);
            if (j >= M) I = NINF;                                         // node M has no insert state
            x_out = X; y_out = Y;
            if (valid) {
                cell.store((size_t)t_mod * w + lane, v_m, v_i, ch);       // (i - 1 + lane) mod L = t mod L
                v_i = I;
                if (i == L) cell.last_row(v_m, j);
                if (!last_strip && lane == 63) {
                    s_bound[2 * (i - 1) + 1] = Y;                         // the delete state of (i, j + 1)
                    if (i < L) s_bound[2 * i] = X;                        // the candidate of the match state of (i + 1, j + 1)
                }
            }
            if (++t_mod == L) t_mod = 0;
        }
        wave_lds_fence();
    }
}

}  // namespace mgta
