// sdbg_build.hip — reads -> succinct-de-Bruijn-graph edge stream on gfx950 (MI355X).
//
// Replaces, behind the C ABI of include/megagta_hip.h, the reference's CX1 stage-2 pipeline
//   s2_lv0_calc_bucket_size   cx1_read2sdbg_s2.cpp:252-315   (bucket census)
//   s2_lv1_fill_offset        cx1_read2sdbg_s2.cpp:475-584   (per-bucket item lists)
//   s2_lv2_extract_substr_    cx1_read2sdbg_s2.cpp:586-677   (key extraction, CopySubstring[RC] packed_reads.h:44-176)
//   lv2_cpu_radix_sort_st     lv2_cpu_sort.h:133-150         (ascending lexicographic sort of the W-word keys)
//   output_ + SdbgWriter::write  cx1_read2sdbg_s2.cpp:742-835, sdbg_multi_io.h:83-112 (edge records)
// with a device-resident design (no differential offset lists, no per-bucket CPU threads):
//
//   pass over a bucket range [b_lo,b_hi) that fits the memory budget (the analogue of CX1's lv1 loop)
//     1. items per workgroup: closed form when every bucket is wanted (2 (len - k) + 4 per read), else
//        item_scan<count>: one wave per read, one lane per (k+1)-mer position: funnel-shift the edge out of the 2-bit read
//        array, reverse-complement it in registers, count the <= 6 sort items of the position whose first 8 characters fall
//        into the range (one scan counts every range that is still ahead -- and, for up to 8 ranges whose sort plan can be told from
//        the attempt that was refused before, the digit of every item that the range's first global sort pass sorts on, per workgroup)
//     2. prefix sum of the per-workgroup counts
//     3. item_scan<write>   same scan, keys written (array-of-structs, W words) with wave-aggregated offsets, and next to every key
//        the byte the first global sort pass sorts on (the SIDE array, W <= 7); or, where step 1 counted that pass's digits and the
//        real plan is the one they were counted for, item_write_fused: the keys are ranked by the digit in LDS and leave as one run
//        per digit value at the offsets the counts give, so that pass neither reads nor moves them again (MGTA_SORT_FUSED)
//     4. sort: P <= 4 global LSD passes on the P leading key bytes (digit census per tile FROM THE SIDE BYTES, row scan, stable
//        LDS-staged scatter with wave-level match ranking and coalesced run writes, which leaves the next pass's side bytes behind:
//        the keys cross HBM once per pass for the scatter, not twice), then every segment of equal prefix is finished inside LDS:
//        one counting pass on (segment, next <= 8 bits) with LDS atomics, then every key ranks itself inside its short run of
//        equal leading bits by comparison (local_sort_kernel); tiles with long runs and segments that did not fit take LSD
//        passes in LDS (local_lsd_kernel), segments longer than a tile are split by their leading digits, one scatter per level,
//        until the pieces fit (segment_split_kernel)
//     5. edge emission: run descriptors (a, b, group head, bucket head) compacted by a chained scan across workgroups -- from one
//        byte per key position that the segment-local finish wrote while the sorted keys were still in LDS (local_sort_kernel's
//        epilogue; emit_info_range_kernel for the ranges the other finishers sorted; emit_compact_info_kernel, MGTA_EMIT_FUSED), or
//        where the sort left no such bytes in one more read of the keys (emit_compact_kernel) -> per run decision (W, last, tip,
//        multiplicity, $-suppression) -> order-preserving compaction of records, large multiplicities and tip labels + per-bucket
//        boundaries
//
// Everything is integer / byte work bound by HBM traffic; no MFMA.  Parity: bit-exact edge stream vs
// the oracle (tests/test_sdbg_build_gpu.py).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <type_traits>

#include "common.hpp"
#include "device_utils.hpp"
#include "scan.hpp"
#include "segment_split.hpp"

namespace mgta {

constexpr int kDollar = 4;   // kSentinelValue, cx1_read2sdbg.h:72

template <int W>
struct Key {
    uint32_t w[W];
};

// ---------------------------------------------------------------------------------------------
// multi-word helpers on big-endian 2-bit strings (x[0] holds the first 16 characters)
// ---------------------------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ void shl_bits(uint32_t (&x)[W], int s) {   // 0 <= s <= 32
    if (s == 0) return;
    if (s == 32) {
#pragma unroll
        for (int j = 0; j < W - 1; ++j) x[j] = x[j + 1];
        x[W - 1] = 0;
        return;
    }
#pragma unroll
    for (int j = 0; j < W; ++j) x[j] = (x[j] << s) | (j + 1 < W ? (x[j + 1] >> (32 - s)) : 0u);
}

template <int W>
__device__ __forceinline__ void keep_chars(uint32_t (&x)[W], int n) {   // keep the first n characters
#pragma unroll
    for (int j = 0; j < W; ++j) {
        int lo = j * 16;
        if (n <= lo) x[j] = 0;
        else if (n < lo + 16) x[j] &= ~0u << (32 - 2 * (n - lo));
    }
}

// key = characters [from, from+n) of `e` (n = k or k-1), zero padded, flags in the low 4 bits of the
// last word: (n == k) << 3 | prev     [cx1_read2sdbg_s2.cpp:613-671]
template <int W>
__device__ __forceinline__ Key<W> make_key(const uint32_t (&e)[W], int from, int n, int k, int prev) {
    uint32_t t[W];
#pragma unroll
    for (int j = 0; j < W; ++j) t[j] = e[j];
    shl_bits<W>(t, 2 * from);
    keep_chars<W>(t, n);
    t[W - 1] |= (uint32_t)(n == k) << 3;
    t[W - 1] |= (uint32_t)prev;
    Key<W> key;
#pragma unroll
    for (int j = 0; j < W; ++j) key.w[j] = t[j];
    return key;
}

__device__ __forceinline__ uint32_t rev_chars(uint32_t x) {   // reverse the 16 characters of a word
    x = __brev(x);
    return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
}

// ---------------------------------------------------------------------------------------------
// 1./3. read scan
// ---------------------------------------------------------------------------------------------
constexpr int kScanBlock = 256;            // 4 waves
constexpr int kReadsPerBlock = 64;

struct ScanArgs {
    const uint32_t *packed;
    uint64_t n_words;
    const uint64_t *start;
    uint64_t n_reads;
    int k;
    uint32_t b_lo, b_hi;                   // bucket range [b_lo, b_hi)
    uint32_t *block_count;                 // count mode: items per workgroup
    const uint64_t *block_base;            // write mode
    void *out;                             // Key<W>*
    unsigned long long *n_kmers;           // count mode, sum over reads of max(0, len - k)
    const unsigned long long *is_solid;    // stage-1 verdicts (bit num_k1_per_read*read + position), nullptr = every position solid
    int num_k1_per_read;
    uint64_t n_short;                      // reads >= n_short (assist sequences) are always solid (s2.cpp:276)
    unsigned long long *n_sentinel;        // closed-form writers, k+1 even: number of sentinel keys written (see item_write_closed_kernel)
    uint32_t multi_width, multi_n;         // count mode: multi_n > 0 counts multi_n consecutive bucket ranges of multi_width buckets from
                                           // b_lo in one scan: block_count[range * gridDim.x + workgroup]
    uint64_t multi_magic;                  // ceil(2^32 / multi_width) (the range of a bucket without a division per item)
    uint8_t *side;                         // write mode, optional: ((word 0 - side_bias) >> side_shift) & 255 of every key next to it (the
    int side_shift;                        // first global sort pass then counts these bytes instead of reading the keys back)
    uint32_t side_bias;
    int side_bits;                         // fused writer: width of that digit; above 8 the entries are uint16_t (SideEntry)
    // fused first sort pass (item_scan_kernel<W, false, true> counts, item_write_fused_kernel places): digit of a key =
    // ((word 0 - fz_bias) >> fz_shift) & 255, per range counted ahead in the count scan, entry 0 in the writer
    uint64_t *fz_hist;                     // count scan: [range][digit value][workgroup]; writer: its range's slice after the row scan
    const uint64_t *fz_totals;             // writer: keys of the pass per digit value
    uint64_t fz_n;                         // writer: keys of the pass (no store goes past them)
    uint32_t fz_bias[8];
    uint32_t fz_shift[8];
};
constexpr int kMaxCountRanges = 64;
constexpr int kMaxFusedRanges = 8;

// tile of workgroup b of n when workgroup b runs on XCD b % 8: contiguous eighths of the tiles per XCD
__device__ __forceinline__ uint32_t xcd_tile(uint32_t b, uint32_t n) {
    if (n < 64) return b;
    const uint32_t x = b & 7u, idx = b >> 3, q = n >> 3, r = n & 7u;
    return x * q + (x < r ? x : r) + idx;
}

// LDS of the fused key writer: the keys of a batch as they are generated, their order by digit value, and per digit value the
// row's place in the output.  The waves of a workgroup meet at a barrier every round and at six per batch, and only other
// workgroups on the CU fill those gaps, so the stage is small: 26 KB per workgroup = six workgroups per CU = batches of 1536 keys at
// W = 3.  Measured at 100 M reads, k = 44 (profiles/r07/build_fused/README.md; key generation of the three ranges per step): 52 KB 355 ms, 40 KB
// 295 ms, 30 KB 265 ms, 26 KB 242 ms, 22 KB (seven workgroups, batches of 1152 keys: runs of 4-5 keys per digit value) 251 ms.
constexpr int kFusedLdsKB = 26;
template <int W> struct FusedCfg {
    static constexpr int kWaveRound = 6 * 64;                                  // keys a round of one wave can yield at most
    static constexpr int kFit = (kFusedLdsKB * 1024 - 5 * 1024) / (4 * W + 2) / 128 * 128;
    static constexpr int kCap = kFit < kWaveRound ? kWaveRound : (kFit > 8192 ? 8192 : kFit);
};
template <int W> struct FusedShared {
    Key<W> stage[FusedCfg<W>::kCap];
    uint16_t perm[FusedCfg<W>::kCap];      // perm[i] = place in `stage` of the i-th key of the batch in digit order
    uint32_t cnt[256];                     // keys of the batch per digit value (counted as they are staged), then the rank cursor
    uint32_t pos[256];                     // first key of the digit value in the batch's digit order
    uint64_t next[256];                    // place in the output of the row's next key of the digit value
    uint32_t wave_tot[2][kScanBlock / 64]; // keys of the round per wave | "more rounds to come" << 31, double-buffered by round parity
    uint32_t scr[kScanBlock / 64];
    uint64_t s64[kScanBlock / 64 + 1];
};

// masks of the first n characters of a W-word string (keep_chars as W ANDs with wave-uniform operands)
template <int W>
__device__ __forceinline__ void keep_masks(int n, uint32_t (&m)[W]) {
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const int lo = j * 16;
        m[j] = n <= lo ? 0u : (n < lo + 16 ? ~0u << (32 - 2 * (n - lo)) : ~0u);
    }
}

// The kernel is bound by VALU issue in write mode (SQ counters at 100 M reads, k = 44: 227 vector instructions per 64 positions, a wave64
// instruction takes four cycles of a 16-lane SIMD) and by load latency in count mode (117), so the write path keeps everything
// wave-uniform out of the vector unit: character masks and the workgroup's slice of the output as scalars, no bounds checks on the read
// words where the workgroup's reads end well inside the array, no staging array for the items of a position.
//
// One body, three kernels.  CENSUS (count mode, <= 8 ranges ahead): every kept item also counts the digit its range's first global sort
// pass will sort on, per workgroup (= row of that pass's offset table).  FUSED (write mode): the keys do not go out in scan order but
// are ranked by that digit in LDS and leave as one run per digit value at the row's offsets (item_write_fused_kernel): the first
// pass of the sort is done when the keys are written.  Both read groups of reads in xcd_tile order, so that the table entries of
// neighbouring rows (one line per 16 rows of a digit value) are written and read through one L2.
template <int W, bool WRITE, bool CENSUS, bool FUSED>
__device__ __forceinline__ void item_scan_body(const ScanArgs &a) {
    static_assert(!(CENSUS && WRITE) && !(FUSED && !WRITE), "the census belongs to the count scan, the placing to the writer");
    static_assert(kScanBlock == 256, "fused writer: one thread per digit value");
    __shared__ uint32_t s_cursor;
    __shared__ uint32_t s_wave_cnt[kScanBlock / 64];
    __shared__ uint32_t s_range_cnt[kMaxCountRanges];
    __shared__ uint32_t s_fz_hist[CENSUS ? kMaxFusedRanges * 256 : 1];
    __shared__ uint32_t s_fz_bias[kMaxFusedRanges], s_fz_shift[kMaxFusedRanges];
    __shared__ std::conditional_t<FUSED, FusedShared<W>, uint32_t> fs;   // (no LDS unless FUSED)
    const int k = a.k;
    const int lane = lane_id(), wv = wave_id();
    __shared__ uint64_t s_start[kReadsPerBlock + 1];                  // one coalesced load instead of two dependent ones per read
    const bool multi = !WRITE && a.multi_n > 0;
    const uint64_t multi_magic = a.multi_magic;                      // ceil(2^32 / multi_width): exact quotients for operands of at most 2^16
    const bool magic24 = multi_magic < (1u << 24);                   // (multi_width > 256: the product of a 16-bit and a 24-bit operand)
    const uint32_t blk = (CENSUS || FUSED) ? xcd_tile(blockIdx.x, gridDim.x) : blockIdx.x;   // group of 64 reads = row of the table
    uint64_t r0 = (uint64_t)blk * kReadsPerBlock;
    uint64_t r1 = r0 + kReadsPerBlock < a.n_reads ? r0 + kReadsPerBlock : a.n_reads;
    if (threadIdx.x == 0) s_cursor = 0;
    if (!WRITE && threadIdx.x < kMaxCountRanges) s_range_cnt[threadIdx.x] = 0;
    if (threadIdx.x <= r1 - r0) s_start[threadIdx.x] = a.start[r0 + threadIdx.x];
    if constexpr (CENSUS) {
        for (int i = threadIdx.x; i < kMaxFusedRanges * 256; i += kScanBlock) s_fz_hist[i] = 0;
        if (threadIdx.x < kMaxFusedRanges) { s_fz_bias[threadIdx.x] = a.fz_bias[threadIdx.x]; s_fz_shift[threadIdx.x] = a.fz_shift[threadIdx.x]; }
    }
    const uint32_t fz_bias = a.fz_bias[0], fz_shift = a.fz_shift[0];
    uint32_t fz_fill = 0, fz_round = 0;                              // fused writer: keys staged, rounds done (workgroup-uniform)
    if constexpr (FUSED) {
        // place of the row's first key of every digit value: the keys of the smaller values + the keys of the value in earlier rows
        const uint64_t t = a.fz_totals[threadIdx.x];
        const uint64_t ex = block_excl_scan64<kScanBlock>(t, fs.s64, nullptr);
        fs.next[threadIdx.x] = ex + a.fz_hist[(uint64_t)threadIdx.x * gridDim.x + blk];
        fs.cnt[threadIdx.x] = 0;
    }
    __syncthreads();
    Key<W> *out = reinterpret_cast<Key<W> *>(a.out);
    uint64_t base = WRITE && !FUSED ? a.block_base[blockIdx.x] : 0;
    uint32_t my_count = 0;
    unsigned long long kmers = 0;
    const int pad_bits = 2 * (16 * W - (k + 1));   // 2..32
    const bool even = !((k + 1) & 1);
    // up to 8 ranges counted at once: per lane in registers (an LDS atomic per item from 64 lanes on 3 addresses serialises)
    const bool few = multi && a.multi_n <= 8;
    uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t m_edge[W], m_k[W], m_k1[W];                             // the first k+1 / k / k-1 characters
    keep_masks<W>(k + 1, m_edge);
    keep_masks<W>(k, m_k);
    keep_masks<W>(k - 1, m_k1);
    // every word a lane of this workgroup can ask for lies inside the array (all but the workgroups of the array's last reads)
    const bool in_bounds = wave_uniform((s_start[r1 - r0] >> 4) + (uint64_t)(W + 1)) < a.n_words;

    // fused writer: the n staged keys leave in digit order, every digit value's keys as one run behind the row's earlier ones.  All
    // threads call (six barriers); the stage is free again on return.
    auto fz_digit = [&](uint32_t w0) { return ((w0 - fz_bias) >> fz_shift) & 255u; };
    auto flush = [&](uint32_t n) {
        if constexpr (FUSED) {
            const uint32_t tid = threadIdx.x;
            __syncthreads();                                           // the staged keys and their counts are in
            const uint32_t c = fs.cnt[tid], inc = wave_incl_scan(c);
            if (lane == 63) fs.scr[wv] = inc;
            __syncthreads();
            uint32_t ex = inc - c;
            for (int w = 0; w < wv; ++w) ex += fs.scr[w];
            fs.pos[tid] = ex;
            fs.cnt[tid] = 0;
            __syncthreads();
            for (uint32_t j = tid; j < n; j += kScanBlock) {           // (any order inside a digit value: nothing is ordered before the first pass)
                const uint32_t d = fz_digit(fs.stage[j].w[0]);
                fs.perm[fs.pos[d] + atomicAdd(&fs.cnt[d], 1u)] = (uint16_t)j;
            }
            __syncthreads();
            for (uint32_t i = tid; i < n; i += kScanBlock) {           // consecutive threads, consecutive places inside a run
                const Key<W> key = fs.stage[fs.perm[i]];
                const uint32_t d = fz_digit(key.w[0]);
                const uint64_t to = fs.next[d] + (i - fs.pos[d]);
                if (to < a.fz_n) {
                    out[to] = key;
                    if (a.side) {
                        const uint32_t sd = (key.w[0] - a.side_bias) >> a.side_shift;
                        if (a.side_bits > 8) reinterpret_cast<uint16_t *>(a.side)[to] = (uint16_t)(sd & ((1u << a.side_bits) - 1u));
                        else a.side[to] = (uint8_t)sd;
                    }
                }
            }
            __syncthreads();
            fs.next[tid] += c;
            fs.cnt[tid] = 0;
            __syncthreads();
        }
    };
    // one round of 64 positions: lane = position p of read r (s0 = its first character, npos = its positions); `active` lanes have one.
    // FUSED: every wave of the workgroup calls once per round, `more` = the wave has further rounds; returns whether any wave has
    auto positions = [&](bool active, uint64_t r, uint64_t s0, int p, int npos, bool more = false) {
        bool run_first = p == 0, run_last = p == npos - 1;
        if (active && a.is_solid && r < a.n_short) {               // solid runs inside the read (s2.cpp:276,280,288)
            auto sol = [&](int pp) {
                uint64_t bit = (uint64_t)a.num_k1_per_read * r + (uint64_t)pp;
                return (bool)((a.is_solid[bit >> 6] >> (bit & 63)) & 1);
            };
            active = sol(p);
            if (active) {
                run_first = p == 0 || !sol(p - 1);
                run_last = p == npos - 1 || !sol(p + 1);
            }
        }
        int cnt = 0;
        uint32_t fields = 0;                                       // count mode, few ranges: items of this position per range, 4 bits each
        uint32_t mask = 0;                                         // write mode: bit t = item type t of the position is wanted
        uint32_t e[W], rc[W];
        if (active) {
            // edge = characters [p, p+k] of the read
            uint64_t q = s0 + (uint64_t)p;
            uint64_t wi = q >> 4;
            int sh = (int)(q & 15) * 2;
            uint32_t raw[W + 1];
            if (in_bounds) {
#pragma unroll
                for (int j = 0; j <= W; ++j) raw[j] = a.packed[wi + j];
            } else {
#pragma unroll
                for (int j = 0; j <= W; ++j) raw[j] = (wi + j < a.n_words) ? a.packed[wi + j] : 0u;
            }
#pragma unroll
            for (int j = 0; j < W; ++j) e[j] = (uint32_t)(((((uint64_t)raw[j]) << 32) | (uint64_t)raw[j + 1]) >> (32 - sh)) & m_edge[j];
            // reverse complement (MegahitKmer::ReverseComplement, megahit_kmer.h:115-174)
#pragma unroll
            for (int j = 0; j < W; ++j) rc[j] = rev_chars(~e[W - 1 - j]);
            shl_bits<W>(rc, pad_bits);
            bool pal = even;                                       // s2.cpp:278 (an edge of odd length is never its own reverse complement)
            if (even) {
#pragma unroll
                for (int j = 0; j < W; ++j) pal = pal && (e[j] == rc[j]);
            }
            // the bucket (first 8 characters of the key, s2.cpp:832) is known before the key is built: most keys of a
            // narrow bucket range (memory-bound passes, multi-GPU shares) are dropped after three instructions
            auto push = [&](int t, const uint32_t (&src)[W], int from, uint32_t keep0) {
                const uint32_t b = ((src[0] << (2 * from)) >> 16);   // characters [from, from + 8), from <= 2
                if (b < a.b_lo || b >= a.b_hi) return;
                if (WRITE) mask |= 1u << t;
                else if (multi) {
                    const uint32_t x = b - a.b_lo;                  // (b - b_lo) / multi_width: both at most 2^16
                    uint32_t range;
                    if (magic24) asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(range) : "v"(x), "v"((uint32_t)multi_magic));   // full rate (v_mul_hi_u32: a quarter)
                    else range = (uint32_t)(((uint64_t)x * multi_magic) >> 32);
                    if (few) fields += 1u << (4 * range);
                    else atomicAdd(&s_range_cnt[range], 1u);
                    if constexpr (CENSUS) {                         // key word 0 (W >= 2: no flags in it) without building the key
                        const uint32_t w0 = (from ? ((src[0] << (2 * from)) | (src[W > 1 ? 1 : 0] >> (32 - 2 * from))) : src[0]) & keep0;
                        if (range < (uint32_t)kMaxFusedRanges)
                            atomicAdd(&s_fz_hist[range * 256u + (((w0 - s_fz_bias[range]) >> s_fz_shift[range]) & 255u)], 1u);
                    }
                }
                ++cnt;
            };
            if (run_first) {                                       // left $  (s2.cpp:531-540)
                push(0, e, 0, m_k[0]);
                if (!pal) push(1, rc, 2, m_k1[0]);
            }
            push(2, e, 1, m_k[0]);                                 // solid   (s2.cpp:543-550)
            if (!pal) push(3, rc, 1, m_k[0]);
            if (run_last) {                                        // right $ (s2.cpp:553-562)
                push(4, e, 2, m_k1[0]);
                if (!pal) push(5, rc, 0, m_k[0]);
            }
        }
        if (!WRITE) {
            my_count += (uint32_t)cnt;
            if (few) {
#pragma unroll
                for (int g = 0; g < 8; ++g)
                    if (g < (int)a.multi_n) acc[g] += (fields >> (4 * g)) & 15u;
            }
        } else {
            const uint32_t inc = wave_incl_scan((uint32_t)cnt);
            const uint32_t tot = __shfl(inc, 63, 64);
            uint32_t fz_before = 0, fz_tot[kScanBlock / 64] = {};
            bool any_more = false;
            if constexpr (FUSED) {
                // the keys every wave brings this round, and whether any wave has rounds left
                const uint32_t par = fz_round & 1u;
                ++fz_round;
                if (lane == 0) fs.wave_tot[par][wv] = tot | (more ? 0x80000000u : 0u);
                __syncthreads();
                for (int w = 0; w < kScanBlock / 64; ++w) fz_tot[w] = wave_uniform(fs.wave_tot[par][w]);
            }
            // FUSED: the waves take their places in the stage in turn; a wave whose keys do not fit behind the ones before flushes first
            // (every wave decides the same from the same four totals, so all reach that flush, each between the same two waves' turns):
            // the turns up to this wave's own before its keys are staged, the others after
            auto take_turns = [&](int from, int to) {
                if constexpr (FUSED) {
#pragma unroll
                    for (int turn = 0; turn < kScanBlock / 64; ++turn) {   // (constant bounds: fz_tot stays in registers)
                        if (turn < from || turn >= to) continue;
                        const uint32_t tw = fz_tot[turn] & 0x7FFFFFFFu;
                        any_more = any_more || (fz_tot[turn] >> 31);
                        if (fz_fill + tw > (uint32_t)FusedCfg<W>::kCap) { flush(fz_fill); fz_fill = 0; }
                        fz_before = fz_fill;
                        fz_fill += tw;
                    }
                }
            };
            take_turns(0, wv + 1);
            if (tot) {
                uint32_t wbase = 0;
                if (!FUSED && lane == 0) wbase = atomicAdd(&s_cursor, tot);
                const uint64_t first = base + (uint64_t)wave_uniform(wbase);   // the wave's slots [first, first + tot): a scalar
                char *const wave_out = reinterpret_cast<char *>(out + first);
                uint8_t *const wave_side = !FUSED && a.side ? a.side + first : nullptr;
                uint32_t slot = inc - (uint32_t)cnt + fz_before;        // < 6 * 64 (FUSED: place in the stage)
                // every wanted item straight to its slot (no staging array: a lane-varying index into one costs a waterfall loop per store).
                // key = characters [from, from + n) of src, flags in the low 4 bits: (n == k) << 3 | prev   [cx1_read2sdbg_s2.cpp:613-671]
                auto put = [&](int t, const uint32_t (&src)[W], int from, const uint32_t (&keep)[W], uint32_t flags) {
                    if (!((mask >> t) & 1u)) return;
                    Key<W> key;
#pragma unroll
                    for (int j = 0; j < W; ++j) {
                        const uint32_t nx = j + 1 < W ? src[j + 1 < W ? j + 1 : j] : 0u;
                        key.w[j] = (from ? ((src[j] << (2 * from)) | (nx >> (32 - 2 * from))) : src[j]) & keep[j];
                    }
                    key.w[W - 1] |= flags;
                    if constexpr (FUSED) {
                        // (a wave's keys of a round always fit an empty stage, kCap >= kWaveRound: the test only keeps a store
                        // inside the array should that ever be broken; MGTA_SORT_FUSED=2 would then report the missing keys)
                        if (slot < (uint32_t)FusedCfg<W>::kCap) {
                            fs.stage[slot] = key;
                            atomicAdd(&fs.cnt[fz_digit(key.w[0])], 1u);
                        }
                    } else {
                        *reinterpret_cast<Key<W> *>(wave_out + slot * (uint32_t)sizeof(Key<W>)) = key;
                        if (wave_side) wave_side[slot] = (uint8_t)((key.w[0] - a.side_bias) >> a.side_shift);
                    }
                    ++slot;
                };
                const uint32_t e0 = e[0] >> 30, e1 = (e[0] >> 28) & 3u, r0c = rc[0] >> 30, r1c = (rc[0] >> 28) & 3u;
                put(0, e, 0, m_k, 8u | (uint32_t)kDollar);
                put(1, rc, 2, m_k1, r1c);
                put(2, e, 1, m_k, 8u | e0);
                put(3, rc, 1, m_k, 8u | r0c);
                put(4, e, 2, m_k1, e1);
                put(5, rc, 0, m_k, 8u | (uint32_t)kDollar);
            }
            take_turns(wv + 1, kScanBlock / 64);
            if constexpr (FUSED) {
                if (!any_more) flush(fz_fill);                         // the last round of the workgroup
                return any_more;
            }
        }
        return false;
    };
    // The reads of a wave all of one length (the common case) and no solid bits: their positions are numbered through, 64 per round --
    // reads of 150 bp at k = 44 have 106 positions: 26.5 rounds for the wave's 16 reads instead of 32 (the second round of a read of its
    // own has 42 of 64 lanes at work).  Else: a read at a time.
    constexpr int kWaves = kScanBlock / 64, kReadsPerWave = kReadsPerBlock / kWaves;
    const uint32_t n_mine = r0 + wv < r1 ? (uint32_t)((r1 - r0 - wv + kWaves - 1) / kWaves) : 0u;   // reads r0 + wv + kWaves i, i < n_mine
    uint32_t my_len = 0;
    if ((uint32_t)lane < n_mine) my_len = (uint32_t)(s_start[wv + kWaves * lane + 1] - s_start[wv + kWaves * lane]);
    const uint32_t len0 = wave_uniform(my_len);
    const bool uniform = !a.is_solid && n_mine > 0 && len0 >= (uint32_t)(k + 1) && len0 - (uint32_t)k <= 4096u &&
                         __ballot((uint32_t)lane < n_mine && my_len != len0) == 0;
    static_assert(kReadsPerWave <= 64, "one lane per read of the wave");
    if constexpr (FUSED) {
        // the same rounds as below, but in step: every wave goes through a round's barrier until the last wave has had its last round
        // (a wave that is through, or has no read at all, brings no positions)
        uint32_t v = 0, total = 0, npos_u = 1, magic = 0;                     // numbered-through route
        uint64_t rr = r0 + wv;                                                // read-at-a-time route: the read and the round inside it
        int c0 = 0;
        auto skip_short = [&]() {                                             // s2.cpp:262-264
            while (rr < r1 && (int)(s_start[rr - r0 + 1] - s_start[rr - r0]) < k + 1) rr += kWaves;
        };
        if (uniform) {
            npos_u = len0 - (uint32_t)k;
            total = npos_u * n_mine;
            magic = (uint32_t)(((1ull << 32) + npos_u - 1) / npos_u);
        } else
            skip_short();
        struct Round { bool have, active; uint64_t r, s0; int p, npos; };
        auto advance = [&]() {                                                // the wave's next round, if it has one
            Round d{false, false, r0, 0, 0, 1};
            if (uniform) {
                if (v < total) {
                    const uint32_t idx = v + (uint32_t)lane;
                    d.have = true;
                    d.active = idx < total;
                    const uint32_t i = npos_u == 1 ? idx : __umulhi(idx, magic);
                    const uint32_t slot = d.active ? wv + kWaves * i : wv;
                    d.p = (int)(idx - i * npos_u); d.npos = (int)npos_u;
                    d.r = r0 + slot; d.s0 = s_start[slot];
                    v += 64;
                }
            } else if (rr < r1) {
                d.have = true;
                d.r = rr; d.s0 = s_start[rr - r0];
                d.npos = (int)(s_start[rr - r0 + 1] - d.s0) - k;
                d.p = c0 + lane;
                d.active = d.p < d.npos;
                c0 += 64;
                if (c0 >= d.npos) { c0 = 0; rr += kWaves; skip_short(); }
            }
            return d;
        };
        for (;;) {
            const Round cur = advance();
            if (!positions(cur.active, cur.r, cur.s0, cur.p, cur.npos, uniform ? v < total : rr < r1)) break;
        }
    } else if (uniform) {
        const uint32_t npos = len0 - (uint32_t)k, total = npos * n_mine;     // <= 4096 * 16
        const uint32_t magic = (uint32_t)(((1ull << 32) + npos - 1) / npos);  // idx / npos for idx < 2^16 (npos = 1: magic wraps, handled)
        if (lane == 0) kmers += (unsigned long long)total;
        for (uint32_t v = 0; v < total; v += 64) {
            const uint32_t idx = v + (uint32_t)lane;
            const bool active = idx < total;
            const uint32_t i = npos == 1 ? idx : __umulhi(idx, magic), p = idx - i * npos;
            const uint32_t slot = active ? wv + kWaves * i : wv;           // read r0 + slot
            positions(active, r0 + slot, s_start[slot], (int)p, (int)npos);
        }
    } else {
        for (uint64_t r = r0 + wv; r < r1; r += kWaves) {
            const uint64_t s0 = s_start[r - r0];
            const int len = (int)(s_start[r - r0 + 1] - s0);
            if (len < k + 1) continue;                                     // s2.cpp:262-264
            const int npos = len - k;
            if (lane == 0) kmers += (unsigned long long)npos;
            for (int c0 = 0; c0 < npos; c0 += 64) positions(c0 + lane < npos, r, s0, c0 + lane, npos);
        }
    }
    if (!WRITE) {
        my_count = wave_sum(my_count);
        if (few) {
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                if (g < (int)a.multi_n) {
                    const uint32_t t = wave_sum(acc[g]);
                    if (lane == 0 && t) atomicAdd(&s_range_cnt[g], t);
                }
            }
        }
        if (lane == 0) s_wave_cnt[wv] = my_count;
        __syncthreads();
        if (threadIdx.x == 0 && !multi) {
            uint32_t t = 0;
            for (int w = 0; w < kScanBlock / 64; ++w) t += s_wave_cnt[w];
            a.block_count[blockIdx.x] = t;
        }
        if (multi && threadIdx.x < a.multi_n) a.block_count[(uint64_t)threadIdx.x * gridDim.x + blk] = s_range_cnt[threadIdx.x];
        if (lane == 0 && kmers && a.n_kmers) atomicAdd(a.n_kmers, kmers);
        if constexpr (CENSUS) {                                        // the workgroup's row of every range's table
            const uint32_t n_rows = (a.multi_n < (uint32_t)kMaxFusedRanges ? a.multi_n : (uint32_t)kMaxFusedRanges) * 256u;
            for (uint32_t i = threadIdx.x; i < n_rows; i += kScanBlock) a.fz_hist[(uint64_t)i * gridDim.x + blk] = s_fz_hist[i];
        }
    }
}

template <int W, bool WRITE, bool CENSUS = false>
__global__ __launch_bounds__(kScanBlock) void item_scan_kernel(ScanArgs a) {
    item_scan_body<W, WRITE, CENSUS, false>(a);
}

// The key writer of a pass whose first global sort pass was counted ahead by the count scan (item_scan_kernel<W, false, true>): the
// same positions and keys as item_scan_kernel<W, true>, but every key goes where that sort pass would have moved it, so the pass
// (a census and a scatter over every key) does not run.  The row of a workgroup in the table is its group of 64 reads.
template <int W>
__global__ __launch_bounds__(kScanBlock) void item_write_fused_kernel(ScanArgs a) {
    item_scan_body<W, true, false, true>(a);
}

// MGTA_SORT_FUSED=2: every key of the fused writer's output lies in the slice of its digit value (bad[0] counts those that do not),
// and the slices add up to the keys of the pass (bad[1])
template <int W>
__global__ __launch_bounds__(kScanBlock) void fused_check_kernel(const Key<W> *keys, uint64_t n, const uint64_t *totals, uint32_t bias, uint32_t shift,
                                                                 uint32_t *bad) {
    __shared__ uint64_t s_first[257];
    __shared__ uint64_t s64[kScanBlock / 64 + 1];
    const uint64_t t = totals[threadIdx.x];
    const uint64_t ex = block_excl_scan64<kScanBlock>(t, s64, nullptr);
    s_first[threadIdx.x] = ex;
    if (threadIdx.x == kScanBlock - 1) s_first[256] = ex + t;
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0 && s_first[256] != n) atomicAdd(&bad[1], 1u);
    for (uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kScanBlock) {
        const uint32_t d = ((keys[i].w[0] - bias) >> shift) & 255u;
        if (i < s_first[d] || i >= s_first[d + 1]) atomicAdd(&bad[0], 1u);
    }
}

// Key generation when the item layout is known in closed form (every position solid; k+1 odd: no palindromes, k+1 even: see below; every bucket
// wanted): read r owns 2 npos + 4 consecutive keys [left $ of e, left $ of rc, then (e, rc) of every position, right $ of e,
// right $ of rc], so every lane stores its two keys at a fixed place: no staging, no prefix sums, fully coalesced 24-byte pairs.
// With k+1 even a (k+1)-mer can be its own reverse complement; the reference then emits the forward items only (s2.cpp:278).  The
// layout stays closed: the rc slot of such a position takes a SENTINEL key (all ones: larger than any real key, whose low three bits
// are a character code <= 4), the sentinels are counted, end up behind every real key in the sorted array and the emitter stops
// before them.
template <int W>
__global__ __launch_bounds__(kScanBlock) void item_write_closed_kernel(ScanArgs a) {
    __shared__ uint32_t s_read_base[kReadsPerBlock];
    __shared__ uint64_t s_start[kReadsPerBlock + 1];                  // one coalesced load instead of two dependent ones per read
    const int k = a.k;
    const int lane = lane_id(), wv = wave_id();
    const uint64_t r0 = (uint64_t)blockIdx.x * kReadsPerBlock;
    const uint64_t r1 = r0 + kReadsPerBlock < a.n_reads ? r0 + kReadsPerBlock : a.n_reads;
    if (wv == 0) {                                                    // first key of every read of the workgroup
        const uint64_t st = r0 + lane <= r1 ? a.start[r0 + lane] : 0, st_next = r0 + lane < r1 ? a.start[r0 + lane + 1] : st;
        s_start[lane] = st;
        if (r0 + lane + 1 == r1) s_start[lane + 1] = st_next;
        uint32_t items = 0;
        if (r0 + lane < r1) {
            const int len = (int)(st_next - st);
            if (len >= k + 1) items = 2u * (uint32_t)(len - k) + 4u;
        }
        s_read_base[lane] = wave_incl_scan(items) - items;
    }
    __syncthreads();
    Key<W> *out = reinterpret_cast<Key<W> *>(a.out) + a.block_base[blockIdx.x];
    const int pad_bits = 2 * (16 * W - (k + 1));
    for (uint64_t r = r0 + wv; r < r1; r += kScanBlock / 64) {
        const uint64_t s0 = s_start[r - r0];
        const int len = (int)(s_start[r - r0 + 1] - s0);
        if (len < k + 1) continue;
        const int npos = len - k;
        Key<W> *ro = out + s_read_base[r - r0];
        for (int c0 = 0; c0 < npos; c0 += 64) {
            const int p = c0 + lane;
            if (p >= npos) continue;
            const uint64_t q = s0 + (uint64_t)p, wi = q >> 4;
            const int sh = (int)(q & 15) * 2;
            uint32_t raw[W + 1], e[W], rc[W];
#pragma unroll
            for (int j = 0; j <= W; ++j) raw[j] = (wi + j < a.n_words) ? a.packed[wi + j] : 0u;
#pragma unroll
            for (int j = 0; j < W; ++j) e[j] = sh ? ((raw[j] << sh) | (raw[j + 1] >> (32 - sh))) : raw[j];
            keep_chars<W>(e, k + 1);
#pragma unroll
            for (int j = 0; j < W; ++j) rc[j] = rev_chars(~e[W - 1 - j]);
            shl_bits<W>(rc, pad_bits);
            const int e0 = e[0] >> 30, e1 = (e[0] >> 28) & 3, r0c = rc[0] >> 30, r1c = (rc[0] >> 28) & 3;
            bool pal = false;                                           // s2.cpp:278 (only possible when k+1 is even)
            if (!((k + 1) & 1)) {
                pal = true;
#pragma unroll
                for (int j = 0; j < W; ++j) pal = pal && e[j] == rc[j];
            }
            Key<W> sentinel;
#pragma unroll
            for (int j = 0; j < W; ++j) sentinel.w[j] = ~0u;
            ro[2 + 2 * p] = make_key<W>(e, 1, k, k, e0);                 // solid   (s2.cpp:543-550)
            ro[3 + 2 * p] = pal ? sentinel : make_key<W>(rc, 1, k, k, r0c);
            if (p == 0) {                                               // left $  (s2.cpp:531-540)
                ro[0] = make_key<W>(e, 0, k, k, kDollar);
                ro[1] = pal ? sentinel : make_key<W>(rc, 2, k - 1, k, r1c);
            }
            if (p == npos - 1) {                                        // right $ (s2.cpp:553-562)
                ro[2 + 2 * npos] = make_key<W>(e, 2, k - 1, k, e1);
                ro[3 + 2 * npos] = pal ? sentinel : make_key<W>(rc, 0, k, k, kDollar);
            }
            const unsigned long long pm = __ballot(pal);                 // rare: one atomic per wave that saw any
            if (pm && lane == __ffsll((long long)pm) - 1) {
                unsigned long long c = 0;
                for (unsigned long long m = pm; m; m &= m - 1) {
                    const int l = __ffsll((long long)m) - 1, pp = c0 + l;
                    c += 1ull + (pp == 0) + (pp == npos - 1);
                }
                atomicAdd(a.n_sentinel, c);
            }
        }
    }
}

// Items per workgroup of item_scan_kernel in closed form.  With k+1 odd no (k+1)-mer equals its reverse complement (with k+1 even the
// slot of the missing item takes a sentinel key, item_write_closed_kernel), so when
// every position is solid and every bucket is wanted a read with npos = len - k >= 1 positions yields exactly
// 2 npos + 4 items (two per position, two more at each end of the read): no edge has to be built to count them.
__global__ __launch_bounds__(256) void item_count_closed_kernel(const uint64_t *start, uint64_t n_reads, uint64_t n_blocks, int k,
                                                                uint32_t *block_count, unsigned long long *n_kmers) {
    // a wave per 16 consecutive workgroups of item_scan_kernel (64 reads each), one lane per read
    unsigned long long kmers = 0;
    for (int q = 0; q < 16; ++q) {
        const uint64_t blk = ((uint64_t)blockIdx.x * 4 + wave_id()) * 16 + q;
        if (blk >= n_blocks) break;
        const uint64_t r = blk * kReadsPerBlock + lane_id();
        uint32_t items = 0, npos = 0;
        if (r < n_reads) {
            const int len = (int)(start[r + 1] - start[r]);
            if (len >= k + 1) { npos = (uint32_t)(len - k); items = 2 * npos + 4; }
        }
        items = wave_sum(items);
        kmers += wave_sum(npos);
        if (lane_id() == 0 && block_count) block_count[blk] = items;   // (nullptr: only the k-mer total is wanted)
    }
    if (lane_id() == 0 && n_kmers && kmers) atomicAdd(n_kmers, kmers);
}

// ---------------------------------------------------------------------------------------------
// 4. LSD radix sort (8-bit digits)
// ---------------------------------------------------------------------------------------------
constexpr int kSortThreads = 1024;                   // 16 waves
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kItemsPerThread = 4;
constexpr int kSubTile = kSortThreads * kItemsPerThread;   // 4096 keys staged in LDS at a time
constexpr int kSubTilesPerBlock = 8;
constexpr int kBlockTile = kSubTile * kSubTilesPerBlock;   // 32768 keys per workgroup

struct Digit {
    int pos;     // bit position counted from the least significant bit of the whole key
    int bits;    // <= 8 (a global pass: the BITS of its kernels, 8 or 9)
    uint32_t bias;   // subtracted from key word 0 before the bits are taken (0 except for the global passes of a bucket sub-range build,
                     // where word 0 - (first bucket << 16) has leading zero bits that the digits skip)
};

template <int W, bool BIASED = false>          // BIASED: honour d.bias (only the global passes of a sub-range build set it)
__device__ __forceinline__ uint32_t get_digit(const Key<W> &key, Digit d) {
    // the word is picked by a wave-uniform branch on compile-time indices: a run-time index into key.w[] would push every
    // register-resident key of the caller into scratch memory, and a chain of selects costs 2W VALU ops per key
    // (the empty asm keeps the compiler from turning the branches back into selects)
    const int wi = W - 1 - (d.pos >> 5), off = d.pos & 31;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j == wi) {
            lo = key.w[j] - (BIASED && j == 0 ? d.bias : 0u);
            hi = j > 0 ? key.w[j - 1] - (BIASED && j == 1 ? d.bias : 0u) : 0u;
            asm volatile("" : "+v"(lo), "+v"(hi));
        }
    }
    return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)off) & ((1u << d.bits) - 1u);
}

// the same digit of N register-resident keys: one wave-uniform branch chain for all of them
template <int W, int N, bool BIASED = false>
__device__ __forceinline__ void get_digits(const Key<W> (&key)[N], Digit d, uint32_t (&dg)[N]) {
    const int wi = W - 1 - (d.pos >> 5), off = d.pos & 31;
    uint32_t lo[N], hi[N];
#pragma unroll
    for (int i = 0; i < N; ++i) { lo[i] = 0; hi[i] = 0; }
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j == wi) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                lo[i] = key[i].w[j] - (BIASED && j == 0 ? d.bias : 0u);
                hi[i] = j > 0 ? key[i].w[j - 1] - (BIASED && j == 1 ? d.bias : 0u) : 0u;
                asm volatile("" : "+v"(lo[i]), "+v"(hi[i]));
            }
        }
    }
    const uint32_t mask = (1u << d.bits) - 1u;
#pragma unroll
    for (int i = 0; i < N; ++i) dg[i] = __builtin_amdgcn_alignbit(hi[i], lo[i], (uint32_t)off) & mask;
}

// wave_match (device_utils.hpp) for digits of a fixed width above 8 bits: one more ballot per bit
template <int BITS>
__device__ __forceinline__ void wave_match_wide(uint32_t dg, bool valid, uint32_t &rank, uint32_t &cnt) {
    static_assert(BITS > 8 && BITS <= 16, "wave_match covers digits of up to 8 bits");
    const uint64_t v = __ballot(valid);
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        const int sx = (int)(dg << (31 - b)) >> 31;
        const uint64_t bal = __ballot(sx < 0);
        lo &= ~((uint32_t)bal ^ (uint32_t)sx);
        hi &= ~((uint32_t)(bal >> 32) ^ (uint32_t)sx);
    }
    rank = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
    cnt = (uint32_t)__popc(lo) + (uint32_t)__popc(hi);
}

// census: hist[digit * n_tiles + tile] (BITS: width of the digit's kernels, 1 << BITS values)
template <int W, int BITS = 8>
__global__ __launch_bounds__(kSortThreads) void radix_census_kernel(const Key<W> *keys, uint64_t n, Digit d, uint64_t n_tiles,
                                                                     uint64_t *hist) {
    constexpr int kVals = 1 << BITS;
    __shared__ uint32_t h[kVals];
    for (int i = threadIdx.x; i < kVals; i += kSortThreads) h[i] = 0;
    __syncthreads();
    const uint32_t tile = xcd_tile(blockIdx.x, (uint32_t)n_tiles);     // (neighbouring tiles' counters share lines: one L2 writes them)
    uint64_t base = (uint64_t)tile * kBlockTile;
    int wi = W - 1 - (d.pos >> 5), off = d.pos & 31;
    bool straddle = off + d.bits > 32 && wi > 0;
    uint32_t mask = (1u << d.bits) - 1u;
    for (int i = 0; i < kBlockTile / kSortThreads; ++i) {
        uint64_t idx = base + (uint64_t)i * kSortThreads + threadIdx.x;
        if (idx < n) {
            uint32_t v = (keys[idx].w[wi] - (wi == 0 ? d.bias : 0u)) >> off;
            if (straddle) v |= (keys[idx].w[wi - 1] - (wi == 1 ? d.bias : 0u)) << (32 - off);
            atomicAdd(&h[v & mask], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kVals; i += kSortThreads) hist[(uint64_t)i * n_tiles + tile] = h[i];
}

// The same census from the SIDE array of the previous scatter (one byte per key: the digit this pass sorts on, written next to the
// key at its destination): 1 byte read per key instead of the whole key (W = 3: 7.2 GB instead of 86 GB per launch at 100 M reads).
// A digit of more than 8 bits travels as uint16_t: 2 bytes per key, eight keys per 16-byte load.
template <int BITS> using SideEntry = std::conditional_t<(BITS > 8), uint16_t, uint8_t>;

template <int BITS = 8>
__global__ __launch_bounds__(kSortThreads) void radix_census_side_kernel(const SideEntry<BITS> *side, uint64_t n, uint64_t n_tiles, uint64_t *hist) {
    constexpr int kVals = 1 << BITS;
    constexpr uint32_t kMask = kVals - 1;
    __shared__ uint32_t h[kVals];
    for (int i = threadIdx.x; i < kVals; i += kSortThreads) h[i] = 0;
    __syncthreads();
    const uint32_t tile = xcd_tile(blockIdx.x, (uint32_t)n_tiles);
    const uint64_t base = (uint64_t)tile * kBlockTile;                       // a multiple of 32768: 16-byte loads are aligned
    constexpr int kPerThread = kBlockTile / kSortThreads;                    // 32 entries = two (four) 16-byte loads, consecutive threads consecutive
    constexpr int kPerLoad = 16 / (int)sizeof(SideEntry<BITS>);              // entries of a 16-byte load
#pragma unroll
    for (int half = 0; half < kPerThread / kPerLoad; ++half) {
        const uint64_t idx = base + (uint64_t)half * (kSortThreads * kPerLoad) + (uint64_t)threadIdx.x * kPerLoad;
        if (idx + kPerLoad <= n) {
            const uint4 v = *reinterpret_cast<const uint4 *>(side + idx);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (BITS > 8) {
                    atomicAdd(&h[w[j] & kMask], 1u);
                    atomicAdd(&h[(w[j] >> 16) & kMask], 1u);
                } else {
                    atomicAdd(&h[w[j] & 255u], 1u);
                    atomicAdd(&h[(w[j] >> 8) & 255u], 1u);
                    atomicAdd(&h[(w[j] >> 16) & 255u], 1u);
                    atomicAdd(&h[w[j] >> 24], 1u);
                }
            }
        } else {
            for (uint64_t i = idx; i < n && i < idx + kPerLoad; ++i) atomicAdd(&h[side[i] & kMask], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kVals; i += kSortThreads) hist[(uint64_t)i * n_tiles + tile] = h[i];
}

// Closed-form key generation (see item_write_closed_kernel) cut along the census tiles of the first global sort pass: workgroup t
// writes exactly the keys [t kBlockTile, (t+1) kBlockTile) and counts their first-pass digit in LDS on the way, so the keys are not
// read back for that census (one of the 11 HBM crossings of the key array).  A read owns npos + 2 PAIRS of keys (left $ pair, one pair
// per position, right $ pair); read bases and tile bounds are even, so a pair never straddles a tile: lane = pair, 24 contiguous
// bytes per lane, consecutive lanes consecutive pairs.  The reads of a tile are found from block_base (first key of every 64 reads).
template <int W>
__global__ __launch_bounds__(kScanBlock) void item_write_tiled_kernel(ScanArgs a, uint64_t n_blocks, uint64_t n_items, int digit_shift,
                                                                      uint64_t n_tiles, uint64_t *hist) {
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_read_base[kReadsPerBlock];
    __shared__ uint64_t s_start[kReadsPerBlock + 1];
    const int k = a.k;
    const int lane = lane_id(), wv = wave_id();
    for (int i = threadIdx.x; i < 256; i += kScanBlock) s_hist[i] = 0;
    const uint64_t lo = (uint64_t)blockIdx.x * kBlockTile;
    const uint64_t hi = lo + kBlockTile < n_items ? lo + kBlockTile : n_items;
    // last group of 64 reads whose first key is at or before `lo`: 64-ary search, every wave on its own (block_base[0] = 0 <= lo)
    uint64_t left = 0, right = n_blocks;
    while (right - left > 1) {
        const uint64_t step = (right - left + 63) / 64, idx = left + (uint64_t)lane * step;
        const bool ok = idx < right && a.block_base[idx] <= lo;
        const unsigned long long m = __ballot(ok);                     // a prefix of lanes: block_base is non-decreasing
        const uint64_t nl = left + (uint64_t)(__popcll(m) - 1) * step;
        right = nl + step < right ? nl + step : right;
        left = nl;
    }
    Key<W> *out = reinterpret_cast<Key<W> *>(a.out);
    const int pad_bits = 2 * (16 * W - (k + 1));
    for (uint64_t b = left; b < n_blocks; ++b) {
        const uint64_t bb = a.block_base[b];
        if (bb >= hi) break;
        const uint64_t r0 = b * kReadsPerBlock;
        const uint64_t r1 = r0 + kReadsPerBlock < a.n_reads ? r0 + kReadsPerBlock : a.n_reads;
        __syncthreads();                                               // the previous group's table is no longer read
        if (wv == 0) {
            const uint64_t st = r0 + lane <= r1 ? a.start[r0 + lane] : 0, st_next = r0 + lane < r1 ? a.start[r0 + lane + 1] : st;
            s_start[lane] = st;
            if (r0 + lane + 1 == r1) s_start[lane + 1] = st_next;
            uint32_t items = 0;
            if (r0 + lane < r1) {
                const int len = (int)(st_next - st);
                if (len >= k + 1) items = 2u * (uint32_t)(len - k) + 4u;
            }
            s_read_base[lane] = wave_incl_scan(items) - items;
        }
        __syncthreads();
        for (uint64_t r = r0 + wv; r < r1; r += kScanBlock / 64) {
            const uint64_t s0 = s_start[r - r0];
            const int len = (int)(s_start[r - r0 + 1] - s0);
            if (len < k + 1) continue;
            const int npos = len - k;
            const uint64_t rb = bb + s_read_base[r - r0], re = rb + 2ull * (uint64_t)npos + 4ull;
            if (re <= lo || rb >= hi) continue;
            const int j_lo = rb >= lo ? 0 : (int)((lo - rb) >> 1), j_hi = re <= hi ? npos + 2 : (int)((hi - rb) >> 1);
            Key<W> *ro = out + rb;
            for (int c0 = j_lo; c0 < j_hi; c0 += 64) {
                const int j = c0 + lane;
                if (j >= j_hi) continue;
                const int p = j == 0 ? 0 : (j == npos + 1 ? npos - 1 : j - 1);
                const uint64_t q = s0 + (uint64_t)p, wi = q >> 4;
                const int sh = (int)(q & 15) * 2;
                uint32_t raw[W + 1], e[W], rc[W];
#pragma unroll
                for (int i = 0; i <= W; ++i) raw[i] = (wi + i < a.n_words) ? a.packed[wi + i] : 0u;
#pragma unroll
                for (int i = 0; i < W; ++i) e[i] = sh ? ((raw[i] << sh) | (raw[i + 1] >> (32 - sh))) : raw[i];
                keep_chars<W>(e, k + 1);
#pragma unroll
                for (int i = 0; i < W; ++i) rc[i] = rev_chars(~e[W - 1 - i]);
                shl_bits<W>(rc, pad_bits);
                const int e0 = e[0] >> 30, e1 = (e[0] >> 28) & 3, r0c = rc[0] >> 30, r1c = (rc[0] >> 28) & 3;
                bool pal = false;                                       // s2.cpp:278: the rc slot takes a sentinel (item_write_closed_kernel)
                if (!((k + 1) & 1)) {
                    pal = true;
#pragma unroll
                    for (int i = 0; i < W; ++i) pal = pal && e[i] == rc[i];
                }
                Key<W> ka, kb;
                if (j == 0) {                                           // left $  (s2.cpp:531-540)
                    ka = make_key<W>(e, 0, k, k, kDollar);
                    kb = make_key<W>(rc, 2, k - 1, k, r1c);
                } else if (j == npos + 1) {                             // right $ (s2.cpp:553-562)
                    ka = make_key<W>(e, 2, k - 1, k, e1);
                    kb = make_key<W>(rc, 0, k, k, kDollar);
                } else {                                                // solid   (s2.cpp:543-550)
                    ka = make_key<W>(e, 1, k, k, e0);
                    kb = make_key<W>(rc, 1, k, k, r0c);
                }
                if (pal) {
#pragma unroll
                    for (int i = 0; i < W; ++i) kb.w[i] = ~0u;
                }
                const unsigned long long pm = __ballot(pal);
                if (pm && lane == __ffsll((long long)pm) - 1) atomicAdd(a.n_sentinel, (unsigned long long)__popcll(pm));
                ro[2 * j] = ka;
                ro[2 * j + 1] = kb;
                atomicAdd(&s_hist[(ka.w[0] >> digit_shift) & 255u], 1u);
                atomicAdd(&s_hist[(kb.w[0] >> digit_shift) & 255u], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += kScanBlock) hist[(uint64_t)i * n_tiles + blockIdx.x] = s_hist[i];
}

// one workgroup per digit value: exclusive scan of its row of tile counts, in place; row total -> totals[digit]
__global__ __launch_bounds__(1024) void radix_rowscan_kernel(uint64_t *hist, uint64_t n_tiles, uint64_t *totals) {
    __shared__ uint64_t scratch[1024 / 64 + 1];
    __shared__ uint64_t carry_s;
    uint64_t *row = hist + (uint64_t)blockIdx.x * n_tiles;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint64_t b = 0; b < n_tiles; b += 1024) {
        uint64_t idx = b + threadIdx.x;
        uint64_t x = idx < n_tiles ? row[idx] : 0, tot;
        uint64_t ex = block_excl_scan64<1024>(x, scratch, &tot);
        uint64_t carry = carry_s;
        if (idx < n_tiles) row[idx] = carry + ex;
        __syncthreads();
        if (threadIdx.x == 0) carry_s = carry + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry_s;
}

// keys staged in LDS per round of the scatter: 4096, or 2048 for the 10- and 11-word records of stage 1 at k > 110 (a 4096-key stage
// of those would not fit the 160 KB); a tile stays 32768 keys either way (census and scatter agree on that)
template <int W> struct ScatterCfg {
    static constexpr int kIpt = W >= 10 ? 2 : kItemsPerThread;
    static constexpr int kSub = kSortThreads * kIpt;
    static constexpr int kChunk = kSub / kSortWaves;
};

// shared state of one scatter workgroup (BITS: width of the digit it scatters by, 8..10)
template <int W, int BITS = 8>
struct ScatterShared {
    static constexpr int kVals = 1 << BITS;
    Key<W> keys[ScatterCfg<W>::kSub];
    uint16_t whist[kSortWaves][kVals]; // per wave: running count, then position of the wave's first key of the digit value in the sorted sub-tile
    uint64_t gbase[kVals];             // global destination of the next key of each digit value
    uint64_t gdelta[kVals];            // global destination minus position in the sorted sub-tile
    uint32_t scratch[kSortThreads / 64 + 1];
};

// stable scatter of in[0..n) by digit d to out[gbase[digit]++...], sub-tile by sub-tile (gbase must be set and visible; all threads
// call).  Four workgroup barriers per sub-tile; the next sub-tile's keys are on their way while the current one is placed.
// SIDE: the digit the NEXT pass sorts on (d_next) of every key, one byte per key, for that pass's census.  The bytes of a 32768-key
// tile are collected in LDS in the order the tile's keys land in (per digit value the eight sub-tiles append to ONE run of ~128 keys)
// and written run by run when the tile is done: byte stores straight from the sub-tiles (runs of ~16 bytes, four per wave
// instruction) cost the scatter 21 % (100 M reads: 43.9 -> 53.4 ms per launch).
// An entry is as wide as the digit it carries (NEXT_BITS, SideEntry): uint16_t where the next pass sorts on more than 8 bits.
template <int BITS = 8, int NEXT_BITS = 8>
struct SideShared {
    static constexpr int kVals = 1 << BITS;
    SideEntry<NEXT_BITS> bytes[kBlockTile];
    uint64_t gtile[kVals];             // global destination of the tile's first key of a digit value minus that key's place in `bytes`
    uint32_t toff[kVals + 1];          // place in `bytes` of the tile's first key of a digit value
};

// STABLE = false: keys of one digit value may leave in any order -- all the FIRST pass of an LSD sort needs (nothing is ordered yet).
// The rank inside the wave's chunk then comes from an LDS atomic on the wave's counter instead of the eight ballots of wave_match,
// which are 45 % of the stable kernel's vector instructions (54 of ~120 per key).
// BITS: width of d (1 << BITS digit values: 8, or 9..10 for the wide passes of a plan); NEXT_BITS: width of d_next (SIDE).
template <int W, bool BIASED = false, bool SIDE = false, bool STABLE = true, int BITS = 8, int NEXT_BITS = 8>
__device__ __forceinline__ void scatter_subtiles(ScatterShared<W, BITS> &sh, const Key<W> *in, Key<W> *out, uint64_t n, Digit d,
                                                 SideShared<BITS, NEXT_BITS> *ss = nullptr, Digit d_next = Digit{0, 0, 0}) {
    constexpr int kItemsPerThread = ScatterCfg<W>::kIpt, kSubTile = ScatterCfg<W>::kSub, kWaveChunk = ScatterCfg<W>::kChunk;   // (shadow the 4096-key constants)
    constexpr int kVals = 1 << BITS, kValWaves = kVals / 64;       // digit values; waves that hold one value per thread in phase 2
    constexpr uint32_t kDigitMask = kVals - 1;
    static_assert(BITS >= 8 && kValWaves <= kSortWaves && BITS + 13 <= 31, "a thread per digit value; digit | place in the sub-tile << BITS | valid << 31");
    static_assert(STABLE || BITS == 8, "only the first pass to run is unstable, and that one sorts on 8 bits");
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    uint16_t *whist = sh.whist[wv];               // wave-private row, updated lane-to-lane inside the wave
    for (int i = lane; i < kVals; i += 64) whist[i] = 0;
    constexpr bool kPrefetch = W * kItemsPerThread <= 16;   // wider keys: the registers are better spent on the keys in flight
    Key<W> key[kItemsPerThread], nxt[kItemsPerThread];
    auto load = [&](Key<W> (&dst)[kItemsPerThread], uint64_t sub_base) {   // wave w owns keys [w*512, w*512+512) of the sub-tile, 64 at a time
#pragma unroll
        for (int it = 0; it < kItemsPerThread; ++it) {
            uint64_t idx = sub_base + (uint32_t)wv * kWaveChunk + (uint32_t)it * 64 + (uint32_t)lane;
            if (idx < n) dst[it] = in[idx];
        }
    };
    load(key, 0);
    for (uint64_t sub_base = 0; sub_base < n; sub_base += kSubTile) {
        uint32_t n_valid = (uint32_t)((n - sub_base) < (uint64_t)kSubTile ? (n - sub_base) : (uint64_t)kSubTile);
        // phase 1: rank inside the wave chunk: digit + peers of every key, then the wave's running counts round by round
        uint32_t dr[kItemsPerThread], cnt[kItemsPerThread];   // digit | rank-in-wave-chunk << BITS | valid << 31
        get_digits<W, kItemsPerThread, BIASED>(key, d, dr);
        if constexpr (STABLE) {
#pragma unroll
            for (int it = 0; it < kItemsPerThread; ++it) {
                uint32_t j = (uint32_t)wv * kWaveChunk + (uint32_t)it * 64 + (uint32_t)lane;
                bool valid = j < n_valid;
                uint32_t dg = valid ? dr[it] : 0u, rank;
                if constexpr (BITS > 8) wave_match_wide<BITS>(dg, valid, rank, cnt[it]);
                else wave_match(dg, d.bits, valid, rank, cnt[it]);
                dr[it] = dg | (rank << BITS) | ((uint32_t)valid << 31);
            }
#pragma unroll
            for (int it = 0; it < kItemsPerThread; ++it) {
                if (dr[it] >> 31) {
                    const uint32_t dg = dr[it] & kDigitMask, rank = (dr[it] >> BITS) & 0xFFu, prev = whist[dg];
                    if (rank == cnt[it] - 1) whist[dg] = (uint16_t)(prev + cnt[it]);   // highest peer lane publishes the new count
                    dr[it] += prev << BITS;
                }
                wave_lds_fence();
            }
        } else {
            uint32_t *const wh32 = reinterpret_cast<uint32_t *>(whist);      // two 16-bit counters per word: a wave's chunk holds <= 512 keys
#pragma unroll
            for (int it = 0; it < kItemsPerThread; ++it) {
                const uint32_t j = (uint32_t)wv * kWaveChunk + (uint32_t)it * 64 + (uint32_t)lane;
                const bool valid = j < n_valid;
                const uint32_t dg = valid ? dr[it] : 0u;
                uint32_t taken = 0;
                if (valid) taken = (atomicAdd(&wh32[dg >> 1], 1u << (16u * (dg & 1u))) >> (16u * (dg & 1u))) & 0xFFFFu;   // keys of the value before this one, in any order
                dr[it] = dg | (taken << BITS) | ((uint32_t)valid << 31);
            }
            wave_lds_fence();
        }
        if (kPrefetch && sub_base + kSubTile < n) load(nxt, sub_base + kSubTile);
        __syncthreads();
        // phase 2: per digit value (threads 0..255 = waves 0..3 at 8 bits): total over the waves, scan over the values, wave bases, global bases
        uint32_t tot = 0, inc = 0;
        if (wv < kValWaves) {
#pragma unroll
            for (int w = 0; w < kSortWaves; ++w) tot += sh.whist[w][tid];
            inc = wave_incl_scan(tot);
            if (lane == 63) sh.scratch[wv] = inc;
        }
        __syncthreads();
        if (wv < kValWaves) {
            uint32_t running = inc - tot;
            for (int w = 0; w < wv; ++w) running += sh.scratch[w];
            const uint64_t g = sh.gbase[tid];
            sh.gdelta[tid] = g - running;
            sh.gbase[tid] = g + tot;
#pragma unroll
            for (int w = 0; w < kSortWaves; ++w) { uint32_t c = sh.whist[w][tid]; sh.whist[w][tid] = (uint16_t)running; running += c; }
        }
        __syncthreads();
        // phase 3: place the keys in sorted order in LDS
#pragma unroll
        for (int it = 0; it < kItemsPerThread; ++it) {
            if (dr[it] >> 31) {
                const uint32_t pos = whist[dr[it] & kDigitMask] + ((dr[it] >> BITS) & (0x7FFFFFFFu >> BITS));
#pragma unroll
                for (int w = 0; w < W; ++w) sh.keys[pos].w[w] = key[it].w[w];
            }
        }
        __syncthreads();
        for (int i = lane; i < kVals; i += 64) whist[i] = 0;              // own row, read by this wave only since the last barrier
        // phase 4: stream the sorted sub-tile out; consecutive threads hit consecutive addresses inside a run
        if (kPrefetch) {
            Key<W> kk[kItemsPerThread];
            uint32_t dg[kItemsPerThread];
#pragma unroll
            for (int it = 0; it < kItemsPerThread; ++it) {
                uint32_t j = (uint32_t)it * kSortThreads + (uint32_t)tid;
                if (j < n_valid) kk[it] = sh.keys[j];
            }
            get_digits<W, kItemsPerThread, BIASED>(kk, d, dg);
            if constexpr (SIDE) {
                uint32_t dn[kItemsPerThread];
                get_digits<W, kItemsPerThread, BIASED>(kk, d_next, dn);
#pragma unroll
                for (int it = 0; it < kItemsPerThread; ++it) {
                    uint32_t j = (uint32_t)it * kSortThreads + (uint32_t)tid;
                    if (j < n_valid) {
                        const uint64_t to = sh.gdelta[dg[it]] + j;
                        out[to] = kk[it];
                        ss->bytes[(uint32_t)(to - ss->gtile[dg[it]])] = (SideEntry<NEXT_BITS>)dn[it];
                    }
                }
            } else {
#pragma unroll
                for (int it = 0; it < kItemsPerThread; ++it) {
                    uint32_t j = (uint32_t)it * kSortThreads + (uint32_t)tid;
                    if (j < n_valid) out[sh.gdelta[dg[it]] + j] = kk[it];
                }
            }
#pragma unroll
            for (int it = 0; it < kItemsPerThread; ++it) key[it] = nxt[it];
        } else {
#pragma unroll
            for (int it = 0; it < kItemsPerThread; ++it) {
                uint32_t j = (uint32_t)it * kSortThreads + (uint32_t)tid;
                if (j < n_valid) {
                    Key<W> kk = sh.keys[j];
                    const uint32_t dg = get_digit<W, BIASED>(kk, d);
                    const uint64_t to = sh.gdelta[dg] + j;
                    out[to] = kk;
                    if constexpr (SIDE) ss->bytes[(uint32_t)(to - ss->gtile[dg])] = (SideEntry<NEXT_BITS>)get_digit<W, BIASED>(kk, d_next);
                }
            }
            if (sub_base + kSubTile < n) load(key, sub_base + kSubTile);
        }
    }
}

// stable scatter of one 32768-key tile by the current digit
// What a key width supports: the staged keys, the tables of 1 << BITS digit values and (SIDE_BITS > 0) the tile's side entries of a
// SIDE_BITS-wide next digit must fit the 160 KB of LDS.  Side digits at all: W <= 7 key words.  Wide digits (9 bits with 16-bit side
// entries, 8 bits with 16-bit side entries): W = 2 and 3; every other key width, stage 1's W + 2 words among them, keeps 8-bit
// digits (W = 4 with 9 bits and 16-bit entries would come within 952 bytes of the 160 KB, the 1 KB of slack included: not built).
// 10 bits fit W = 3 without side entries only (98 KB; with them 176 KB), i.e. as a plan's last pass: 8 + 8 + 10 was measured equal
// to 8 + 9 + 9 and is not built (profiles/r08/build_wide/README.md).
template <int W, int BITS, int SIDE_BITS>
constexpr bool kScatterFits = sizeof(ScatterShared<W, BITS>) + (SIDE_BITS ? sizeof(SideShared<BITS, (SIDE_BITS ? SIDE_BITS : 8)>) : 0) + 1024 <= 160 * 1024;
template <int W> constexpr bool kSideFits = kScatterFits<W, 8, 8>;
template <int W> constexpr bool kWideFits = W >= 2 && W <= 3 && kSideFits<W> && kScatterFits<W, 9, 9> && kScatterFits<W, 8, 9>;
static_assert(kWideFits<3> && kWideFits<2> && !kWideFits<4> && !kScatterFits<3, 10, 9>, "DESIGN.md 5: the LDS bound of the wide scatter variants");

template <int W, bool BIASED, bool SIDE = false, bool STABLE = true, int BITS = 8, int NEXT_BITS = 8>
__global__ __launch_bounds__(kSortThreads, 4) void radix_scatter_kernel(const Key<W> *in, Key<W> *out, uint64_t n, Digit d,
                                                                      uint64_t n_tiles, const uint64_t *rowoff,
                                                                      const uint64_t *totals, SideEntry<NEXT_BITS> *side = nullptr,
                                                                      Digit d_next = Digit{0, 0, 0}) {
    constexpr int kVals = 1 << BITS;
    static_assert(kVals <= kSortThreads, "a thread per digit value");
    __shared__ ScatterShared<W, BITS> sh;
    __shared__ uint64_t s64[kSortThreads / 64 + 1];
    const int tid = threadIdx.x;
    // workgroups go to the 8 XCDs in turn: XCD x takes the x-th eighth of the tiles, so that the tiles that run side by side on one
    // L2 are neighbours (their runs of a digit value are adjacent in the output: lines shared by two tiles are completed in one L2)
    const uint32_t tile = xcd_tile(blockIdx.x, (uint32_t)n_tiles);
    // global base of every digit value for this tile = scan(totals)[digit] + rowoff[digit][tile]
    uint64_t t = tid < kVals ? totals[tid] : 0;
    uint64_t ex = block_excl_scan64<kSortThreads>(t, s64, nullptr);
    const uint64_t my_off = tid < kVals ? rowoff[(uint64_t)tid * n_tiles + tile] : 0;
    if (tid < kVals) sh.gbase[tid] = ex + my_off;
    const uint64_t tile_base = (uint64_t)tile * kBlockTile;
    if constexpr (SIDE) {
        __shared__ SideShared<BITS, NEXT_BITS> ss;
        // keys of the tile per digit value: the next tile's row offset (the row total behind the last tile) minus this tile's
        uint64_t c = 0;
        if (tid < kVals) c = (tile + 1 < n_tiles ? rowoff[(uint64_t)tid * n_tiles + tile + 1] : t) - my_off;
        __syncthreads();                                                 // s64 is free again
        const uint64_t place = block_excl_scan64<kSortThreads>(c, s64, nullptr);
        if (tid < kVals) {
            ss.toff[tid] = (uint32_t)place;
            ss.gtile[tid] = ex + my_off - place;
            if (tid == kVals - 1) ss.toff[kVals] = (uint32_t)(place + c);
        }
        __syncthreads();
        if (tile_base >= n) return;
        const uint64_t cnt = (n - tile_base) < (uint64_t)kBlockTile ? (n - tile_base) : (uint64_t)kBlockTile;
        scatter_subtiles<W, BIASED, true, STABLE, BITS, NEXT_BITS>(sh, in + tile_base, out, cnt, d, &ss, d_next);
        __syncthreads();
        // the tile's entries, run by run: a wave per 16 (32, 64) digit values, consecutive lanes consecutive entries
        const int lane = lane_id(), wv = wave_id();
        for (int v = wv * (kVals / kSortWaves); v < (wv + 1) * (kVals / kSortWaves); ++v) {
            const uint32_t from = ss.toff[v], len = ss.toff[v + 1] - from;
            SideEntry<NEXT_BITS> *to = side + ss.gtile[v] + from;
            for (uint32_t i = lane; i < len; i += 64) to[i] = ss.bytes[from + i];
        }
    } else {
        __syncthreads();
        if (tile_base >= n) return;
        const uint64_t cnt = (n - tile_base) < (uint64_t)kBlockTile ? (n - tile_base) : (uint64_t)kBlockTile;
        scatter_subtiles<W, BIASED, false, STABLE, BITS>(sh, in + tile_base, out, cnt, d);
    }
}

// The oversized route: segments longer than lds_cap keys (no LDS tile holds them) are split by their most significant digit not yet
// split on, level by level, until every piece fits a tile (lds_finish drives the levels).  A list entry is (first | buffer << 63,
// end): positions in the key array, and which of the two key buffers holds the keys (0: buf0, where the result belongs).
constexpr uint64_t kSegInOther = 1ull << 63;
struct SegList {
    uint64_t *first, *end;
    uint32_t *count;         // entries wanted (the host compares it with cap: beyond cap nothing is written)
    uint32_t cap;
};
struct SplitLists {
    SegList small, mid, next;   // SplitClass (segment_split.hpp)
    uint32_t *n_split;          // segments this level found longer than lds_cap
};

// One level: one workgroup per listed segment.  Census of digit d over the segment, exclusive scan, ONE stable scatter into the
// other key buffer; then one wave packs the pieces (the keys of a digit value, now contiguous) into the lists of the finishers and
// of the next level.  A segment whose keys all share the digit value stays where it is and goes to the next level as it is.  The
// launch never reads what it wrote.
template <int W>
__global__ __launch_bounds__(kSortThreads) void segment_split_kernel(Key<W> *buf0, Key<W> *buf1, const uint64_t *seg_first, const uint64_t *seg_end,
                                                                      Digit d, uint32_t local_tile, uint32_t lds_cap, SplitLists out) {
    __shared__ ScatterShared<W> sh;
    __shared__ uint64_t s64[kSortThreads / 64 + 1];
    __shared__ uint32_t s_cnt[256];
    __shared__ uint32_t e_meta[256];                                // class | index among the segment's ranges of that class << 2
    __shared__ uint32_t s_one;
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const uint64_t f = wave_uniform(seg_first[blockIdx.x]), s0 = f & ~kSegInOther, cnt = wave_uniform(seg_end[blockIdx.x]) - s0;
    if (cnt <= (uint64_t)lds_cap) return;                           // (level 0 lists every deferred segment: the shorter ones are sorted in LDS)
    const bool in_other = (f & kSegInOther) != 0;
    const Key<W> *x = (in_other ? buf1 : buf0) + s0;
    Key<W> *y = (in_other ? buf0 : buf1) + s0;
    if (tid < 256) s_cnt[tid] = 0;
    if (tid == 0) { s_one = 0; atomicAdd(out.n_split, 1u); }
    __syncthreads();
    for (uint64_t base = (uint64_t)wv * 64; base < cnt; base += kSortThreads) {   // (wave-uniform trip count)
        const uint64_t i = base + (uint64_t)lane;
        const bool valid = i < cnt;
        const uint32_t dg = valid ? get_digit<W>(x[i], d) : 0u;
        const uint32_t dg0 = wave_uniform(dg);                      // lane 0 is valid in every round
        const uint64_t vm = __ballot(valid);
        if (__ballot(valid && dg == dg0) == vm) {                   // hot k-mers: one add for the wave instead of 64 to one address
            if (lane == 0) atomicAdd(&s_cnt[dg0], (uint32_t)__popcll(vm));
        } else if (valid)
            atomicAdd(&s_cnt[dg], 1u);
    }
    __syncthreads();
    const uint64_t c = tid < 256 ? s_cnt[tid] : 0;
    if (c == cnt) s_one = 1;
    const uint64_t ex = block_excl_scan64<kSortThreads>(c, s64, nullptr);
    if (tid < 256) sh.gbase[tid] = ex;
    __syncthreads();
    auto append = [&](const SegList &l, uint32_t q, uint64_t first, uint64_t end) {
        if (q < l.cap) { l.first[q] = first; l.end[q] = end; }
    };
    if (s_one) {
        if (tid == 0) append(out.next, atomicAdd(out.next.count, 1u), f, s0 + cnt);
        return;
    }
    scatter_subtiles<W>(sh, x, y, cnt, d);
    __syncthreads();                                                // the scatter's tables are free: they hold the segment's ranges now
    if (wv != 0) return;
    uint64_t *const e_first = sh.gbase, *const e_end = sh.gdelta;   // at most one range per non-empty digit value
    // the pieces lie in y in digit order: pack them (wave-uniform walk over the counts, which lane v & 63 holds for value v)
    uint32_t cv[4], n_cls[kSplitClasses] = {0, 0, 0}, n_ent = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) cv[q] = s_cnt[q * 64 + lane];
    SplitPacker pk(s0, local_tile, lds_cap);
    auto emit = [&](uint32_t cls, uint64_t first, uint64_t end) {
        const uint32_t idx = cls == kSplitSmall ? n_cls[0]++ : (cls == kSplitMid ? n_cls[1]++ : n_cls[2]++);
        if (lane == 0) { e_first[n_ent] = first; e_end[n_ent] = end; e_meta[n_ent] = cls | (idx << 2); }
        ++n_ent;
    };
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int i = 0; i < 64; ++i) pk.step((uint32_t)__builtin_amdgcn_readlane((int)cv[q], i), emit);
    pk.finish(emit);
    uint32_t base[kSplitClasses] = {0, 0, 0};
    if (lane == 0) {
        if (n_cls[0]) base[0] = atomicAdd(out.small.count, n_cls[0]);
        if (n_cls[1]) base[1] = atomicAdd(out.mid.count, n_cls[1]);
        if (n_cls[2]) base[2] = atomicAdd(out.next.count, n_cls[2]);
    }
#pragma unroll
    for (int q = 0; q < kSplitClasses; ++q) base[q] = wave_uniform(base[q]);
    wave_lds_fence();
    const uint64_t where = in_other ? 0ull : kSegInOther;           // the pieces are in the buffer the segment was not in
    for (uint32_t e = lane; e < n_ent; e += 64) {
        const uint32_t cls = e_meta[e] & 3u, idx = e_meta[e] >> 2;
        const uint64_t first = e_first[e] | where, end = e_end[e];
        if (cls == kSplitSmall) append(out.small, base[0] + idx, first, end);
        else if (cls == kSplitMid) append(out.mid, base[1] + idx, first, end);
        else append(out.next, base[2] + idx, first, end);
    }
}

// what is still listed after the last level: runs of keys equal on every compared bit, finished as they stand.  Those that sit in
// the other buffer are copied to the result buffer.
template <int W>
__global__ __launch_bounds__(kSortThreads) void segment_copy_kernel(Key<W> *res, const Key<W> *other, const uint64_t *seg_first, const uint64_t *seg_end) {
    const uint64_t f = seg_first[blockIdx.x], s0 = f & ~kSegInOther, cnt = seg_end[blockIdx.x] - s0;
    if (!(f & kSegInOther)) return;
    for (uint64_t i = threadIdx.x; i < cnt; i += kSortThreads) res[s0 + i] = other[s0 + i];
}

// ---------------------------------------------------------------------------------------------
// 4b. segment-local finish.  After P global passes on the P most significant key bytes the array is
// partitioned into segments of equal 8P-bit prefix (in arbitrary inner order).  Each workgroup takes
// the whole segments that START in its stride of the array (<= LocalCfg<W>::kTile keys) and sorts
// them in LDS, so these keys cross HBM once more instead of once per remaining digit:
//   local_sort_kernel  two or three stable LSD passes in LDS (the 8 key bits below the prefix, then the rank of the
//                      segment inside the tile) leave runs of equal leading 8P+8 bits — a handful of keys unless the
//                      input is highly redundant; every key then finds its rank inside its run by comparing itself
//                      with the run's other keys and goes straight to its final place -- or, where the edge emission wants them
//                      (LocalPlan::info), to its place in the LDS tile first, so that every position can be compared with the one
//                      before it and leave with the emitter's info byte.
//   local_lsd_kernel   tiles whose runs are too long for that (reported by the first kernel), and single segments
//                      that did not fit a tile next to their neighbours: LSD passes in LDS over every remaining digit.
//   segment_lds_kernel   single segments of up to twice a tile: the same passes with the LDS of a whole CU.
//   segment_split_kernel (above)  longer segments: split by the highest digit below the prefix, one stable scatter per level into
//                      the other key buffer; the pieces are packed into ranges that the two kernels above finish (reading from the
//                      buffer the pieces are in, writing to the result buffer), pieces still longer than a tile go down a level.
// ---------------------------------------------------------------------------------------------
template <int W> struct LocalCfg {
    static constexpr int kTile = W <= 4 ? 4096 : 2048;           // keys sorted in LDS by one workgroup (LDS budget: kTile * 4W bytes)
    static constexpr int kIpt = kTile / kSortThreads;
    static constexpr int kChunk = kTile / kSortWaves;
};

// segments just too long for that tile still fit the LDS of a workgroup that has it to itself: twice the tile (one segment, no
// neighbours: segment_lds_kernel); 0 = no such tile for this key width
template <int W> struct BigCfg {
    static constexpr int kTile = W <= 4 ? 8192 : (W <= 8 ? 4096 : 0);
};

template <int W, int TILE = LocalCfg<W>::kTile>
struct LocalShared {
    Key<W> keys[TILE];
    uint16_t seg[TILE];
    uint16_t whist[kSortWaves][256];
    uint32_t start[256];
    uint32_t scratch[kSortThreads / 64 + 1];
    uint32_t wheads[kSortWaves + 1];
};

// LDS of local_sort_kernel: the tile, one 16-bit counter per (segment, upper digit) bin, head masks
template <int W>
struct CompareShared {
    // two workgroups per CU (80 KB each) where the keys leave room for >= 2048 counters, else one
    static constexpr int kRoom = (80 * 1024 - 1024 - LocalCfg<W>::kTile * 4 * W) / 2;
    static constexpr int kBins = kRoom >= 2048 ? (kRoom / 2048 * 2048 < 16384 ? kRoom / 2048 * 2048 : 16384) : 16384;
    static_assert(kBins >= LocalCfg<W>::kTile || kBins == 16384, "a bin per segment at least");
    Key<W> keys[LocalCfg<W>::kTile];
    uint32_t hist[kBins / 2];                                        // bin b: bits [16 (b & 1), +16) of word b >> 1
    uint32_t scratch[kSortThreads / 64 + 1];
    uint32_t flags[2];                                              // runs in the tile, "a run is too long"
    uint64_t masks[LocalCfg<W>::kTile / 64];                         // segment / run heads, one bit per key
};

template <int W>
__device__ __forceinline__ uint32_t key_prefix(const Key<W> &key, int T) { return T == 0 ? 0u : (key.w[0] >> (32 - T)); }   // leading T <= 32 bits

// What the edge emission (5.) takes from a sorted key and its predecessor: one definition for the emitter, the epilogue of
// local_sort_kernel and emit_info_range_kernel.
template <int W>
__device__ __forceinline__ bool keys_equal(const Key<W> &x, const Key<W> &y) {
    bool eq = true;
#pragma unroll
    for (int j = 0; j < W; ++j) eq = eq && (x.w[j] == y.w[j]);
    return eq;
}
template <int W>
__device__ __forceinline__ bool same_km1(const Key<W> &x, const Key<W> &y, int k) {   // IsDiffKMinusOneMer, s2.cpp:54-75
    int full = (k - 1) >> 4, rem = (k - 1) & 15;
    bool eq = true;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < full) eq = eq && (x.w[j] == y.w[j]);
        else if (j == full && rem > 0) eq = eq && ((x.w[j] >> (16 - rem) * 2) == (y.w[j] >> (16 - rem) * 2));
    }
    return eq;
}
template <int W>
__device__ __forceinline__ int key_a(const Key<W> &x, int k) {   // Extract_a, s2.cpp:83-94
    if ((x.w[W - 1] >> 3) & 1u) {
        int wi = (k - 1) >> 4, ci = (k - 1) & 15;
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < W; ++j) if (j == wi) word = x.w[j];
        return (word >> (15 - ci) * 2) & 3;
    }
    return kDollar;
}
template <int W>
__device__ __forceinline__ int key_b(const Key<W> &x) { return x.w[W - 1] & 7u; }   // Extract_b, s2.cpp:96-98

// the descriptor byte of a run (distinct key) whose first key is `cur`: a | b << 3 | group head << 6 | bucket head << 7
template <int W>
__device__ __forceinline__ uint8_t head_info(const Key<W> &cur, int k, bool ghead, bool bhead) {
    return (uint8_t)(key_a<W>(cur, k) | (key_b<W>(cur) << 3) | ((int)ghead << 6) | ((int)bhead << 7));
}
// the same for a key whose predecessor in the sorted array is `prv`; head: the key is the first of its run
template <int W>
__device__ __forceinline__ uint8_t key_info(const Key<W> &cur, const Key<W> &prv, int k, bool &head) {
    head = !keys_equal<W>(cur, prv);
    return head_info<W>(cur, k, !same_km1<W>(cur, prv, k), (cur.w[0] >> 16) != (prv.w[0] >> 16));
}
// The info array of a sort (one byte per key position, MGTA_EMIT_FUSED): the descriptor byte where the key is the first of its
// run, else this marker (a = 7; a run head has a <= 4)
constexpr uint8_t kInfoNoHead = 7;

// What the segment-local kernels need besides the keys (host-built, passed by value)
struct LocalPlan {
    const Digit *low_plan;   // every significant digit below the 8P-bit prefix, least significant first
    int n_low;
    int T;                   // bits of the prefix the global passes sorted on (8 per pass, + the leading zero bits a bucket sub-range skips)
    Digit upper;             // the (<= 8) key bits right below the prefix (inside the first two key words)
    uint32_t mask_last2;     // significant bits of key word W-2 / W-1 (stage 1 carries a payload there that must not be compared);
    uint32_t mask_last;      // the digits of low_plan never look at a masked-out bit
    uint32_t stride;         // keys of the array per workgroup of local_sort_kernel (multiple of 64, < kTile): a workgroup owns the segments
                             // that START in its stride; the rest of the tile is room for the last one to hang over
    uint64_t *lsd_list;      // [2 * lsd_cap]: (first, end) of the tiles left to local_lsd_kernel
    uint32_t *lsd_count;
    uint32_t lsd_cap;
    int debug;               // timing experiments only
    uint8_t *info;           // local_sort_kernel<W, true, true>: the info byte of every key position of the tiles it finishes (kInfoNoHead
    int emit_k;              // where no run starts), for the edge emission of a graph of this k; needs T <= 2 (k - 1) and unmasked keys
};

constexpr uint32_t kMaxAvgRun = 40;    // finish by comparison when the runs of equal (prefix, upper digit) are short on average ...
constexpr uint32_t kMaxRun = 256;      // ... and none of them is longer than this

// a < b on words FIRST..W-1, two words per comparison; MASKED: only the bits m2 / m1 of words W-2 / W-1 count
template <int W, int FIRST, bool MASKED>
__device__ __forceinline__ bool key_less(const Key<W> &a, const Key<W> &b, uint32_t m2, uint32_t m1) {
    bool lt = false;
    auto word = [&](const Key<W> &k, int j) {
        uint32_t x = k.w[j];
        if (MASKED && j == W - 1) x &= m1;
        if (MASKED && j == W - 2) x &= m2;
        return x;
    };
#pragma unroll
    for (int j = W - 1; j >= FIRST; j -= 2) {                          // least significant pair first
        if (j - 1 >= FIRST) {
            const uint64_t x = ((uint64_t)word(a, j - 1) << 32) | word(a, j), y = ((uint64_t)word(b, j - 1) << 32) | word(b, j);
            lt = x < y || (x == y && lt);
        } else {
            const uint32_t x = word(a, j), y = word(b, j);
            lt = x < y || (x == y && lt);
        }
    }
    return lt;
}

// loads the tile keys[first, first + nt) in (wave chunk, round, lane) order and ranks the segments inside the tile;
// returns the number of LSD passes the segment rank needs (0: one segment).  All threads call.
template <int W>
__device__ __forceinline__ int tile_load(LocalShared<W> &sh, const Key<W> *keys, uint64_t first, uint32_t nt, int T, Key<W> (&key)[LocalCfg<W>::kIpt],
                                         uint32_t (&seg)[LocalCfg<W>::kIpt]) {
    constexpr int kIpt = LocalCfg<W>::kIpt, kChunk = LocalCfg<W>::kChunk;
    const int lane = lane_id(), wv = wave_id();
    const uint64_t le_mask = lanemask_lt() | (1ull << lane);
    uint32_t running = 0;
#pragma unroll
    for (int it = 0; it < kIpt; ++it) {
        uint32_t j = (uint32_t)wv * kChunk + (uint32_t)it * 64 + (uint32_t)lane;
        bool valid = j < nt, head = false;
        if (valid) {
            key[it] = keys[first + j];
            head = j == 0 || key_prefix<W>(key[it], T) != key_prefix<W>(keys[first + j - 1], T);
        }
        uint64_t bal = __ballot(head);
        seg[it] = running + (uint32_t)__popcll(bal & le_mask);         // heads at positions <= j inside this wave chunk
        running += (uint32_t)__popcll(bal);
    }
    if (lane == 0) sh.wheads[wv] = running;
    __syncthreads();
    uint32_t before = 0, nseg = 0;
    for (int w = 0; w < kSortWaves; ++w) { uint32_t c = sh.wheads[w]; if (w < wv) before += c; nseg += c; }
    before = wave_uniform(before);
    nseg = wave_uniform(nseg);
#pragma unroll
    for (int it = 0; it < kIpt; ++it) seg[it] = seg[it] + before - 1;
    return nseg <= 1 ? 0 : (nseg <= 256 ? 1 : 2);
}

// one stable LSD pass over the tile: keys (+ segment ranks) go from registers (wave-chunk order) to their sorted LDS positions
// [0, nt); with `reload` they come back into registers in position order.  All threads call; every wave's row of sh.whist
// must be zero on entry (tile_zero_counts) and is zero again on return.  Four workgroup barriers.
template <int W, int TILE = LocalCfg<W>::kTile>
__device__ __forceinline__ void tile_zero_counts(LocalShared<W, TILE> &sh) {
    uint16_t *whist = sh.whist[wave_id()];
    for (int i = lane_id(); i < 256; i += 64) whist[i] = 0;             // wave-private: no barrier needed before the wave counts
}

template <int W, int TILE = LocalCfg<W>::kTile>
__device__ __forceinline__ void lds_pass(LocalShared<W, TILE> &sh, Key<W> (&key)[TILE / kSortThreads], uint32_t (&seg)[TILE / kSortThreads], uint32_t nt,
                                         Digit d, bool by_seg, int seg_shift, bool reload, uint32_t off = 0) {
    constexpr int kIpt = TILE / kSortThreads, kChunk = TILE / kSortWaves;
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    uint16_t *whist = sh.whist[wv];
    uint32_t dr[kIpt], cnt[kIpt];
    // digit + peers of every key first (independent work the compiler can interleave) ...
    if (by_seg) {
#pragma unroll
        for (int it = 0; it < kIpt; ++it) dr[it] = (seg[it] >> seg_shift) & 255u;
    } else {
        get_digits<W, kIpt>(key, d, dr);
    }
#pragma unroll
    for (int it = 0; it < kIpt; ++it) {
        uint32_t j = (uint32_t)wv * kChunk + (uint32_t)it * 64 + (uint32_t)lane;
        bool valid = j - off < nt;                                        // the registers hold positions [off, off + nt) of what was loaded
        uint32_t dg = valid ? dr[it] : 0u, rank;
        wave_match(dg, by_seg ? 8 : d.bits, valid, rank, cnt[it]);
        dr[it] = dg | (rank << 8) | ((uint32_t)valid << 31);
    }
    // ... then the wave's running counts, round by round (lane-to-lane hand-over through LDS)
#pragma unroll
    for (int it = 0; it < kIpt; ++it) {
        if (dr[it] >> 31) {
            const uint32_t dg = dr[it] & 255u, rank = (dr[it] >> 8) & 0xFFu, prev = whist[dg];
            if (rank == cnt[it] - 1) whist[dg] = (uint16_t)(prev + cnt[it]);
            dr[it] += prev << 8;
        }
        wave_lds_fence();
    }
    __syncthreads();
    // per digit value (threads 0..255 = waves 0..3): total over the waves, scan over the values, base of every wave
    uint32_t tot = 0, inc = 0;
    if (wv < 4) {
#pragma unroll
        for (int w = 0; w < kSortWaves; ++w) tot += sh.whist[w][tid];
        inc = wave_incl_scan(tot);
        if (lane == 63) sh.scratch[wv] = inc;
    }
    __syncthreads();
    if (wv < 4) {
        uint32_t running = inc - tot;
        for (int w = 0; w < wv; ++w) running += sh.scratch[w];
#pragma unroll
        for (int w = 0; w < kSortWaves; ++w) { uint32_t c = sh.whist[w][tid]; sh.whist[w][tid] = (uint16_t)running; running += c; }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kIpt; ++it) {
        if (dr[it] >> 31) {
            uint32_t pos = whist[dr[it] & 255u] + ((dr[it] >> 8) & 0x7FFFFFu);
            sh.keys[pos] = key[it];
            sh.seg[pos] = (uint16_t)seg[it];
        }
    }
    __syncthreads();
    tile_zero_counts<W, TILE>(sh);                                        // own row, read by this wave only since the last barrier
    if (reload) {
#pragma unroll
        for (int it = 0; it < kIpt; ++it) {
            uint32_t j = (uint32_t)wv * kChunk + (uint32_t)it * 64 + (uint32_t)lane;
            if (j < nt) { key[it] = sh.keys[j]; seg[it] = sh.seg[j]; }
        }
    }
}

// Last step of local_sort_kernel.  The tile lies in sh.keys sorted by (segment, upper digit): runs of equal leading
// `32 - run_shift` bits.  Run heads are balloted per 64-key window and the masks shared through LDS, so every key reads its
// run [rs, re) off a few masks; it then finds its rank among the run's keys by comparing words FIRST..W-1 (equal keys keep
// their order) and goes to its final place in global memory.  Returns false (nothing written) when the runs are longer than
// kMaxAvgRun on average or one of them is longer than kMaxRun.
// the leading PW words of a key as one integer (PW = 2: the run prefix reaches into the second word)
template <int W, int PW>
__device__ __forceinline__ uint64_t key_top(const Key<W> &k) {
    return PW == 1 ? (uint64_t)k.w[0] : (((uint64_t)k.w[0] << 32) | (uint64_t)k.w[W > 1 ? 1 : 0]);
}

template <int W, int FIRST, bool MASKED, int PW, bool INFO = false>   // INFO: see the epilogue (info, emit_k = the graph's k, emit_T = LocalPlan::T)
__device__ __forceinline__ bool finish_by_comparison(CompareShared<W> &sh, Key<W> *keys, uint64_t first, uint32_t nt, int run_bits, uint32_t m2,
                                                     uint32_t m1, bool skip_compare, uint8_t *info = nullptr, int emit_k = 0, int emit_T = 0) {
    const int run_shift = 32 * PW - run_bits;                          // runs = equal leading run_bits bits
    constexpr int kIpt = LocalCfg<W>::kIpt, kWindows = LocalCfg<W>::kTile / 64;
    const int lane = lane_id(), wv = wave_id();
    const uint64_t le_mask = lanemask_lt() | (1ull << lane);
    uint32_t heads = 0;
#pragma unroll
    for (int it = 0; it < kIpt; ++it) {
        const uint32_t win = (uint32_t)it * kSortWaves + (uint32_t)wv, j = win * 64 + (uint32_t)lane;
        const bool head = j < nt && (j == 0 || ((key_top<W, PW>(sh.keys[j - 1]) ^ key_top<W, PW>(sh.keys[j])) >> run_shift) != 0);
        const uint64_t hm = __ballot(head);
        if (lane == 0) sh.masks[win] = hm;
        heads += (uint32_t)__popcll(hm);
    }
    if (lane == 0 && heads) atomicAdd(&sh.flags[0], heads);
    __syncthreads();
    if (nt > wave_uniform(sh.flags[0]) * kMaxAvgRun) return false;
    uint32_t run[kIpt];                                               // rs | (re - rs) << 16
    bool over = false;
#pragma unroll
    for (int it = 0; it < kIpt; ++it) {
        const uint32_t win = (uint32_t)it * kSortWaves + (uint32_t)wv, j = win * 64 + (uint32_t)lane;
        run[it] = 0;
        if (j < nt) {
            const uint64_t hm = sh.masks[win];
            // last head at or before j: window 0 holds the head of key 0, so the walk back ends there at the latest
            uint64_t m = hm & le_mask;
            uint32_t w = win;
            while (m == 0 && win - w <= kMaxRun / 64) m = sh.masks[--w];
            const uint32_t rs = m ? w * 64 + 63u - (uint32_t)__clzll((long long)m) : j;
            over = over || m == 0;                                                 // no head within kMaxRun keys
            // first head behind j (masks beyond nt are 0: the last run ends with the tile)
            m = hm & ~le_mask;
            w = win;
            while (m == 0 && w + 1 < (uint32_t)kWindows && w - win <= kMaxRun / 64) m = sh.masks[++w];
            const uint32_t re = m ? w * 64 + (uint32_t)__ffsll((long long)m) - 1u : nt;
            over = over || re - rs > kMaxRun;
            run[it] = rs | ((re - rs) << 16);
        }
    }
    if (__ballot(over) && lane == 0) sh.flags[1] = 1;
    __syncthreads();
    if (wave_uniform(sh.flags[1])) return false;
    // place of key j (= mine) in the sorted tile
    auto place = [&](uint32_t j, uint32_t rn, const Key<W> &mine) {
        const uint32_t rs = rn & 0xFFFFu, re = rs + (rn >> 16);
        uint32_t r = j - rs;
        if (!skip_compare) {
            r = 0;
#pragma unroll 2
            for (uint32_t t = rs; t < j; ++t) r += key_less<W, FIRST, MASKED>(mine, sh.keys[t], m2, m1) ? 0u : 1u;
#pragma unroll 2
            for (uint32_t t = j + 1; t < re; ++t) r += key_less<W, FIRST, MASKED>(sh.keys[t], mine, m2, m1) ? 1u : 0u;
        }
        return rs + r;
    };
    if constexpr (!INFO) {
#pragma unroll
        for (int it = 0; it < kIpt; ++it) {
            const uint32_t j = ((uint32_t)it * kSortWaves + (uint32_t)wv) * 64 + (uint32_t)lane;
            if (j < nt) {
                const Key<W> mine = sh.keys[j];
                keys[first + place(j, run[it], mine)] = mine;
            }
        }
    } else {
        // The keys take their places inside the tile in LDS first; then every position reads its key and the one before it, and
        // the key leaves with its info byte (edge emission, 5.), both coalesced.  The tile starts a segment of equal leading T bits,
        // T <= 2 (k - 1): its first key starts a run and a group, and a bucket too when T < 16; else one word of the key before the
        // tile tells (whatever the workgroup that owns it has made of its tile by now: every key of that segment carries the same
        // leading T >= 16 bits).
        static_assert(!MASKED, "stage 1 emits no edges");
        Key<W> mine[kIpt];
#pragma unroll
        for (int it = 0; it < kIpt; ++it) {
            const uint32_t j = ((uint32_t)it * kSortWaves + (uint32_t)wv) * 64 + (uint32_t)lane;
            if (j < nt) {
                mine[it] = sh.keys[j];
                run[it] = place(j, run[it], mine[it]);
            }
        }
        __syncthreads();                                                  // the last read of the tile in run order
#pragma unroll
        for (int it = 0; it < kIpt; ++it) {
            const uint32_t j = ((uint32_t)it * kSortWaves + (uint32_t)wv) * 64 + (uint32_t)lane;
            if (j < nt) sh.keys[run[it]] = mine[it];
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kIpt; ++it) {
            const uint32_t j = ((uint32_t)it * kSortWaves + (uint32_t)wv) * 64 + (uint32_t)lane;
            if (j < nt) {
                const Key<W> cur = sh.keys[j];
                bool head = true;
                uint8_t byte;
                if (j == 0) {
                    const bool bhead = emit_T < 16 || first == 0 || (cur.w[0] >> 16) != (keys[first - 1].w[0] >> 16);
                    byte = head_info<W>(cur, emit_k, true, bhead);
                } else
                    byte = key_info<W>(cur, sh.keys[j - 1], emit_k, head);
                keys[first + j] = cur;
                info[first + j] = head ? byte : kInfoNoHead;
            }
        }
    }
    return true;
}

template <int W, bool WANT_KEYS, bool INFO = false>   // !WANT_KEYS: only the tile bounds are wanted (every tile goes to local_lsd_kernel)
__global__ __launch_bounds__(kSortThreads, 8) void local_sort_kernel(Key<W> *keys, uint64_t n, LocalPlan lp, uint64_t *big, uint32_t *big_count,
                                                                     uint32_t big_cap) {
    constexpr int kTile = LocalCfg<W>::kTile, kIpt = LocalCfg<W>::kIpt, kChunk = LocalCfg<W>::kChunk, kWindows = kTile / 64;
    constexpr uint32_t NONE = ~0u;
    static_assert(kWindows <= 64, "tile bounds are read off one 64-bit head mask per lane");
    const uint32_t kLocalStride = lp.stride;
    __shared__ CompareShared<W> sh;
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id(), T = lp.T;
    const uint64_t lo = (uint64_t)blockIdx.x * kLocalStride;
    const uint32_t loaded = (uint32_t)(n - lo < (uint64_t)kTile ? n - lo : (uint64_t)kTile);   // the window [lo, lo + loaded)
    constexpr bool want_keys = WANT_KEYS;
    if (tid == 0) { sh.flags[0] = 0; sh.flags[1] = 0; }
    // 1. one read of the window, in (wave chunk, round, lane) order; segment heads balloted per 64 keys
    Key<W> key[kIpt];
    uint32_t seg[kIpt];
    uint32_t carry = 0;
#pragma unroll
    for (int it = 0; it < kIpt; ++it) {
        const uint32_t j = (uint32_t)wv * kChunk + (uint32_t)it * 64 + (uint32_t)lane;
        const bool inw = j < loaded;
        uint32_t p = 0;
        if (inw) {
            if (want_keys) key[it] = keys[lo + j];
            else key[it].w[0] = keys[lo + j].w[0];
            p = key_prefix<W>(key[it], T);
        }
        uint32_t pp = __shfl_up(p, 1, 64);
        if (lane == 0) pp = it == 0 ? ((inw && lo + j > 0) ? key_prefix<W>(keys[lo + j - 1], T) : 0u) : carry;
        carry = __shfl(p, 63, 64);
        const uint64_t hm = __ballot(inw && (lo + j == 0 || p != pp));
        if (lane == 0) sh.masks[wv * kIpt + it] = hm;                 // window m = positions [64m, 64m + 64)
    }
    __syncthreads();
    // 2. the tile: from the first head in the stride to the first head behind it (every wave computes the same scalars)
    const uint64_t hmask = lane < kWindows ? sh.masks[lane] : 0ull;
    const bool in_stride = (uint32_t)lane < kLocalStride / 64;
    const uint32_t first_off = wave_uniform(wave_min(in_stride && hmask ? (uint32_t)lane * 64 + (uint32_t)__ffsll((long long)hmask) - 1u : NONE));
    if (first_off == NONE) return;                                    // the stride lies inside one long segment
    uint32_t end_off = wave_uniform(wave_min(!in_stride && hmask ? (uint32_t)lane * 64 + (uint32_t)__ffsll((long long)hmask) - 1u : NONE));
    if (end_off == NONE) {
        if (lo + loaded == n) end_off = loaded;
        else {                                                        // the last segment starting here does not fit: deferred
            end_off = wave_uniform(wave_max(in_stride && hmask ? (uint32_t)lane * 64 + 63u - (uint32_t)__clzll((long long)hmask) : 0u));
            if (tid == 0) {
                uint32_t q = atomicAdd(big_count, 1u);
                if (q < big_cap) big[q] = lo + end_off;
            }
        }
    }
    const uint32_t nt = end_off - first_off;
    if (nt == 0) return;
    const uint64_t first = lo + first_off;
    auto leave_to_lsd = [&]() {
        if (tid == 0) {
            uint32_t q = atomicAdd(lp.lsd_count, 1u);
            if (q < lp.lsd_cap) { lp.lsd_list[2 * q] = first; lp.lsd_list[2 * q + 1] = lo + end_off; }
        }
    };
    if (!want_keys) { leave_to_lsd(); return; }
    // rank of every key's segment inside the tile: heads in [first_off, its position]
    uint32_t nseg;
    {
        uint64_t in_tile = hmask;                                     // heads of window `lane` inside [first_off, end_off)
        const uint32_t w0 = (uint32_t)lane * 64;
        if (w0 + 64 <= first_off || w0 >= end_off) in_tile = 0;
        else {
            if (first_off > w0) in_tile &= ~0ull << (first_off - w0);
            if (end_off < w0 + 64) in_tile &= ~0ull >> (w0 + 64 - end_off);
        }
        const uint32_t c = (uint32_t)__popcll(in_tile), inc = wave_incl_scan(c);
        nseg = wave_uniform((uint32_t)__shfl(inc, 63, 64));
        const uint64_t le_mask = lanemask_lt() | (1ull << lane);
#pragma unroll
        for (int it = 0; it < kIpt; ++it) {
            const int m = wv * kIpt + it;
            const uint32_t before = (uint32_t)__shfl(inc - c, m, 64);
            const uint64_t mm = (uint64_t)__shfl((unsigned long long)in_tile, m, 64);
            seg[it] = before + (uint32_t)__popcll(mm & le_mask) - 1u;       // only read for positions inside the tile
        }
    }
    if (lp.debug & 2) return;
    // 3. one counting pass on (segment rank, upper digit): the order inside a bin is left to step 4, so plain LDS atomics rank the keys.
    //    The digit shrinks when the tile holds many (then short) segments: nseg << ub bins fit the counter array.
    constexpr int kBins = CompareShared<W>::kBins, kWordsPerThread = kBins / 2 / kSortThreads;
    int ub = 31 - __clz((int)((uint32_t)kBins / nseg));
    if (ub > lp.upper.bits) ub = lp.upper.bits;
    const uint32_t n_words = ((nseg << ub) + 1u) >> 1;
    for (uint32_t i = tid; i < n_words; i += kSortThreads) sh.hist[i] = 0;
    __syncthreads();
    const int run_bits = T + ub;                                       // <= 40: the digit may reach into the second key word
    uint32_t br[kIpt];                                                // bin | rank inside the bin << 16
#pragma unroll
    for (int it = 0; it < kIpt; ++it) {
        const uint32_t j = (uint32_t)wv * kChunk + (uint32_t)it * 64 + (uint32_t)lane;
        br[it] = ~0u;
        if (j - first_off < nt) {
            const uint32_t dg = ub ? (uint32_t)((key_top<W, 2>(key[it]) << T) >> (64 - ub)) : 0u;
            const uint32_t bin = (seg[it] << ub) | dg, sh16 = (bin & 1u) * 16u;
            const uint32_t old = atomicAdd(&sh.hist[bin >> 1], 1u << sh16);
            br[it] = bin | (((old >> sh16) & 0xFFFFu) << 16);
        }
    }
    __syncthreads();
    {   // exclusive scan of the counters, in place (a tile holds <= 4096 keys: 16 bits never overflow)
        uint32_t wds[kWordsPerThread], run = 0;
#pragma unroll
        for (int i = 0; i < kWordsPerThread; ++i) {
            const uint32_t wi = (uint32_t)tid * kWordsPerThread + i;
            const uint32_t x = wi < n_words ? sh.hist[wi] : 0u;
            wds[i] = run | ((run + (x & 0xFFFFu)) << 16);
            run += (x & 0xFFFFu) + (x >> 16);
        }
        const uint32_t base = block_excl_scan<kSortThreads>(run, sh.scratch, nullptr);
#pragma unroll
        for (int i = 0; i < kWordsPerThread; ++i) {
            const uint32_t wi = (uint32_t)tid * kWordsPerThread + i;
            if (wi < n_words) sh.hist[wi] = wds[i] + base * 0x00010001u;
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kIpt; ++it) {
        if (br[it] != ~0u) {
            const uint32_t bin = br[it] & 0xFFFFu;
            const uint32_t pos = ((sh.hist[bin >> 1] >> ((bin & 1u) * 16u)) & 0xFFFFu) + (br[it] >> 16);
#pragma unroll
            for (int w = 0; w < W; ++w) sh.keys[pos].w[w] = key[it].w[w];
        }
    }
    __syncthreads();
    if (lp.debug & 4) return;
    // 4. runs of equal (prefix, upper digit): every key ranks itself inside its run
    const bool skip = (lp.debug & 1) != 0;
    const bool masked = (lp.mask_last2 & lp.mask_last) != ~0u;
    bool done;
    if constexpr (INFO) {                                             // (the host asks for info bytes of unmasked keys only)
        if (run_bits > 32 && W > 1)
            done = finish_by_comparison<W, (W > 1 ? 1 : 0), false, 2, true>(sh, keys, first, nt, run_bits, ~0u, ~0u, skip, lp.info, lp.emit_k, T);
        else if (run_bits == 32 && W > 1)
            done = finish_by_comparison<W, (W > 1 ? 1 : 0), false, 1, true>(sh, keys, first, nt, run_bits, ~0u, ~0u, skip, lp.info, lp.emit_k, T);
        else
            done = finish_by_comparison<W, 0, false, 1, true>(sh, keys, first, nt, run_bits, ~0u, ~0u, skip, lp.info, lp.emit_k, T);
    } else if (run_bits > 32 && W > 1)
        done = masked ? finish_by_comparison<W, (W > 1 ? 1 : 0), true, 2>(sh, keys, first, nt, run_bits, lp.mask_last2, lp.mask_last, skip)
                      : finish_by_comparison<W, (W > 1 ? 1 : 0), false, 2>(sh, keys, first, nt, run_bits, lp.mask_last2, lp.mask_last, skip);
    else if (run_bits == 32 && W > 1)
        done = masked ? finish_by_comparison<W, (W > 1 ? 1 : 0), true, 1>(sh, keys, first, nt, run_bits, lp.mask_last2, lp.mask_last, skip)
                      : finish_by_comparison<W, (W > 1 ? 1 : 0), false, 1>(sh, keys, first, nt, run_bits, lp.mask_last2, lp.mask_last, skip);
    else
        done = masked ? finish_by_comparison<W, 0, true, 1>(sh, keys, first, nt, run_bits, lp.mask_last2, lp.mask_last, skip)
                      : finish_by_comparison<W, 0, false, 1>(sh, keys, first, nt, run_bits, lp.mask_last2, lp.mask_last, skip);
    if (!done) leave_to_lsd();                                        // global memory still holds the tile as it was
}

// one workgroup per listed range [start[b], end[b]) of whole segments (<= kTile keys, longer ones are skipped: the oversized route):
// stable LSD passes in LDS over every significant digit below the prefix, then the segment rank.  A range whose start carries
// kSegInOther (a packed range of the oversized route) is read from `other` instead of `keys`; the result always goes to `keys`.
template <int W>
__global__ __launch_bounds__(kSortThreads, 8) void local_lsd_kernel(Key<W> *keys, const Key<W> *other, const uint64_t *start, const uint64_t *end,
                                                                    int stride, LocalPlan lp) {
    constexpr int kIpt = LocalCfg<W>::kIpt;
    __shared__ LocalShared<W> sh;
    const int tid = threadIdx.x;
    const uint64_t f = wave_uniform(start[(uint64_t)blockIdx.x * stride]), first = f & ~kSegInOther;
    const uint64_t cnt = wave_uniform(end[(uint64_t)blockIdx.x * stride]) - first;
    if (cnt > (uint64_t)LocalCfg<W>::kTile || cnt == 0) return;
    const uint32_t nt = (uint32_t)cnt;
    const Key<W> *in = (f & kSegInOther) ? other : keys;
    Key<W> key[kIpt];
    uint32_t seg[kIpt];
    const int n_seg_pass = tile_load<W>(sh, in, first, nt, lp.T, key, seg);
    const int n_pass = lp.n_low + n_seg_pass;
    tile_zero_counts<W>(sh);
    for (int pass = 0; pass < n_pass; ++pass) {
        const bool by_seg = pass >= lp.n_low;
        Digit d;
        d.pos = 0; d.bits = 8; d.bias = 0;
        if (!by_seg) d = lp.low_plan[pass];
        lds_pass<W>(sh, key, seg, nt, d, by_seg, by_seg ? 8 * (pass - lp.n_low) : 0, pass + 1 < n_pass);
    }
    // write back (coalesced); n_low >= 1, so LDS holds the result
#pragma unroll
    for (int it = 0; it < kIpt; ++it) {
        uint32_t j = (uint32_t)it * kSortThreads + (uint32_t)tid;
        if (j < nt) keys[first + j] = sh.keys[j];
    }
}

// one workgroup per listed segment of LocalCfg::kTile < keys <= BigCfg::kTile: the same LSD passes with the LDS of a whole CU (a
// hot 16-mer prefix of 5-8 thousand keys took eight global census + scatter round trips of ~100 us each); `other` as in local_lsd_kernel
template <int W>
__global__ __launch_bounds__(kSortThreads) void segment_lds_kernel(Key<W> *keys, const Key<W> *other, const uint64_t *start, const uint64_t *end,
                                                                    LocalPlan lp) {
    constexpr int TILE = BigCfg<W>::kTile > 0 ? BigCfg<W>::kTile : LocalCfg<W>::kTile, kIpt = TILE / kSortThreads, kChunk = TILE / kSortWaves;
    __shared__ LocalShared<W, TILE> sh;
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const uint64_t f = wave_uniform(start[blockIdx.x]), first = f & ~kSegInOther, cnt = wave_uniform(end[blockIdx.x]) - first;
    if (cnt <= (uint64_t)LocalCfg<W>::kTile || cnt > (uint64_t)BigCfg<W>::kTile) return;
    const uint32_t nt = (uint32_t)cnt;
    const Key<W> *in = (f & kSegInOther) ? other : keys;
    Key<W> key[kIpt];
    uint32_t seg[kIpt];
#pragma unroll
    for (int it = 0; it < kIpt; ++it) {
        const uint32_t j = (uint32_t)wv * kChunk + (uint32_t)it * 64 + (uint32_t)lane;
        seg[it] = 0;
        if (j < nt) key[it] = in[first + j];
    }
    tile_zero_counts<W, TILE>(sh);
    for (int pass = 0; pass < lp.n_low; ++pass) lds_pass<W, TILE>(sh, key, seg, nt, lp.low_plan[pass], false, 0, pass + 1 < lp.n_low);
#pragma unroll
    for (int it = 0; it < kIpt; ++it) {                                  // n_low >= 1: LDS holds the result
        const uint32_t j = (uint32_t)it * kSortThreads + (uint32_t)tid;
        if (j < nt) keys[first + j] = sh.keys[j];
    }
}

// first segment head after `start` (end of a big segment): one workgroup per big segment
template <int W>
__global__ __launch_bounds__(256) void segment_end_kernel(const Key<W> *keys, uint64_t n, int T, const uint64_t *big, uint64_t *big_end) {
    __shared__ unsigned long long s_end;
    const uint64_t start = big[blockIdx.x];
    const uint32_t pre = key_prefix<W>(keys[start], T);
    if (threadIdx.x == 0) s_end = ~0ull;
    __syncthreads();
    for (uint64_t base = start + 1; base < n; base += 256 * 16) {
        unsigned long long found = ~0ull;
        for (int i = 0; i < 16; ++i) {
            uint64_t idx = base + (uint64_t)i * 256 + threadIdx.x;
            if (idx < n && key_prefix<W>(keys[idx], T) != pre && (unsigned long long)idx < found) found = idx;
        }
        if (found != ~0ull) atomicMin(&s_end, found);
        __syncthreads();
        if (s_end != ~0ull) break;
    }
    __syncthreads();
    if (threadIdx.x == 0) big_end[blockIdx.x] = s_end == ~0ull ? n : s_end;
}

// ---------------------------------------------------------------------------------------------
// 5. edge emission
// ---------------------------------------------------------------------------------------------
constexpr int kEmitThreads = 256;
constexpr int kEmitPerThread = 16;
constexpr int kEmitTile = kEmitThreads * kEmitPerThread;   // 4096 sorted keys per workgroup
// (keys_equal, same_km1, key_a, key_b, key_info: with the segment-local finish above, whose epilogue shares them)

// Where the runs start: the low 32 bits per run, the full 64 bits for every kRunBaseStep-th run.  Runs are consecutive, so a
// length is a 32-bit difference (a run never holds 2^32 keys) and a full start is rebuilt from the nearest base.
constexpr int kRunBaseStepLog = 10;
struct RunStarts {
    uint32_t *lo;                // [m]
    uint64_t *base;              // [m >> kRunBaseStepLog + 1]
};
__device__ __forceinline__ uint64_t run_full_start(const RunStarts &r, uint64_t s) {
    const uint64_t b = r.base[s >> kRunBaseStepLog];
    return b + (uint32_t)(r.lo[s] - (uint32_t)b);
}
__device__ __forceinline__ uint64_t run_length(const RunStarts &r, uint64_t s, uint64_t m, uint64_t n_items) {
    return s + 1 < m ? (uint64_t)(uint32_t)(r.lo[s + 1] - r.lo[s]) : n_items - run_full_start(r, s);
}

// E1+E2: one descriptor per run (distinct key): start index + (a | b<<3 | group_head<<6 | bucket_head<<7), compacted in key order.
// The keys are read once: the number of runs before a tile comes from a chained scan across the workgroups (device_utils.hpp).
struct EmitChain {
    unsigned long long *state;   // [n_tiles], zeroed
    uint32_t *ticket;            // zeroed
    uint32_t *error;
    unsigned long long *total;   // number of runs, written by the last tile
    unsigned long long *dollar;  // [kDollarSlots], zeroed: the runs whose a is $ (an upper bound of the tips), summed by the host
};
constexpr int kDollarSlots = 64; // one atomic per workgroup, spread over this many addresses
// all threads of the workgroup call once (two barriers): mine = the heads with a = $ this thread saw
__device__ __forceinline__ void count_dollar_heads(const EmitChain &chain, uint32_t tile, uint32_t mine, uint32_t *s_sum) {
    if (threadIdx.x == 0) *s_sum = 0;
    __syncthreads();
    mine = wave_sum(mine);
    if (lane_id() == 0 && mine) atomicAdd(s_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0 && *s_sum) atomicAdd(&chain.dollar[tile % kDollarSlots], (unsigned long long)*s_sum);
}

// TICKET = false numbers the tiles by blockIdx (workgroups are dispatched in that order on this hardware, which nothing guarantees):
// if a tile ever waits in vain the bounded walk raises chain.error and the host repeats the launch with TICKET = true.
template <int W, bool TICKET>
__global__ __launch_bounds__(kEmitThreads) void emit_compact_kernel(const Key<W> *keys, uint64_t n, int k, EmitChain chain, uint32_t n_tiles,
                                                                     RunStarts sub_start, uint8_t *sub_info) {
    __shared__ uint32_t s_cnt[kEmitPerThread * (kEmitThreads / 64)];
    __shared__ uint32_t s_scr[kEmitThreads / 64 + 1];
    __shared__ uint32_t s_tile, s_dollar;
    __shared__ unsigned long long s_base;
    const uint32_t tile = TICKET ? chain_ticket(chain.ticket, &s_tile) : blockIdx.x;
    uint64_t base = (uint64_t)tile * kEmitTile;
    const int lane = lane_id(), wv = wave_id();
    uint32_t headbits = 0, n_dollar = 0;
    uint32_t rank_in_wave[kEmitPerThread];
    uint8_t info[kEmitPerThread];
#pragma unroll
    for (int it = 0; it < kEmitPerThread; ++it) {
        uint64_t idx = base + (uint64_t)it * kEmitThreads + threadIdx.x;
        bool head = false;
        info[it] = 0;
        if (idx < n) {
            Key<W> cur = keys[idx];
            if (idx == 0) {
                head = true;
                info[it] = head_info<W>(cur, k, true, true);
            } else
                info[it] = key_info<W>(cur, keys[idx - 1], k, head);     // (taking it from the neighbouring lane by a shuffle was slower: 9.3 -> 11.2 ms)
        }
        uint64_t bal = __ballot(head);
        rank_in_wave[it] = (uint32_t)__popcll(bal & lanemask_lt());
        headbits |= (uint32_t)head << it;
        if (lane == 0) s_cnt[it * (kEmitThreads / 64) + wv] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    // exclusive scan of the 64 (iteration, wave) counts: order of keys = iteration-major, wave, lane
    uint32_t v = threadIdx.x < kEmitPerThread * (kEmitThreads / 64) ? s_cnt[threadIdx.x] : 0, tile_total = 0;
    uint32_t ex = block_excl_scan<kEmitThreads>(v, s_scr, &tile_total);
    __syncthreads();
    if (threadIdx.x < kEmitPerThread * (kEmitThreads / 64)) s_cnt[threadIdx.x] = ex;
    if (wv == 0) {
        const uint64_t before = chain_exclusive(chain.state, tile, tile_total, chain.error);
        if (lane == 0) {
            s_base = before;
            if (tile + 1 == n_tiles) *chain.total = before + tile_total;
        }
    }
    __syncthreads();
    uint64_t tb = s_base;
#pragma unroll
    for (int it = 0; it < kEmitPerThread; ++it) {
        if ((headbits >> it) & 1u) {
            uint64_t idx = base + (uint64_t)it * kEmitThreads + threadIdx.x;
            uint64_t s = tb + s_cnt[it * (kEmitThreads / 64) + wv] + rank_in_wave[it];
            sub_start.lo[s] = (uint32_t)idx;
            if ((s & ((1u << kRunBaseStepLog) - 1)) == 0) sub_start.base[s >> kRunBaseStepLog] = idx;
            sub_info[s] = info[it];
            n_dollar += (info[it] & 7) == kDollar;
        }
    }
    count_dollar_heads(chain, tile, n_dollar, &s_dollar);
}

// The same compaction from the info array the sort left behind (one byte per key position, kInfoNoHead where no run starts): the
// keys are not read.  A workgroup takes kInfoRounds rounds of kEmitTile positions, 16 per lane and round in one 16-byte load, all
// loads first; one chained scan per workgroup; the descriptors of a round are collected in LDS and leave as one coalesced run.
// (One round per workgroup and every lane storing its own descriptors took 20.8 ms per 7.2 G positions: 1.76 M workgroups, each a
// chain of load, scan, look-back and scattered stores.)  Order of the positions of a tile: round, thread, byte.  The array holds at
// least 16 bytes behind position n - 1 (SortJob::side_bytes).
constexpr int kInfoRounds = 8;
constexpr int kInfoTile = kEmitTile * kInfoRounds;         // 32768 positions per workgroup
template <bool TICKET>
__global__ __launch_bounds__(kEmitThreads) void emit_compact_info_kernel(const uint8_t *info_in, uint64_t n, EmitChain chain, uint32_t n_tiles,
                                                                          RunStarts sub_start, uint8_t *sub_info) {
    static_assert(kEmitPerThread == 16, "one 16-byte load per lane and round");
    static_assert(kInfoRounds == 8 && kEmitTile <= 65535, "round counts are scanned as 2 x 4 fields of 16 bits");
    __shared__ uint64_t s_scr[kEmitThreads / 64 + 1];
    __shared__ uint32_t s_tile, s_dollar;
    __shared__ unsigned long long s_base;
    __shared__ uint16_t s_off[kEmitTile];                  // the descriptors of a round: position inside the round, info byte
    __shared__ uint8_t s_inf[kEmitTile];
    const uint32_t tile = TICKET ? chain_ticket(chain.ticket, &s_tile) : blockIdx.x;
    const uint64_t base = (uint64_t)tile * kInfoTile;
    const uint32_t mine = threadIdx.x * kEmitPerThread;    // first position of the lane inside a round
    uint4 v[kInfoRounds];
#pragma unroll
    for (int r = 0; r < kInfoRounds; ++r) {
        const uint64_t idx0 = base + (uint64_t)r * kEmitTile + mine;
        v[r] = make_uint4(0, 0, 0, 0);
        if (idx0 < n) v[r] = *reinterpret_cast<const uint4 *>(info_in + idx0);
    }
    uint32_t headbits[kInfoRounds];
    uint64_t packed[2] = {0, 0};                           // heads of the lane per round, 16 bits each
#pragma unroll
    for (int r = 0; r < kInfoRounds; ++r) {
        const uint64_t idx0 = base + (uint64_t)r * kEmitTile + mine;
        const uint32_t left = idx0 < n ? (uint32_t)(n - idx0 < (uint64_t)kEmitPerThread ? n - idx0 : (uint64_t)kEmitPerThread) : 0u;
        const uint32_t wd[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
        uint32_t hb = 0;
#pragma unroll
        for (int b = 0; b < kEmitPerThread; ++b) hb |= (uint32_t)(((wd[b >> 2] >> (8 * (b & 3))) & 7u) != (uint32_t)kInfoNoHead) << b;
        headbits[r] = hb & ((1u << left) - 1u);            // (left <= 16)
        packed[r >> 2] |= (uint64_t)__popc(headbits[r]) << (16 * (r & 3));
    }
    uint64_t ex[2], tot[2];
    ex[0] = block_excl_scan64<kEmitThreads>(packed[0], s_scr, &tot[0]);
    ex[1] = block_excl_scan64<kEmitThreads>(packed[1], s_scr, &tot[1]);
    uint32_t round_total[kInfoRounds], round_first[kInfoRounds], tile_total = 0;
#pragma unroll
    for (int r = 0; r < kInfoRounds; ++r) {
        round_total[r] = (uint32_t)(tot[r >> 2] >> (16 * (r & 3))) & 0xFFFFu;
        round_first[r] = tile_total;
        tile_total += round_total[r];
    }
    if (wave_id() == 0) {
        const uint64_t before = chain_exclusive(chain.state, tile, tile_total, chain.error);
        if (lane_id() == 0) {
            s_base = before;
            if (tile + 1 == n_tiles) *chain.total = before + tile_total;
        }
    }
    uint64_t tb = 0;
    uint32_t n_dollar = 0;
#pragma unroll
    for (int r = 0; r < kInfoRounds; ++r) {
        if (round_total[r] == 0) continue;                 // (workgroup-uniform)
        const uint32_t wd[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
        uint32_t q = (uint32_t)(ex[r >> 2] >> (16 * (r & 3))) & 0xFFFFu;
#pragma unroll
        for (int b = 0; b < kEmitPerThread; ++b) {
            if ((headbits[r] >> b) & 1u) {
                s_off[q] = (uint16_t)(mine + (uint32_t)b);
                s_inf[q] = (uint8_t)((wd[b >> 2] >> (8 * (b & 3))) & 255u);
                ++q;
            }
        }
        __syncthreads();                                   // the round's descriptors are staged (the first time: s_base is known)
        tb = s_base;
        const uint64_t out0 = tb + round_first[r], pos0 = base + (uint64_t)r * kEmitTile;
        for (uint32_t i = threadIdx.x; i < round_total[r]; i += kEmitThreads) {
            const uint64_t s = out0 + i, idx = pos0 + s_off[i];
            sub_start.lo[s] = (uint32_t)idx;
            if ((s & ((1u << kRunBaseStepLog) - 1)) == 0) sub_start.base[s >> kRunBaseStepLog] = idx;
            const uint8_t inf = s_inf[i];
            sub_info[s] = inf;
            n_dollar += (inf & 7) == kDollar;
        }
        __syncthreads();                                   // the stage is free again
    }
    count_dollar_heads(chain, tile, n_dollar, &s_dollar);
}

// MGTA_EMIT_FUSED=2: the m run descriptors of emit_compact_info_kernel against those of emit_compact_kernel (bad[0]: starts, bad[1]: info bytes)
__global__ __launch_bounds__(256) void emit_check_kernel(const uint32_t *lo, const uint8_t *info, const uint32_t *lo_ref, const uint8_t *info_ref, uint64_t m,
                                                         uint32_t *bad) {
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < m; s += (uint64_t)gridDim.x * 256) {
        if (lo[s] != lo_ref[s]) atomicAdd(&bad[0], 1u);
        if (info[s] != info_ref[s]) atomicAdd(&bad[1], 1u);
    }
}

// The info bytes of the key ranges local_sort_kernel did not finish itself (the tiles left to local_lsd_kernel, the deferred
// segments): one workgroup per listed range [start[b * stride], end[b * stride]) of the sorted array, every key against its
// predecessor -- the first of the range included: a range may start inside a group or a bucket.
template <int W>
__global__ __launch_bounds__(256) void emit_info_range_kernel(const Key<W> *keys, uint64_t n, int k, const uint64_t *start, const uint64_t *end, int stride,
                                                              uint8_t *key_info_out) {
    const uint64_t first = start[(uint64_t)blockIdx.x * stride] & ~kSegInOther;
    uint64_t last = end[(uint64_t)blockIdx.x * stride];
    if (last > n) last = n;
    for (uint64_t i = first + threadIdx.x; i < last; i += 256) {
        const Key<W> cur = keys[i];
        bool head = true;
        const uint8_t info = i == 0 ? head_info<W>(cur, k, true, true) : key_info<W>(cur, keys[i - 1], k, head);
        key_info_out[i] = head ? info : kInfoNoHead;
    }
}

// E3: decide every run (sub-group): the rules of output_(), cx1_read2sdbg_s2.cpp:763-834.
// rec = w | last<<4 | tip<<5 | min(mult,255)<<8, or 0xFFFF when the run is suppressed.
constexpr int kDecideThreads = 256;
constexpr int kDecidePerThread = 4;
constexpr int kDecideTile = kDecideThreads * kDecidePerThread;   // 1024 runs per workgroup
constexpr int kDecideHalo = 32;

__device__ __forceinline__ bool run_suppressed(int a, int b, int has_a, int has_b) {
    return (a == kDollar && ((has_b >> b) & 1)) || (b == kDollar && ((has_a >> a) & 1));
}

__global__ __launch_bounds__(kDecideThreads) void emit_decide_kernel(RunStarts sub_start, const uint8_t *sub_info, uint64_t m,
                                                                      uint64_t n_items, uint16_t *rec, uint32_t *cnt_e,
                                                                      uint32_t *cnt_l, uint32_t *cnt_t) {
    __shared__ uint32_t s_e[kDecideThreads / 64], s_l[kDecideThreads / 64], s_t[kDecideThreads / 64];
    // the tile's descriptors and a halo of one group on either side, staged once: the group walks below are chains of dependent
    // byte loads (a walk that leaves the window, which no real group does, falls back to global memory)
    __shared__ uint8_t s_info[kDecideTile + 2 * kDecideHalo];
    const uint64_t t0 = (uint64_t)blockIdx.x * kDecideTile;
    const uint64_t w_lo = t0 >= (uint64_t)kDecideHalo ? t0 - kDecideHalo : 0;
    const uint64_t w_hi = t0 + kDecideTile + kDecideHalo < m ? t0 + kDecideTile + kDecideHalo : m;
    for (uint64_t x = w_lo + threadIdx.x; x < w_hi; x += kDecideThreads) s_info[x - w_lo] = sub_info[x];
    __syncthreads();
    auto info_at = [&](uint64_t x) -> int { return (x >= w_lo && x < w_hi) ? (int)s_info[x - w_lo] : (int)sub_info[x]; };
    uint32_t ne = 0, nl = 0, nt = 0;
    for (int q = 0; q < kDecidePerThread; ++q) {
        uint64_t s = t0 + (uint64_t)q * kDecideThreads + threadIdx.x;      // consecutive lanes, consecutive runs
        if (s >= m) break;
        int inf = info_at(s);
        int a = inf & 7, b = (inf >> 3) & 7;
        // group extent [gs, ge): at most 24 runs share a (k-1)-mer; the characters its solid runs carry are collected on the way (the
        // kernel is bound by vector issue: one walk over the group here instead of two, and the walk back also answers outputed_b: 16.3 ->
        // 11.35 ms at 100 M reads; folding the walk over the runs behind in as well costs more than it saves: 15.1 ms)
        int has_a = 0, has_b = 0;
        auto collect = [&](int xi) {
            const int xa = xi & 7, xb = (xi >> 3) & 7;
            if (xa != kDollar && xb != kDollar) { has_a |= 1 << xa; has_b |= 1 << xb; }
        };
        collect(inf);
        // (outputed_b, s2.cpp:822-824, from the same walk back: a run in front with the same b is not suppressed if its a != $, or if its
        // a == $ and no solid run of the group carries b)
        bool front_b_solid = false, front_b_dollar = false;
        uint64_t gs = s;
        for (int gi = inf; !(gi & 64);) {
            --gs; gi = info_at(gs); collect(gi);
            if (((gi >> 3) & 7) == b) { if ((gi & 7) != kDollar) front_b_solid = true; else front_b_dollar = true; }
        }
        uint64_t ge = s + 1;
        while (ge < m) {
            const int xi = info_at(ge);
            if (xi & 64) break;
            collect(xi);
            ++ge;
        }
        uint16_t r = 0xFFFF;
        if (!run_suppressed(a, b, has_a, has_b)) {
            const bool seen_b = front_b_solid || (front_b_dollar && !((has_b >> b) & 1));
            int w = (b == kDollar) ? 0 : (seen_b ? b + 5 : b + 1);
            int last = 0;
            if (a != kDollar) {                                    // last_a[], s2.cpp:776-779,823
                bool later = false;
                for (uint64_t x = s + 1; x < ge; ++x) {
                    int xi = info_at(x), xa = xi & 7, xb = (xi >> 3) & 7;
                    if (xa == a && (xb != kDollar || !((has_a >> a) & 1))) later = true;
                }
                last = later ? 0 : 1;
            }
            uint64_t run = run_length(sub_start, s, m, n_items);
            uint32_t count = run > 65535 ? 65535u : (uint32_t)run;  // kMaxMulti_t
            int tip = a == kDollar;
            r = (uint16_t)(w | (last << 4) | (tip << 5) | ((count > 255 ? 255u : count) << 8));
            ne++;
            nl += count > 254;                                      // kMaxMulti2_t, sdbg_multi_io.h:99
            nt += tip;
        }
        rec[s] = r;
    }
    ne = wave_sum(ne); nl = wave_sum(nl); nt = wave_sum(nt);
    if (lane_id() == 0) { s_e[wave_id()] = ne; s_l[wave_id()] = nl; s_t[wave_id()] = nt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t e = 0, l = 0, t = 0;
        for (int w = 0; w < kDecideThreads / 64; ++w) { e += s_e[w]; l += s_l[w]; t += s_t[w]; }
        cnt_e[blockIdx.x] = e; cnt_l[blockIdx.x] = l; cnt_t[blockIdx.x] = t;
    }
}

// E5: order-preserving compaction into the output stream + per-bucket boundaries
template <int W>
__global__ __launch_bounds__(kDecideThreads) void emit_write_kernel(const Key<W> *keys, RunStarts sub_start, const uint8_t *sub_info, const uint16_t *rec,
                                                                     uint64_t m, uint64_t n_items, const uint64_t *base_e,
                                                                     const uint64_t *base_l, const uint64_t *base_t, int words_per_tip,
                                                                     uint32_t b_lo, uint16_t *out_rec, uint16_t *out_large,
                                                                     uint32_t *out_tips, int64_t *bucket_first /* [nb][3] */) {
    __shared__ uint64_t s_scr[kDecideThreads / 64 + 1];
    uint64_t s0 = (uint64_t)blockIdx.x * kDecideTile + (uint64_t)threadIdx.x * kDecidePerThread;
    uint16_t r[kDecidePerThread];
    uint64_t packed = 0;   // emitted | large << 20 | tips << 40
    uint32_t cnts[kDecidePerThread];
    for (int q = 0; q < kDecidePerThread; ++q) {
        uint64_t s = s0 + q;
        r[q] = 0xFFFF; cnts[q] = 0;
        if (s < m) {
            r[q] = rec[s];
            if (r[q] != 0xFFFF) {
                cnts[q] = r[q] >> 8;                               // (the run starts are read for the runs above 254 only)
                if (cnts[q] == 255) {
                    uint64_t run = run_length(sub_start, s, m, n_items);
                    cnts[q] = run > 65535 ? 65535u : (uint32_t)run;
                }
                packed += 1ull + ((uint64_t)(cnts[q] > 254) << 20) + ((uint64_t)((r[q] >> 5) & 1) << 40);
            }
        }
    }
    uint64_t ex = block_excl_scan64<kDecideThreads>(packed, s_scr, nullptr);
    uint64_t ie = base_e[blockIdx.x] + (ex & 0xFFFFF), il = base_l[blockIdx.x] + ((ex >> 20) & 0xFFFFF),
             it = base_t[blockIdx.x] + (ex >> 40);
    for (int q = 0; q < kDecidePerThread; ++q) {
        uint64_t s = s0 + q;
        if (s >= m) break;
        const bool is_tip = r[q] != 0xFFFF && ((r[q] >> 5) & 1);
        const bool bucket_head = (sub_info[s] & 128) != 0;
        const uint64_t first_item = (is_tip || bucket_head) ? run_full_start(sub_start, s) : 0;   // only these two look at the key
        if (bucket_head) {                                         // number of records/large/tips before this bucket
            uint32_t bucket = keys[first_item].w[0] >> 16;
            int64_t *bf = bucket_first + (uint64_t)(bucket - b_lo) * 3;
            bf[0] = (int64_t)ie; bf[1] = (int64_t)il; bf[2] = (int64_t)it;
        }
        if (r[q] != 0xFFFF) {
            out_rec[ie++] = r[q];
            if (cnts[q] > 254) out_large[il++] = (uint16_t)cnts[q];
            if ((r[q] >> 5) & 1) {
                for (int j = 0; j < words_per_tip; ++j) out_tips[it * words_per_tip + j] = keys[first_item].w[j];   // s2.cpp:826-830
                it++;
            }
        }
    }
}

// E3-E5 in one kernel (MGTA_EMIT_CHAIN): emit_decide_kernel's decision and emit_write_kernel's compaction behind two chained scans
// across the workgroups, so that no record of a run, no per-tile count and no base ever goes through device memory.  A workgroup
// takes kChainRounds rounds of kDecideTile runs (lane <-> run as in emit_decide_kernel) and issues the loads of the descriptors
// -- the info bytes of the tile and a halo, 16 at a time, and both run starts of every run, half the rounds at a time -- before it
// uses one.  The decision (one byte: w | last << 4 | tip << 5, 0xFF suppressed) and the capped count of every run stay in
// registers; the counts per (round, q, wave) are scanned in LDS, wave 0 publishes the tile's emitted records to one chain and wave 1
// its large << kChainTipBits | tips to the other, every wave collects its records in LDS in stream order, and only then do the two
// waves look back.  The records leave as one run of 16-byte stores.  Runs above 254, tips and bucket heads are rare; they leave
// lane by lane.  sub_info is 16-byte aligned and readable up to the next multiple of 16 behind m.
constexpr int kChainRounds = 8;
constexpr int kChainTile = kDecideTile * kChainRounds;     // 8192 runs per workgroup
constexpr int kChainSlots = kChainRounds * kDecidePerThread * (kDecideThreads / 64);
constexpr int kChainTipBits = 34;                          // host: tips <= m < 2^34, large <= n_items / 255 < 2^(62 - 34)
static_assert(kChainTipBits < 62 && kChainTile < (1 << 20), "the second chain's value, the packed tile counts");
struct DecideChain {
    unsigned long long *state_e, *state_lt;   // [n_tiles] each, zeroed
    uint32_t *ticket, *error;                  // zeroed
    uint64_t *totals;                          // [3] emitted, large, tips: written by the last tile
};

template <int W, bool TICKET>
__global__ __launch_bounds__(kDecideThreads, 6) void emit_decide_write_kernel(const Key<W> *keys, RunStarts sub_start, const uint8_t *sub_info, uint64_t m,
                                                                            uint64_t n_items, DecideChain chain, uint32_t n_tiles, int words_per_tip,
                                                                            uint32_t b_lo, uint16_t *out_rec, uint16_t *out_large, uint32_t *out_tips,
                                                                            int64_t *bucket_first /* [nb][3] */) {
    constexpr int NW = kDecideThreads / 64, NQ = kDecidePerThread;
    constexpr int kChunks = (kChainTile + 2 * kDecideHalo) / 16, kChunkIters = (kChunks + kDecideThreads - 1) / kDecideThreads;
    static_assert(NQ == 4 && kDecideHalo % 16 == 0 && kChainSlots <= kDecideThreads, "four decisions per word; 16-byte loads; one scan");
    __shared__ uint4 s_info4[kChunks];
    __shared__ uint16_t s_out[kChainTile];
    __shared__ uint64_t s_cnt[kChainSlots];                // emitted | large << 20 | tips << 40 per (round, q, wave), then their prefix
    __shared__ uint64_t s_scr[NW + 1];
    __shared__ uint32_t s_tile;
    __shared__ unsigned long long s_base[2];
    const uint8_t *s_info = reinterpret_cast<const uint8_t *>(s_info4);    // s_info[x - t0 + kDecideHalo]
    const uint32_t tile = TICKET ? chain_ticket(chain.ticket, &s_tile) : blockIdx.x;
    const uint64_t t0 = (uint64_t)tile * kChainTile;
    const uint32_t tid = threadIdx.x;
    const int lane = lane_id(), wv = wave_id();
    // positions inside the tile are 32-bit offsets from t0 (a walk stays within a group's 24 runs): j < m_l <=> t0 + j < m
    const uint8_t *info_t = sub_info + t0;
    const uint32_t *lo_t = sub_start.lo + t0;
    const int m_l = (int)(m - t0 < (1ull << 30) ? m - t0 : (1ull << 30));
    const uint32_t n_t = (uint32_t)(m_l < kChainTile + 1 ? m_l : kChainTile + 1);      // the runs of the tile, and the one behind it
    const int w_lo = tile ? -kDecideHalo : 0, w_hi = m_l < kChainTile + kDecideHalo ? m_l : kChainTile + kDecideHalo;   // what LDS holds

    // ---- every load first
    uint4 iv[kChunkIters];
#pragma unroll
    for (int j = 0; j < kChunkIters; ++j) {
        const uint32_t c = (uint32_t)j * kDecideThreads + tid;
        const int at = 16 * (int)c - kDecideHalo;
        iv[j] = make_uint4(0, 0, 0, 0);
        if (c < (uint32_t)kChunks && at >= w_lo && at < m_l) iv[j] = *reinterpret_cast<const uint4 *>(info_t + at);
    }
    // the count of every run, capped at 65535 (kMaxMulti_t), two per word: both starts of the runs of half the rounds are in flight at
    // a time (all of them at once need more registers than six waves per SIMD leave)
    uint32_t cnt2[kChainRounds][NQ / 2];
    const bool owns_last = n_t <= (uint32_t)kChainTile && ((n_t - 1) & (kDecideThreads - 1)) == tid;   // the last run of all ends with the keys
    uint32_t last_len = 0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        uint32_t lo0[kChainRounds / 2][NQ], lo1[kChainRounds / 2][NQ];
#pragma unroll
        for (int r = 0; r < kChainRounds / 2; ++r)
#pragma unroll
            for (int q = 0; q < NQ; ++q) {                 // (clamped, not skipped: no branch between the loads)
                const uint32_t idx = (uint32_t)(((half * (kChainRounds / 2) + r) * NQ + q) * kDecideThreads) + tid;
                lo0[r][q] = lo_t[idx < n_t - 1 ? idx : n_t - 1];
                lo1[r][q] = lo_t[idx + 1 < n_t - 1 ? idx + 1 : n_t - 1];
            }
        if (half == 0) {
#pragma unroll
            for (int j = 0; j < kChunkIters; ++j) {
                const uint32_t c = (uint32_t)j * kDecideThreads + tid;
                if (c < (uint32_t)kChunks) s_info4[c] = iv[j];
            }
            if (owns_last) {
                const uint64_t rest = n_items - run_full_start(sub_start, t0 + n_t - 1);
                last_len = rest > 65535 ? 65535u : (uint32_t)rest;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < kChainRounds / 2; ++r) {
            const int rr = half * (kChainRounds / 2) + r;
            cnt2[rr][0] = cnt2[rr][1] = 0;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                uint32_t len = lo1[r][q] - lo0[r][q];
                if (owns_last && (uint32_t)(rr * NQ + q) == (n_t - 1) / kDecideThreads) len = last_len;
                cnt2[rr][q >> 1] |= (len > 65535u ? 65535u : len) << (16 * (q & 1));
            }
            // (the compiler must not see through the packing, or it keeps all the counts in a register each)
            asm volatile("" : "+v"(cnt2[rr][0]), "+v"(cnt2[rr][1]));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();

    // ---- the decision of every run: emit_decide_kernel's, on the LDS copy of the descriptors
    auto info_at = [&](int j) -> int { return (j >= w_lo && j < w_hi) ? (int)s_info[j + kDecideHalo] : (int)info_t[j]; };
    uint32_t dec[kChainRounds];
#pragma unroll
    for (int r = 0; r < kChainRounds; ++r) dec[r] = ~0u;
#pragma unroll 1
    for (int r = 0; r < kChainRounds; ++r) {               // (one copy of the walks; the round's registers are picked by compares)
        uint32_t c01 = 0, c23 = 0, dr = 0;
#pragma unroll
        for (int rr = 0; rr < kChainRounds; ++rr)
            if (rr == r) { c01 = cnt2[rr][0]; c23 = cnt2[rr][1]; }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int s = (r * NQ + q) * kDecideThreads + (int)tid;
            const uint32_t count = ((q & 2 ? c23 : c01) >> (16 * (q & 1))) & 0xFFFFu;
            uint32_t d = 0xFFu;
            if (s < m_l) {
                const int inf = info_at(s);
                const int a = inf & 7, b = (inf >> 3) & 7;
                // group extent [gs, ge): the characters its solid runs carry are collected on the way, and the walk back also answers
                // outputed_b (s2.cpp:822-824): a run in front with the same b is not suppressed if its a != $, or if its a == $ and no
                // solid run of the group carries b
                int has_a = 0, has_b = 0;
                auto collect = [&](int xi) {
                    const int xa = xi & 7, xb = (xi >> 3) & 7;
                    if (xa != kDollar && xb != kDollar) { has_a |= 1 << xa; has_b |= 1 << xb; }
                };
                collect(inf);
                bool front_b_solid = false, front_b_dollar = false;
                int gs = s;
                for (int gi = inf; !(gi & 64);) {
                    --gs; gi = info_at(gs); collect(gi);
                    if (((gi >> 3) & 7) == b) { if ((gi & 7) != kDollar) front_b_solid = true; else front_b_dollar = true; }
                }
                int ge = s + 1;
                while (ge < m_l) {
                    const int xi = info_at(ge);
                    if (xi & 64) break;
                    collect(xi);
                    ++ge;
                }
                if (!run_suppressed(a, b, has_a, has_b)) {
                    const bool seen_b = front_b_solid || (front_b_dollar && !((has_b >> b) & 1));
                    const int w = (b == kDollar) ? 0 : (seen_b ? b + 5 : b + 1);
                    int last = 0;
                    if (a != kDollar) {                    // last_a[], s2.cpp:776-779,823
                        bool later = false;
                        for (int x = s + 1; x < ge; ++x) {
                            const int xi = info_at(x), xa = xi & 7, xb = (xi >> 3) & 7;
                            if (xa == a && (xb != kDollar || !((has_a >> a) & 1))) later = true;
                        }
                        last = later ? 0 : 1;
                    }
                    d = (uint32_t)(w | (last << 4) | ((a == kDollar) << 5));
                }
            }
            dr |= d << (8 * q);
            const bool em = d != 0xFFu;
            const uint64_t bal_e = __ballot(em), bal_l = __ballot(em && count > 254u), bal_t = __ballot(em && (d & 32u));   // > 254: kMaxMulti2_t
            if (lane == 0)
                s_cnt[(r * NQ + q) * NW + wv] = (uint64_t)__popcll(bal_e) | (uint64_t)__popcll(bal_l) << 20 | (uint64_t)__popcll(bal_t) << 40;
        }
#pragma unroll
        for (int rr = 0; rr < kChainRounds; ++rr)
            if (rr == r) dec[rr] = dr;
    }
    __syncthreads();

    // ---- the tile's three counts, their prefix inside the tile, and the aggregates out to the chains
    uint64_t tot = 0;
    const uint64_t ex = block_excl_scan64<kDecideThreads>(tid < (uint32_t)kChainSlots ? s_cnt[tid] : 0ull, s_scr, &tot);
    if (tid < (uint32_t)kChainSlots) s_cnt[tid] = ex;
    const uint32_t te = (uint32_t)tot & 0xFFFFFu, tl = (uint32_t)(tot >> 20) & 0xFFFFFu, tt = (uint32_t)(tot >> 40);
    const uint64_t agg_lt = (uint64_t)tl << kChainTipBits | tt;
    if (wv == 0) chain_publish(chain.state_e, tile, te);
    if (wv == 1) chain_publish(chain.state_lt, tile, agg_lt);
    __syncthreads();

    // ---- the records in stream order, in LDS (order of the runs: round, q, wave, lane)
#pragma unroll
    for (int r = 0; r < kChainRounds; ++r)
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const uint32_t d = (dec[r] >> (8 * q)) & 0xFFu, count = (cnt2[r][q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
            const bool em = d != 0xFFu;
            const uint64_t bal_e = __ballot(em);
            if (em) {
                const uint32_t at = ((uint32_t)s_cnt[(r * NQ + q) * NW + wv] & 0xFFFFFu) + (uint32_t)__popcll(bal_e & lanemask_lt());
                s_out[at] = (uint16_t)(d | (count > 255u ? 255u : count) << 8);
            }
        }
    if (wv == 0) {
        const uint64_t before = chain_look_back(chain.state_e, tile, te, chain.error);
        if (lane == 0) {
            s_base[0] = before;
            if (tile + 1 == n_tiles) chain.totals[0] = before + te;
        }
    }
    if (wv == 1) {
        const uint64_t before = chain_look_back(chain.state_lt, tile, agg_lt, chain.error);
        if (lane == 0) {
            s_base[1] = before;
            if (tile + 1 == n_tiles) { chain.totals[1] = (before >> kChainTipBits) + tl; chain.totals[2] = (before & ((1ull << kChainTipBits) - 1ull)) + tt; }
        }
    }
    __syncthreads();
    const uint64_t be = s_base[0], bl = s_base[1] >> kChainTipBits, bt = s_base[1] & ((1ull << kChainTipBits) - 1ull);

    // ---- the records out: single ones up to the first 16-byte boundary of the stream, eight per store, single ones again
    {
        uint32_t head = (uint32_t)((8u - (uint32_t)(be & 7u)) & 7u);
        if (head > te) head = te;
        const uint32_t n8 = (te - head) >> 3, tail0 = head + (n8 << 3);
        if (tid < head) out_rec[be + tid] = s_out[tid];
        for (uint32_t c = tid; c < n8; c += kDecideThreads) {
            const uint32_t i = head + (c << 3);
            uint4 v;
            v.x = (uint32_t)s_out[i] | (uint32_t)s_out[i + 1] << 16; v.y = (uint32_t)s_out[i + 2] | (uint32_t)s_out[i + 3] << 16;
            v.z = (uint32_t)s_out[i + 4] | (uint32_t)s_out[i + 5] << 16; v.w = (uint32_t)s_out[i + 6] | (uint32_t)s_out[i + 7] << 16;
            *reinterpret_cast<uint4 *>(out_rec + be + i) = v;
        }
        if (tail0 + tid < te) out_rec[be + tail0 + tid] = s_out[tail0 + tid];
    }

    // ---- the runs above 254, the tips and the bucket heads: the only ones with a second output, the last two the only ones that
    // look at a key
#pragma unroll
    for (int r = 0; r < kChainRounds; ++r)
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int k0 = (r * NQ + q) * kDecideThreads;                               // the run is t0 + k0 + tid
            const uint32_t d = (dec[r] >> (8 * q)) & 0xFFu, count = (cnt2[r][q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
            const bool em = d != 0xFFu, large = em && count > 254u, tip = em && (d & 32u);
            const bool bucket_head = (int)tid < m_l - k0 && (s_info[kDecideHalo + k0 + tid] & 128) != 0;
            if (__ballot(large || tip || bucket_head) == 0) continue;                  // (wave-uniform)
            const uint64_t bal_e = __ballot(em), bal_l = __ballot(large), bal_t = __ballot(tip), lt = lanemask_lt();
            const uint64_t x = s_cnt[(r * NQ + q) * NW + wv];
            const uint64_t ie = be + ((uint32_t)x & 0xFFFFFu) + (uint32_t)__popcll(bal_e & lt);
            const uint64_t il = bl + ((uint32_t)(x >> 20) & 0xFFFFFu) + (uint32_t)__popcll(bal_l & lt);
            const uint64_t it = bt + (uint32_t)(x >> 40) + (uint32_t)__popcll(bal_t & lt);
            if (large) out_large[il] = (uint16_t)count;
            if (tip || bucket_head) {
                const uint64_t first_item = run_full_start(sub_start, t0 + k0 + tid);
                if (bucket_head) {                                                     // number of records/large/tips before this bucket
                    const uint32_t bucket = keys[first_item].w[0] >> 16;
                    int64_t *bf = bucket_first + (uint64_t)(bucket - b_lo) * 3;
                    bf[0] = (int64_t)ie; bf[1] = (int64_t)il; bf[2] = (int64_t)it;
                }
                if (tip)
                    for (int j = 0; j < words_per_tip; ++j) out_tips[it * words_per_tip + j] = keys[first_item].w[j];   // s2.cpp:826-830
            }
        }
}

// MGTA_EMIT_CHAIN=2: an output of emit_decide_write_kernel against that of the three-step route
template <class T>
__global__ __launch_bounds__(256) void emit_equal_kernel(const T *a, const T *b, uint64_t n, uint32_t *bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        if (a[i] != b[i]) atomicAdd(bad, 1u);
}

}  // namespace mgta
#include "sdbg_solid.hpp"
namespace mgta {

// ---------------------------------------------------------------------------------------------
// host orchestration
// ---------------------------------------------------------------------------------------------
// digits of the bits below 32W - T (T = prefix bits the global passes sorted on), least significant first (flags, then characters; the zero pad is skipped)
static std::vector<Digit> low_digit_plan(int k, int W, int T) {
    std::vector<Digit> plan;
    int pad = 32 * W - 2 * k - 4, top = 32 * W - T;
    if (top > 0) plan.push_back(Digit{0, std::min(4, top)});
    for (int pos = 4 + pad; pos < top; pos += 8) plan.push_back(Digit{pos, std::min(8, top - pos)});
    return plan;
}

// hipMalloc/hipFree of multi-GB buffers costs far more than the kernels that use them: the pool slots (enum Slot) only grow
template <class T>
static T *pool_get(mgta_ctx *ctx, int slot, uint64_t bytes) {
    if ((int)ctx->pool.size() < S_NUM) ctx->pool.resize(S_NUM);
    DevBuf &b = ctx->pool[slot];
    if (b.bytes < bytes || !b.p) {
        b.release();
        // an eighth of headroom (the pass planner leaves that much): the builds of a multi-k run need a few per cent more from one k to
        // the next (contigs join the reads), and obtaining the buffers again costs more than a build (20 M reads: 1.7 s for 9 % more)
        b.alloc(bytes + bytes / 8, &ctx->live_bytes, &ctx->peak_bytes);
    }
    return b.as<T>();
}
static uint64_t pool_bytes(const mgta_ctx *ctx) {
    uint64_t t = 0;
    for (const DevBuf &b : ctx->pool) t += b.bytes;
    return t;
}

// MGTA_SORT_BIAS: 0 never, 1 (default) when it saves a pass and leaves short segments, 2 whenever valid (tests) -- see choose_top_plan.
// MGTA_SORT_SIDE: side digits (see SortJob::uses_side) 0 off, 1 (default) on, 2 on and every side census checked against the census
// of the keys (tests).  Read once per build and never cached: tests and scripts flip them between builds.
// MGTA_SORT_FUSED: the key writer of a range pass does the first global sort pass (see Build::count_pass) 0 never, 1 (default) where
// the plan of the pass was known when its items were counted, 2 the same and the writer's output checked on the device (tests).
// MGTA_SORT_WIDE: global passes on digits of more than 8 bits (see widen_top_plan) 0 never, 1 (default) where they save a global pass
// and leave short segments, 2 every pass but the first to run, whatever it saves (tests: small inputs take the wide kernels).
// MGTA_EMIT_FUSED: the segment-local finish leaves the emitter's info byte of every key position behind, and the emitter compacts
// those bytes instead of reading the keys again (see lds_finish) 0 never, 1 (default) wherever the sorted prefix lies inside the
// (k-1)-mer, 2 the same and the run descriptors checked on the device against those of emit_compact_kernel (tests).
// MGTA_EMIT_CHAIN: the runs are decided and their records written by one kernel behind two chained scans (emit_decide_write_kernel)
// 0 never: emit_decide_kernel, three scans, a host round trip and emit_write_kernel, 1 (default) always, 2 both and every output
// of the one kernel checked on the device against the three steps' (tests).
struct SortModes {
    int bias = 1, side = 1, fused = 1, wide = 1, emit_fused = 1, emit_chain = 1;
    static SortModes from_env() {
        const char *bias = getenv("MGTA_SORT_BIAS"), *side = getenv("MGTA_SORT_SIDE"), *fused = getenv("MGTA_SORT_FUSED"), *wide = getenv("MGTA_SORT_WIDE");
        const char *emit_fused = getenv("MGTA_EMIT_FUSED"), *emit_chain = getenv("MGTA_EMIT_CHAIN");
        return SortModes{bias ? atoi(bias) : 1, side ? atoi(side) : 1, fused ? atoi(fused) : 1, wide ? atoi(wide) : 1, emit_fused ? atoi(emit_fused) : 1,
                         emit_chain ? atoi(emit_chain) : 1};
    }
};

// The global passes sort on P leading bytes of the keys: the smallest P that leaves segments of <= 256 keys on average -- up to 1024
// rather than a fourth global pass: a 4096-key tile still holds several such segments, and the comparison route needs key bits left in
// word 0.  prefix_frac: share of the leading-byte values the keys can take (a pass over a bucket sub-range only holds that share of
// the prefixes, so its segments are as long as those of the whole key set)
static double avg_segment_len(uint64_t n_items, int p, double prefix_frac) { return (double)n_items / std::max(1.0, std::pow(256.0, p) * prefix_frac); }
// the same for passes that sorted on `bits` key bits in all
static double avg_segment_len_bits(uint64_t n_items, int bits, double prefix_frac) { return (double)n_items / std::max(1.0, std::pow(2.0, bits) * prefix_frac); }
// The global passes of a build over the buckets [b_lo, b_hi) need not spend digit values on prefixes no key has: word 0 minus
// (b_lo << 16) has `skip` leading zero bits, and P digits of 8 bits taken right below them order the keys by their leading
// T = 8P + skip bits (a third of the buckets: skip = 1, so three passes leave the 645-key segments that otherwise take four).
// T >= 16 is required: then the bias is a multiple of 2^(32 - T) and equal biased prefixes are equal key prefixes.
// A pass may sort on more than 8 bits (width[]): the pass that runs first keeps 8 (its census comes from the key writers), later
// ones take 9 where the scatter of the key width has the LDS for 512 digit values and 16-bit side entries (kWideFits).
constexpr int kMaxTop = 4;
struct TopPlan {
    int P = 0, skip = 0;
    uint32_t bias = 0;
    double frac = 1.0;           // share of the 2^T prefix values the keys can take
    int width[kMaxTop] = {8, 8, 8, 8};   // bits of global pass i, most significant first (pass P - 1 runs first)
    int key_bits() const { int t = 0; for (int i = 0; i < P; ++i) t += width[i]; return t; }
    int T() const { return key_bits() + skip; }
    int n_wide() const { int c = 0; for (int i = 0; i < P; ++i) c += width[i] > 8; return c; }
    int max_width() const { int m = 8; for (int i = 0; i < P; ++i) m = std::max(m, width[i]); return m; }
    bool same_digits(const TopPlan &o) const {
        bool same = P == o.P && skip == o.skip && bias == o.bias;
        for (int i = 0; same && i < P; ++i) same = width[i] == o.width[i];
        return same;
    }
    // digit of global pass i, most significant first (i = 0: the key bits right below the `skip` bits every key shares, after the bias)
    Digit pass_digit(int W, int i) const {
        int below = skip;
        for (int j = 0; j <= i; ++j) below += width[j];
        return Digit{32 * W - below, width[i], bias};
    }
    double avg_segment(uint64_t n_items) const { return avg_segment_len_bits(n_items, key_bits(), frac); }
};
// mode: SortModes::bias
static TopPlan choose_top_plan(const mgta_ctx *ctx, uint64_t n_items, int max_top, double prefix_frac, uint32_t b_lo = 0, uint32_t b_hi = 0,
                               int mode = 0) {
    TopPlan plain;
    plain.frac = prefix_frac;
    if (ctx && ctx->force_full_lsd) return plain;
    while (plain.P < max_top && avg_segment_len(n_items, plain.P, prefix_frac) > (plain.P >= 3 ? 700.0 : 256.0)) ++plain.P;
    if (mode == 0 || b_hi <= b_lo || (b_lo == 0 && b_hi >= (uint32_t)MGTA_NUM_BUCKETS)) return plain;
    const uint32_t span = ((b_hi - b_lo) << 16) - 1u;                  // largest biased word 0
    const int skip_full = __builtin_clz(span | 1u);
    for (int P = 1; P <= max_top; ++P) {
        const int skip = std::min(skip_full, 32 - 8 * P);
        if (skip <= 0 || 8 * P + skip < 16) continue;
        const double frac = std::min(1.0, prefix_frac * std::pow(2.0, skip));
        // measured at 100 M reads (7.2 G keys per pass, a third of the buckets): three biased passes leave 645-key segments and the LDS
        // finish then costs 170 ms instead of 100 ms — exactly what the fourth scatter + census (45 + 17 ms) would have cost.  The pass is
        // only worth skipping when the segments stay short (<= 400 keys).
        const double limit = mode >= 2 ? (P >= 3 ? 700.0 : 256.0) : (P >= 3 ? 400.0 : 256.0);
        if (P < max_top && avg_segment_len(n_items, P, frac) > limit) continue;
        if (P < plain.P || (mode >= 2 && P <= plain.P)) return TopPlan{P, skip, b_lo << 16, frac};
        break;
    }
    return plain;
}

// Wide digits (wide: SortModes::wide, for key widths with kWideFits only).  `base` is choose_top_plan's choice.  1: one pass fewer
// with 8 bits in the pass that runs first and 9 in every later one, below the most leading bits the range's keys share that still
// fit 32 (bias_mode != 0), where that leaves segments of <= 256 keys on average -- at 100 M reads (7.2 G keys per range, a third of
// the buckets) 8 + 9 + 9 bits below 1 skipped bit, T = 27, 161-key segments, in place of four 8-bit passes.  2: the passes of `base`,
// as many of the later ones 9 bits wide as fit 32 bits (the leading ones first), the skipped bits cut to what is left.
static TopPlan widen_top_plan(const TopPlan &base, uint64_t n_items, int max_top, double prefix_frac, uint32_t b_lo, uint32_t b_hi, int bias_mode,
                              int wide) {
    const int max_bits = 8 * std::min(max_top, kMaxTop);
    if (wide <= 0 || base.P < 2) return base;
    if (wide >= 2) {
        TopPlan tp = base;
        for (int i = 0; i < tp.P - 1 && tp.key_bits() < max_bits; ++i) tp.width[i] = 9;
        if (tp.key_bits() + tp.skip > max_bits) {
            tp.skip = max_bits - tp.key_bits();
            if (tp.skip < 0 || (tp.skip > 0 && tp.T() < 16)) return base;
            if (tp.skip == 0) tp.bias = 0;
            tp.frac = std::min(1.0, prefix_frac * std::pow(2.0, tp.skip));
        }
        return tp;
    }
    if (base.P < 3) return base;               // (one pass fewer must still hold a wide pass behind the first)
    TopPlan tp;
    tp.P = base.P - 1;
    for (int i = 0; i < tp.P - 1; ++i) tp.width[i] = 9;
    const bool sub_range = bias_mode != 0 && b_hi > b_lo && !(b_lo == 0 && b_hi >= (uint32_t)MGTA_NUM_BUCKETS);
    const int skip_full = sub_range ? __builtin_clz((((b_hi - b_lo) << 16) - 1u) | 1u) : 0;
    tp.skip = std::max(0, std::min(skip_full, max_bits - tp.key_bits()));
    if (tp.skip > 0 && tp.T() < 16) tp.skip = 0;
    tp.bias = tp.skip > 0 ? b_lo << 16 : 0u;
    tp.frac = std::min(1.0, prefix_frac * std::pow(2.0, tp.skip));
    if (tp.key_bits() > max_bits || tp.avg_segment(n_items) > 256.0) return base;
    return tp;
}

// One sort: n keys of WT words in `a` (`b` is the other buffer of the ping-pong) ascending on the digits that matter: top.P global LSD
// passes on the leading bytes, then every segment of equal prefix finished inside LDS on the `low` digits.  The key writer of a build
// pass reads the same object (fused census, side digits), so the writer and the sort cannot disagree on the plan.
template <int WT>
struct SortJob {
    Key<WT> *a = nullptr, *b = nullptr;
    uint64_t n = 0;
    TopPlan top;
    std::vector<Digit> low;                   // the significant digits below the leading top.T() bits, least significant first
    uint32_t mask_last2 = ~0u, mask_last = ~0u;   // significant bits of the last two key words (LocalPlan)
    int side_mode = 1;                        // SortModes::side
    bool census_done = false;                 // the first global pass's census (tiles of kBlockTile keys of a) is already in S_HIST
    bool side_done = false;                   // S_SIDE already holds the digit of every key that the first global pass to run sorts on
    bool first_pass_done = false;             // the key writer placed the keys by the first global pass's digit: the passes start at the second
    int emit_k = 0;                           // > 0: the keys are those of a graph of this k, and the finish may leave the emitter's info bytes behind
    // side digits: the scatter of a pass leaves the NEXT pass's digit of every key in a byte array (S_SIDE), and that pass's census
    // reads the bytes instead of the keys
    bool uses_side() const { return side_mode > 0 && top.P >= 2 && kSideFits<WT>; }
    // bytes of S_SIDE (an entry is as wide as the digit it carries) and of the census table S_HIST (a row per digit value of the widest
    // pass): the key writer and the sort ask for the same, so that neither's request moves what the other left there
    uint64_t side_bytes() const { return n * (top.max_width() > 8 ? 2u : 1u) + 64; }
    uint64_t hist_bytes() const { return std::max<uint64_t>(1, (n + kBlockTile - 1) / kBlockTile) * ((uint64_t)8 << top.max_width()); }
};
// keys per digit value of the pass about to run (radix_rowscan_kernel -> radix_scatter_kernel, the fused key writer)
static uint64_t *digit_totals(mgta_ctx *ctx) { return pool_get<uint64_t>(ctx, S_DIGIT_TOTALS, 1024 * 8); }
struct SortLog {                              // what the stats of a build take from its sorts
    mgta_build_stats *S = nullptr;
    std::vector<Timer> scatter;               // one per global scatter, read when the build is done (ms_sort_scatter)
};

// census, row scan and scatter of ONE global pass on a digit of BITS bits (NEXT_BITS: width of the next pass's digit, whose side
// entries this scatter writes where write_side); false on an error (set)
template <int WT, int BITS, int NEXT_BITS>
static bool global_pass(mgta_ctx *ctx, const SortJob<WT> &job, SortLog *log, const Key<WT> *src, Key<WT> *dst, Digit dg, Digit dn, bool first,
                        bool side_valid, bool write_side, void *d_side, uint64_t *d_hist, uint64_t *d_totals) {
    hipStream_t stream = ctx->stream;
    const uint64_t n = job.n, tiles = (n + kBlockTile - 1) / kBlockTile;
    constexpr uint64_t kVals = 1ull << BITS;
    const dim3 grid((unsigned)tiles), block(kSortThreads);
    if (!(first && job.census_done)) {
        if (side_valid) {
            hipLaunchKernelGGL((radix_census_side_kernel<BITS>), grid, block, 0, stream, static_cast<const SideEntry<BITS> *>(d_side), n, tiles, d_hist);
            if (job.side_mode >= 2) {                               // (test aid) the same census from the keys must agree
                std::vector<uint64_t> h_side(tiles * kVals), h_keys(tiles * kVals);
                MGTA_HIP_CHECK(hipStreamSynchronize(stream));
                MGTA_HIP_CHECK(hipMemcpy(h_side.data(), d_hist, tiles * kVals * 8, hipMemcpyDeviceToHost));
                hipLaunchKernelGGL((radix_census_kernel<WT, BITS>), grid, block, 0, stream, src, n, dg, tiles, d_hist);
                MGTA_HIP_CHECK(hipStreamSynchronize(stream));
                MGTA_HIP_CHECK(hipMemcpy(h_keys.data(), d_hist, tiles * kVals * 8, hipMemcpyDeviceToHost));
                if (h_side != h_keys) { set_error("internal: side-digit census differs from the census of the keys"); return false; }
            }
        } else
            hipLaunchKernelGGL((radix_census_kernel<WT, BITS>), grid, block, 0, stream, src, n, dg, tiles, d_hist);
    }
    hipLaunchKernelGGL(radix_rowscan_kernel, dim3((unsigned)kVals), dim3(1024), 0, stream, d_hist, tiles, d_totals);   // a row per digit value
    if (log) log->scatter.emplace_back(stream).start();
    // (the first pass of the sort orders nothing that was ordered before: its ranks need not be stable)
    auto launch = [&](auto biased, auto side, auto stable) {
        constexpr bool kSide = decltype(side)::value;
        hipLaunchKernelGGL((radix_scatter_kernel<WT, decltype(biased)::value, kSide, decltype(stable)::value, BITS, kSide ? NEXT_BITS : 8>), grid, block, 0, stream,
                           src, dst, n, dg, tiles, d_hist, d_totals, kSide ? static_cast<SideEntry<kSide ? NEXT_BITS : 8> *>(d_side) : nullptr, dn);
    };
    auto pick_stable = [&](auto biased, auto side) {
        if constexpr (BITS == 8) {
            if (first) { launch(biased, side, std::false_type{}); return; }
        }
        launch(biased, side, std::true_type{});                 // (a wide pass never runs first)
    };
    auto pick_side = [&](auto biased) {
        if constexpr (kScatterFits<WT, BITS, NEXT_BITS>) {
            if (write_side) { pick_stable(biased, std::true_type{}); return; }
        }
        pick_stable(biased, std::false_type{});
    };
    dg.bias ? pick_side(std::true_type{}) : pick_side(std::false_type{});
    if (log) {
        log->scatter.back().end();
        log->S->n_sort_launches++;
        if (BITS > 8) log->S->n_wide_passes++;
    }
    return true;
}

// the top.P global passes, least significant digit first; returns the buffer that holds their result, nullptr on an error (set)
template <int WT>
static Key<WT> *global_passes(mgta_ctx *ctx, const SortJob<WT> &job, SortLog *log) {
    uint64_t *d_hist = pool_get<uint64_t>(ctx, S_HIST, job.hist_bytes());
    uint64_t *d_totals = digit_totals(ctx);
    void *d_side = job.uses_side() ? pool_get<uint8_t>(ctx, S_SIDE, job.side_bytes()) : nullptr;
    bool side_valid = job.side_done && d_side;                          // d_side holds the digits of the pass about to run
    Key<WT> *src = job.a, *dst = job.b;
    for (int i = job.top.P - 1 - (job.first_pass_done ? 1 : 0); i >= 0; --i) {
        const bool first = i == job.top.P - 1;
        const Digit dg = job.top.pass_digit(WT, i), dn = i > 0 ? job.top.pass_digit(WT, i - 1) : Digit{0, 0, 0};
        const bool write_side = d_side && i > 0;
        // the kernels of the plan's widths: 8 (next 8 or 9), 9 (next 9, or none: a plan's last pass)
        const int bits = dg.bits, next = i > 0 ? dn.bits : 8;
        bool ok = false, known = true;
        auto run = [&](auto b, auto nb) {
            ok = global_pass<WT, decltype(b)::value, decltype(nb)::value>(ctx, job, log, src, dst, dg, dn, first, side_valid, write_side, d_side, d_hist, d_totals);
        };
        using std::integral_constant;
        if (bits == 8 && next == 8) run(integral_constant<int, 8>{}, integral_constant<int, 8>{});
        else if constexpr (kWideFits<WT>) {
            if (bits == 8 && next == 9) run(integral_constant<int, 8>{}, integral_constant<int, 9>{});
            else if (bits == 9 && (next == 9 || i == 0)) run(integral_constant<int, 9>{}, integral_constant<int, 9>{});
            else known = false;
        } else
            known = false;
        if (!known) { set_error("internal: no scatter kernel for a %d-bit digit before a %d-bit one at %d key words", bits, next, WT); return nullptr; }
        if (!ok) return nullptr;
        side_valid = write_side;
        std::swap(src, dst);
    }
    return src;
}

// keys of the longest segment an LDS kernel finishes at WT key words
template <int WT> constexpr uint32_t kLdsCap = BigCfg<WT>::kTile > 0 ? BigCfg<WT>::kTile : LocalCfg<WT>::kTile;
template <int WT>
static uint64_t split_list_bytes(uint64_t n_items) { return split_list_caps(n_items, LocalCfg<WT>::kTile, kLdsCap<WT>).bytes(); }

// The oversized route of lds_finish: the n_seg listed segments (seg_first, seg_end; all in src) that are longer than kLdsCap are split
// on the low digits from the top down, a launch per level; what a level leaves short enough is finished in LDS from the buffer it
// is in, into src.  The host reads a level's four counts back before it launches the next, so a level with nothing listed is never
// launched.  Returns the number of levels that split something, -1 on an error (set).
template <int WT>
static int split_oversized(mgta_ctx *ctx, const SortJob<WT> &job, Key<WT> *src, Key<WT> *dst, const uint64_t *seg_first, const uint64_t *seg_end,
                           uint32_t n_seg, const LocalPlan &lp) {
    hipStream_t stream = ctx->stream;
    const SplitCaps caps = split_list_caps(job.n, LocalCfg<WT>::kTile, kLdsCap<WT>);
    if (caps.n_small > 0xFFFFFFFFull) { set_error("too many keys for the lists of the oversized segments"); return -1; }
    uint64_t *d_lists = pool_get<uint64_t>(ctx, S_SPLIT, caps.bytes());
    uint64_t *at = d_lists;
    auto take = [&](uint64_t entries) { SegList l{at, at + entries, nullptr, (uint32_t)entries}; at += 2 * entries; return l; };
    SegList small = take(caps.n_small), mid = take(caps.n_mid), next[2] = {take(caps.n_next), take(caps.n_next)};
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(at);            // small, mid, next, segments split
    small.count = d_counts; mid.count = d_counts + 1; next[0].count = next[1].count = d_counts + 2;
    int levels = 0;
    const int n_low = (int)job.low.size();
    for (int level = 0; level < n_low && n_seg > 0; ++level) {
        MGTA_HIP_CHECK(hipMemsetAsync(d_counts, 0, 16, stream));
        const SplitLists out{small, mid, next[level & 1], d_counts + 3};
        hipLaunchKernelGGL((segment_split_kernel<WT>), dim3(n_seg), dim3(kSortThreads), 0, stream, src, dst, seg_first, seg_end, job.low[n_low - 1 - level],
                           (uint32_t)LocalCfg<WT>::kTile, kLdsCap<WT>, out);
        uint32_t h[4] = {0, 0, 0, 0};
        MGTA_HIP_CHECK(hipMemcpyAsync(h, d_counts, 16, hipMemcpyDeviceToHost, stream));
        MGTA_HIP_CHECK(hipStreamSynchronize(stream));
        if (h[0] > small.cap || h[1] > mid.cap || h[2] > out.next.cap) {
            set_error("internal: list overflow of the oversized segments at level %d (%u / %u / %u entries)", level, h[0], h[1], h[2]);
            return -1;
        }
        if (h[3] > 0) ++levels;
        if (h[0] > 0) hipLaunchKernelGGL((local_lsd_kernel<WT>), dim3(h[0]), dim3(kSortThreads), 0, stream, src, dst, small.first, small.end, 1, lp);
        if (h[1] > 0) hipLaunchKernelGGL((segment_lds_kernel<WT>), dim3(h[1]), dim3(kSortThreads), 0, stream, src, dst, mid.first, mid.end, lp);
        seg_first = out.next.first; seg_end = out.next.end; n_seg = h[2];
    }
    // behind the last digit: runs of keys equal on every compared bit stay as they are, in src
    if (n_seg > 0) hipLaunchKernelGGL((segment_copy_kernel<WT>), dim3(n_seg), dim3(kSortThreads), 0, stream, src, dst, seg_first, seg_end);
    return levels;
}

// every segment of equal leading top.T() bits finished inside LDS (local_sort_kernel, local_lsd_kernel), segments that did not fit a
// tile on their own (segment_lds_kernel, and the split levels of split_oversized for the longer ones).  `src` holds the keys, `dst`
// is scratch.  Returns src, nullptr on an error (set).
template <int WT>
static Key<WT> *lds_finish(mgta_ctx *ctx, const SortJob<WT> &job, Key<WT> *src, Key<WT> *dst, SortLog *log, const uint8_t **info_out = nullptr) {
    hipStream_t stream = ctx->stream;
    const uint64_t n_items = job.n;
    const int T = job.top.T();
    const std::vector<Digit> &low = job.low;
    if (low.size() > 64) { set_error("too many sort digits"); return nullptr; }
    Digit *d_plan = pool_get<Digit>(ctx, S_PLAN, 64 * sizeof(Digit));
    MGTA_HIP_CHECK(hipMemcpyAsync(d_plan, low.data(), low.size() * sizeof(Digit), hipMemcpyHostToDevice, stream));
    // room behind the stride for the last segment of a tile: ~2.5 average segments, an eighth of the tile at least, half at most
    const double avg_seg = job.top.avg_segment(n_items);
    uint32_t margin = (uint32_t)std::min<double>(LocalCfg<WT>::kTile / 2, std::max<double>(LocalCfg<WT>::kTile / 8, 2.5 * avg_seg));
    margin = (margin + 63u) & ~63u;
    const uint32_t stride = (uint32_t)LocalCfg<WT>::kTile - margin;
    const uint64_t l_blocks = (n_items + stride - 1) / stride;
    if (l_blocks > 0x7FFFFFFFull) { set_error("too many sort tiles"); return nullptr; }
    const uint32_t big_cap = (uint32_t)l_blocks + 1;                  // every workgroup defers one segment at most
    uint64_t *d_big = pool_get<uint64_t>(ctx, S_BIG, (2 * (uint64_t)big_cap + 2) * 8);
    uint32_t *d_big_count = reinterpret_cast<uint32_t *>(d_big + 2 * (uint64_t)big_cap);
    MGTA_HIP_CHECK(hipMemsetAsync(d_big_count, 0, 8, stream));
    uint64_t *d_lsd = pool_get<uint64_t>(ctx, S_LSD, 2 * l_blocks * 8);
    Timer t(stream);
    t.start();
    // the comparison route is skipped for a few sorts after one that found mostly long runs (highly redundant input)
    const bool skip_a = ctx->lsd_skip_left > 0;
    if (skip_a) --ctx->lsd_skip_left;
    const int ub = ((ctx->force_lsd_tiles & 1) || skip_a) ? 0 : std::max(0, std::min(8, (WT > 1 ? 40 : 32) - T));
    LocalPlan lp;
    lp.low_plan = d_plan; lp.n_low = (int)low.size(); lp.T = T;
    lp.upper = Digit{32 * WT - T - ub, ub};
    lp.mask_last2 = job.mask_last2; lp.mask_last = job.mask_last; lp.stride = stride;
    lp.lsd_list = d_lsd; lp.lsd_count = d_big_count + 1; lp.lsd_cap = (uint32_t)l_blocks;
    lp.debug = ctx->force_lsd_tiles >> 1;
    // The emitter's info byte of every key position, for jobs that ask (emit_k): the tiles local_sort_kernel finishes write theirs as
    // the keys leave LDS, emit_info_range_kernel those of every other range once its keys are final.  Its rule for a tile's first
    // key needs the sorted prefix inside the (k-1)-mer; masked keys (stage 1) emit nothing.  The bytes take the S_SIDE slot, idle since
    // the last global pass read its digits (same request as the sort's where it has a side array: the slot does not move).
    uint8_t *d_info = nullptr;
    if (info_out) *info_out = nullptr;
    if (info_out && job.emit_k > 0 && T <= 2 * (job.emit_k - 1) && (job.mask_last2 & job.mask_last) == ~0u && !lp.debug)
        d_info = pool_get<uint8_t>(ctx, S_SIDE, job.uses_side() ? job.side_bytes() : n_items + 64);
    lp.info = d_info; lp.emit_k = job.emit_k;
    if (ub > 0 && d_info)
        hipLaunchKernelGGL((local_sort_kernel<WT, true, true>), dim3((unsigned)l_blocks), dim3(kSortThreads), 0, stream, src, n_items, lp, d_big, d_big_count,
                           big_cap);
    else if (ub > 0)
        hipLaunchKernelGGL((local_sort_kernel<WT, true>), dim3((unsigned)l_blocks), dim3(kSortThreads), 0, stream, src, n_items, lp, d_big, d_big_count,
                           big_cap);
    else
        hipLaunchKernelGGL((local_sort_kernel<WT, false>), dim3((unsigned)l_blocks), dim3(kSortThreads), 0, stream, src, n_items, lp, d_big, d_big_count,
                           big_cap);
    t.end();
    uint32_t n_big = 0, n_lsd_tiles = 0;
    MGTA_HIP_CHECK(hipMemcpyAsync(&n_lsd_tiles, d_big_count + 1, 4, hipMemcpyDeviceToHost, stream));
    MGTA_HIP_CHECK(hipMemcpyAsync(&n_big, d_big_count, 4, hipMemcpyDeviceToHost, stream));
    MGTA_HIP_CHECK(hipStreamSynchronize(stream));
    const float ms_local = t.ms();
    if (n_big > big_cap) { set_error("more than %u oversized key segments in one pass", big_cap); return nullptr; }
    if (n_lsd_tiles > lp.lsd_cap) { set_error("internal: tile list overflow"); return nullptr; }
    if (ub > 0 && l_blocks >= 64 && 2 * (uint64_t)n_lsd_tiles > l_blocks) ctx->lsd_skip_left = 7;   // then look again
    t.start();
    if (n_lsd_tiles > 0 && !(lp.debug & 2))
        hipLaunchKernelGGL((local_lsd_kernel<WT>), dim3(n_lsd_tiles), dim3(kSortThreads), 0, stream, src, dst, d_lsd, d_lsd + 1, 2, lp);
    if (n_big > 0) {
        // segments that did not fit a tile next to their neighbours: alone in LDS if they fit, else (hot k-mers, conserved genes, or
        // the whole array when it is tiny) split level by level
        hipLaunchKernelGGL((segment_end_kernel<WT>), dim3(n_big), dim3(256), 0, stream, src, n_items, T, d_big, d_big + big_cap);
        hipLaunchKernelGGL((local_lsd_kernel<WT>), dim3(n_big), dim3(kSortThreads), 0, stream, src, dst, d_big, d_big + big_cap, 1, lp);
        const bool use_big = BigCfg<WT>::kTile > 0 && !low.empty();
        if (use_big) hipLaunchKernelGGL((segment_lds_kernel<WT>), dim3(n_big), dim3(kSortThreads), 0, stream, src, dst, d_big, d_big + big_cap, lp);
        if (!low.empty()) {
            const int levels = split_oversized<WT>(ctx, job, src, dst, d_big, d_big + big_cap, n_big, lp);
            if (levels < 0) return nullptr;
            ctx->split_levels = std::max(ctx->split_levels, levels);
        }
    }
    if (d_info) {
        if (n_lsd_tiles > 0)
            hipLaunchKernelGGL((emit_info_range_kernel<WT>), dim3(n_lsd_tiles), dim3(256), 0, stream, src, n_items, job.emit_k, d_lsd, d_lsd + 1, 2, d_info);
        if (n_big > 0)
            hipLaunchKernelGGL((emit_info_range_kernel<WT>), dim3(n_big), dim3(256), 0, stream, src, n_items, job.emit_k, d_big, d_big + big_cap, 1, d_info);
        *info_out = d_info;
    }
    t.end();
    MGTA_HIP_CHECK(hipEventSynchronize(t.b));
    const float ms = t.ms();
    if (log) { log->S->ms_local_sort += ms_local + ms; log->S->n_lsd_tiles += n_lsd_tiles; log->S->n_big_segments += n_big; }
    return src;
}

// Sort job.n keys (see SortJob).  Returns the buffer (a or b) that holds the result, nullptr on an unsupported input (error set).
template <int WT>
static Key<WT> *device_sort(mgta_ctx *ctx, const SortJob<WT> &job, SortLog *log = nullptr, const uint8_t **info_out = nullptr) {
    Key<WT> *src = global_passes(ctx, job, log);
    return src ? lds_finish(ctx, job, src, src == job.a ? job.b : job.a, log, info_out) : nullptr;
}

// ---- stage 1 (min_count >= 2): fills the is_solid bit-vector (+ mercy edges) that stage 2 then honours -------------
template <int W>
static int run_stage1(mgta_ctx *ctx, const mgta_reads *rd, uint64_t n_short, int k, int min_count, int need_mercy, uint64_t budget,
                      int side_mode, unsigned long long **is_solid_out, int *num_k1_out) {
    constexpr int WT = W + 2;                                          // key words (= words_per_substring of s1, s1.cpp:248) + 64-bit payload
    hipStream_t stream = ctx->stream;
    const uint64_t n_reads = rd->n_reads;
    const uint64_t n_blocks = (n_reads + kReadsPerBlock - 1) / kReadsPerBlock;
    uint64_t *d_small = pool_get<uint64_t>(ctx, S_SMALL, 4096);
    uint64_t *d_total = d_small;
    unsigned int *d_maxlen = reinterpret_cast<unsigned int *>(d_small + 300);
    unsigned long long *d_mercy_count = reinterpret_cast<unsigned long long *>(d_small + 302), *d_num_mercy = d_mercy_count + 1;
    MGTA_HIP_CHECK(hipMemsetAsync(d_small + 300, 0, 64, stream));
    if (n_short > n_reads) n_short = n_reads;
    if (n_short) hipLaunchKernelGGL(max_len_kernel, dim3((unsigned)((n_short + 255) / 256)), dim3(256), 0, stream, rd->d_start, n_short, d_maxlen);
    unsigned int max_len = 0;
    MGTA_HIP_CHECK(hipMemcpyAsync(&max_len, d_maxlen, 4, hipMemcpyDeviceToHost, stream));
    MGTA_HIP_CHECK(hipStreamSynchronize(stream));
    // base index -> read id table (one entry per 1024 bases, one past the end) and the left shift that puts the highest bit a mercy
    // candidate (base index << 2 | code) can have at bit 63
    if (n_reads >= 0xFFFFFFFFull) { set_error("stage 1: more than 2^32 reads"); return MGTA_EUNSUPPORTED; }
    const uint64_t bases_bound = rd->n_words * 16 + 16;
    const uint64_t n_pos_entries = (bases_bound >> kPosStepLog) + 2;
    uint32_t *d_pos2id = pool_get<uint32_t>(ctx, S_POS2ID, n_pos_entries * 4);
    hipLaunchKernelGGL(pos_to_id_kernel, dim3((unsigned)((n_pos_entries + 255) / 256)), dim3(256), 0, stream, rd->d_start, n_reads, n_pos_entries, d_pos2id);
    int cand_shift = 0;
    while (cand_shift < 40 && (((bases_bound << 2) | 3ull) << (cand_shift + 1)) >> (cand_shift + 1) == ((bases_bound << 2) | 3ull)) ++cand_shift;
    const int num_k1 = std::max<int>(0, (int)max_len - k);                 // num_k1_per_read, s1.cpp:152
    const uint64_t n_bits = (uint64_t)num_k1 * n_short;
    unsigned long long *d_solid = pool_get<unsigned long long>(ctx, S_SOLID, (n_bits / 64 + 2) * 8);
    MGTA_HIP_CHECK(hipMemsetAsync(d_solid, 0, (n_bits / 64 + 2) * 8, stream));
    unsigned long long *d_edge_count = pool_get<unsigned long long>(ctx, S_EDGE_COUNT, 65536 * 8);
    MGTA_HIP_CHECK(hipMemsetAsync(d_edge_count, 0, 65536 * 8, stream));
    uint32_t *d_block_count = pool_get<uint32_t>(ctx, S_BLOCK_COUNT, std::max<uint64_t>(1, n_blocks) * 4);
    uint64_t *d_block_base = pool_get<uint64_t>(ctx, S_BLOCK_BASE, std::max<uint64_t>(1, n_blocks) * 8);

    S1Args sa;
    sa.packed = rd->d_packed; sa.n_words = rd->n_words; sa.start = rd->d_start; sa.n_reads = n_reads; sa.k = k;
    sa.block_count = d_block_count; sa.block_base = d_block_base; sa.out = nullptr;
    Key<2> *d_mercy = nullptr;
    uint64_t mercy_cap = 0;
    int n_pass = 1;
    uint32_t b_lo = 0;
    while (b_lo < MGTA_NUM_BUCKETS) {
        uint32_t width = (MGTA_NUM_BUCKETS + n_pass - 1) / n_pass;
        uint32_t b_hi = std::min<uint32_t>(MGTA_NUM_BUCKETS, b_lo + width);
        sa.b_lo = b_lo; sa.b_hi = b_hi;
        uint64_t *d_scan_tmp = pool_get<uint64_t>(ctx, S_SCAN_TMP, scan_tmp_elems(std::max<uint64_t>(n_blocks, 1024)) * 8);
        if (n_blocks) hipLaunchKernelGGL((s1_scan_kernel<W, false>), dim3((unsigned)n_blocks), dim3(kScanBlock), 0, stream, sa);
        exclusive_scan_u32(stream, d_block_count, n_blocks, d_block_base, d_scan_tmp, d_total);
        uint64_t n_items = 0;
        MGTA_HIP_CHECK(hipMemcpyAsync(&n_items, d_total, 8, hipMemcpyDeviceToHost, stream));
        MGTA_HIP_CHECK(hipStreamSynchronize(stream));
        uint64_t n_tiles = (n_items + kBlockTile - 1) / kBlockTile;
        uint64_t need = 2 * n_items * sizeof(Key<WT>) + n_tiles * 256 * 8 + (need_mercy ? n_items * 8 : 0) + (8u << 20);
        uint64_t other = ctx->live_bytes - pool_bytes(ctx);
        if (need + need / 8 > budget - std::min<uint64_t>(budget, other) && width > 1) { n_pass *= 2; continue; }
        if (n_items > 0) {
            Key<WT> *d_a = pool_get<Key<WT>>(ctx, S_KEYS_A, n_items * sizeof(Key<WT>));
            Key<WT> *d_b = pool_get<Key<WT>>(ctx, S_KEYS_B, n_items * sizeof(Key<WT>));
            if (need_mercy && (!d_mercy || mercy_cap < 2 * n_items)) {
                // a candidate list that only grows: keep what earlier passes appended
                uint64_t have = 0;
                MGTA_HIP_CHECK(hipMemcpy(&have, d_mercy_count, 8, hipMemcpyDeviceToHost));
                uint64_t new_cap = have + 2 * n_items;
                DevBuf keep;
                if (have) { keep.alloc(have * 8); MGTA_HIP_CHECK(hipMemcpy(keep.p, d_mercy, have * 8, hipMemcpyDeviceToDevice)); }
                d_mercy = pool_get<Key<2>>(ctx, S_MERCY, new_cap * 8);
                if (have) MGTA_HIP_CHECK(hipMemcpy(d_mercy, keep.p, have * 8, hipMemcpyDeviceToDevice));
                mercy_cap = new_cap;
            }
            sa.out = d_a;
            hipLaunchKernelGGL((s1_scan_kernel<W, true>), dim3((unsigned)n_blocks), dim3(kScanBlock), 0, stream, sa);
            // sort on: key characters + head/tail (key words), then prev/next (low 6 bits of the payload); positions are ignored
            const int pad1 = 32 * W - 2 * (k - 1) - 6;
            auto low_plan = [&](int T) {
                std::vector<Digit> plan;
                int top = 32 * WT - T;
                plan.push_back(Digit{0, 6});
                if (top > 64) plan.push_back(Digit{64, std::min(6, top - 64)});
                for (int pos = 64 + 6 + pad1; pos < top; pos += 8) plan.push_back(Digit{pos, std::min(8, top - pos)});
                return plan;
            };
            const int max_top = std::min(4, std::max(0, (2 * (k - 1)) / 8));
            SortJob<WT> job{d_a, d_b, n_items, choose_top_plan(ctx, n_items, max_top, (double)(b_hi - b_lo) / MGTA_NUM_BUCKETS)};
            job.low = low_plan(job.top.T()); job.mask_last2 = 0u; job.mask_last = 0x3Fu; job.side_mode = side_mode;
            Key<WT> *sorted = device_sort(ctx, job);
            if (!sorted) return MGTA_EUNSUPPORTED;
            char *scratch = reinterpret_cast<char *>(sorted == d_a ? d_b : d_a);
            uint64_t e_tiles = (n_items + kEmitTile - 1) / kEmitTile;
            uint32_t *d_tile_heads = pool_get<uint32_t>(ctx, S_TILE_HEADS, e_tiles * 4);
            uint64_t *d_tile_base = pool_get<uint64_t>(ctx, S_TILE_BASE, e_tiles * 8);
            d_scan_tmp = pool_get<uint64_t>(ctx, S_SCAN_TMP, scan_tmp_elems(std::max<uint64_t>(n_blocks, e_tiles)) * 8);
            hipLaunchKernelGGL((s1_mark_kernel<W>), dim3((unsigned)e_tiles), dim3(kEmitThreads), 0, stream, sorted, n_items, d_tile_heads);
            exclusive_scan_u32(stream, d_tile_heads, e_tiles, d_tile_base, d_scan_tmp, d_total);
            uint64_t m = 0;
            MGTA_HIP_CHECK(hipMemcpyAsync(&m, d_total, 8, hipMemcpyDeviceToHost, stream));
            MGTA_HIP_CHECK(hipStreamSynchronize(stream));
            uint64_t *run_start = reinterpret_cast<uint64_t *>(scratch);               // 12 bytes per run <= sizeof(Key<WT>) per key
            uint16_t *run_info = reinterpret_cast<uint16_t *>(scratch + m * 8);
            uint16_t *group_mask = reinterpret_cast<uint16_t *>(scratch + m * 10);
            hipLaunchKernelGGL((s1_compact_kernel<W>), dim3((unsigned)e_tiles), dim3(kEmitThreads), 0, stream, sorted, n_items, k, d_tile_base,
                               run_start, run_info);
            unsigned rb = (unsigned)((m + 255) / 256);
            hipLaunchKernelGGL(s1_group_kernel, dim3(rb), dim3(256), 0, stream, run_start, run_info, m, n_items, min_count, group_mask);
            hipLaunchKernelGGL((s1_apply_kernel<W>), dim3(std::min(rb, 8192u)), dim3(256), 0, stream, sorted, run_start, run_info, group_mask, m, n_items, min_count,
                               k, rd->d_start, n_reads, n_short, num_k1, d_solid, d_edge_count, d_mercy, d_mercy_count, mercy_cap, need_mercy,
                               d_pos2id, cand_shift);
        }
        b_lo = b_hi;
    }
    // .counting histogram (s1_post_proc, s1.cpp:905-930)
    ctx->edge_counting.assign(65536, 0);
    MGTA_HIP_CHECK(hipMemcpyAsync(ctx->edge_counting.data(), d_edge_count, 65536 * 8, hipMemcpyDeviceToHost, stream));
    MGTA_HIP_CHECK(hipStreamSynchronize(stream));
    if (need_mercy) {
        uint64_t n_cand = 0;
        MGTA_HIP_CHECK(hipMemcpy(&n_cand, d_mercy_count, 8, hipMemcpyDeviceToHost));
        if (n_cand > mercy_cap) { set_error("mercy candidate list overflow"); return MGTA_ENOMEM; }
        if (n_cand > 0) {
            Key<2> *d_tmp = pool_get<Key<2>>(ctx, S_KEYS_A, n_cand * 8);
            auto low64 = [&](int T) {
                std::vector<Digit> plan;
                for (int pos = 0; pos < 64 - T; pos += 8) plan.push_back(Digit{pos, std::min(8, 64 - T - pos)});
                return plan;
            };
            SortJob<2> job{d_mercy, d_tmp, n_cand, choose_top_plan(ctx, n_cand, 4, 1.0)};
            job.low = low64(job.top.T()); job.side_mode = side_mode;
            Key<2> *cs = device_sort(ctx, job);
            if (!cs) return MGTA_EUNSUPPORTED;
            if ((int)max_len <= kMercyMaxLen) {
                hipLaunchKernelGGL(mercy_kernel<false>, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, stream, cs, n_cand, rd->d_start, n_reads, k,
                                   num_k1, d_solid, d_num_mercy, d_pos2id, cand_shift, (uint8_t *)nullptr, (uint64_t)0);
                MGTA_HIP_CHECK(hipGetLastError());
                MGTA_HIP_CHECK(hipStreamSynchronize(stream));
            } else {     // reads longer than the LDS flags hold: the flags of every wave go to device memory, a fixed grid walks the groups
                const uint64_t stride = ((uint64_t)max_len + 64 + 63) & ~63ull;
                const unsigned grid = (unsigned)std::min<uint64_t>((n_cand + 255) / 256, (uint64_t)ctx->num_cus * 8);
                DevBuf d_flags;
                d_flags.alloc((uint64_t)grid * 4 * 3 * stride, &ctx->live_bytes, &ctx->peak_bytes);
                hipLaunchKernelGGL(mercy_kernel<true>, dim3(grid), dim3(256), 0, stream, cs, n_cand, rd->d_start, n_reads, k, num_k1, d_solid,
                                   d_num_mercy, d_pos2id, cand_shift, d_flags.as<uint8_t>(), stride);
                MGTA_HIP_CHECK(hipGetLastError());
                MGTA_HIP_CHECK(hipStreamSynchronize(stream));
            }
        }
    }
    *is_solid_out = d_solid;
    *num_k1_out = num_k1;
    return MGTA_OK;
}

// ---- stage 2: a loop over bucket ranges (passes) that fit the memory budget; a pass counts its sort items, writes the keys, sorts
// them and emits the edges of its buckets
struct Pass {                                  // one bucket range [b_lo, b_hi) and what the stages make of it
    uint32_t b_lo = 0, b_hi = 0, width = 0;
    bool closed_form = false;                  // every bucket, no stage-1 verdicts: items and keys by the closed-form layout
    uint64_t n_items = 0, n_tiles = 0, key_b = 0;   // sort items, tiles of the global sort passes, bytes of each key buffer
    uint64_t n_edges = 0, n_large = 0, n_tips = 0;
    uint16_t *rec = nullptr, *large = nullptr; // the pass's output in the pool
    uint32_t *tips = nullptr;
    int64_t *first = nullptr;
    uint32_t nb() const { return b_hi - b_lo; }
};

template <int W>
struct Build {                                 // a build of keys of W words: what its stages share, and the stages
    mgta_ctx *ctx;
    hipStream_t stream = ctx->stream;
    const mgta_reads *rd = nullptr;
    uint64_t n_short = 0, n_blocks = 0;        // n_blocks: workgroups of the read scans (kReadsPerBlock reads each)
    int k = 0, words_per_tip = 0, min_count = 1, need_mercy = 0;
    uint32_t bucket_begin = 0, bucket_end = 0;
    mgta_edge_sink sink = nullptr; void *user = nullptr;
    SortModes modes;
    uint64_t budget = 0;                       // device bytes the build may hold
    bool acc = false;                          // mgta_ctx_keep_stream: the whole stream of every pass stays on the device
    ScanArgs sa{};
    uint64_t *d_block_base = nullptr, *d_total = nullptr, *d_kmers = nullptr, *d_tot3 = nullptr, *d_sentinel = nullptr;
    uint32_t multi_n = 0, multi_width = 0, multi_lo = 0;   // ranges counted ahead by one scan (rows of d_multi_count)
    uint32_t *d_multi_count = nullptr;
    // Fused first sort pass.  The digit a range's first global pass sorts on depends on the plan of its sort, and that on its item
    // count -- which the count scan is about to produce.  A scan of several ranges only runs after a wider attempt was refused, so
    // every range's count is estimated from that attempt's (its share of the buckets), the plan chosen from the estimate, and the
    // scan counts that plan's first digit per workgroup next to the items (fz_table: [range][digit value][workgroup]).  A pass
    // whose real plan equals the estimated one takes the fused writer; any other the plain route, its histogram unused.
    struct FusedAhead { bool on = false; TopPlan top; };
    FusedAhead fz_plan[kMaxFusedRanges];
    uint64_t *fz_table = nullptr;              // nullptr: the ranges ahead were counted without the digits
    uint64_t wide_items = 0;                   // items and buckets of the last attempt admit_pass refused
    uint32_t wide_nb = 0;
    bool fz_check_failed = false;              // MGTA_SORT_FUSED=2: the fused writer's output failed its check
    const uint8_t *sorted_info = nullptr;      // the info bytes the pass's sort left behind (MGTA_EMIT_FUSED), nullptr: the emitter reads the keys
    mgta_build_stats S{};
    Timer t_all{stream}, t_ph{stream};
    SortLog log{&S, {}};
    std::vector<int64_t> h_first, h_items;    // host staging of a pass
    std::vector<uint16_t> h_rec, h_large;
    std::vector<uint32_t> h_tips;
    explicit Build(mgta_ctx *c) : ctx(c) {}

    int run() {
        int rc = start();
        if (rc == MGTA_OK) rc = solid_from_stage1();
        if (rc != MGTA_OK) return rc;
        t_all.start();
        int n_pass = 1;
        for (uint32_t b_lo = bucket_begin; b_lo < bucket_end;) {
            Pass p;
            p.width = (bucket_end - bucket_begin + n_pass - 1) / n_pass;
            p.b_lo = b_lo; p.b_hi = std::min<uint32_t>(bucket_end, b_lo + p.width);
            count_pass(p);
            if (const int more = admit_pass(p, n_pass)) { n_pass = more; wide_items = p.n_items; wide_nb = p.nb(); continue; }
            S.n_items += (int64_t)p.n_items;
            S.n_passes++;
            if (p.n_items > 0) {
                Key<W> *a = pool_get<Key<W>>(ctx, S_KEYS_A, p.key_b), *b = pool_get<Key<W>>(ctx, S_KEYS_B, p.key_b);
                const SortJob<W> job = plan_sort(p, a, b);
                write_keys(p, job);
                if (fz_check_failed) { set_error("internal: the fused key writer left keys outside the slice of their first sort digit"); return MGTA_EINTERNAL; }
                Key<W> *sorted = sort_keys(job);
                if (!sorted) return MGTA_EUNSUPPORTED;
                if ((rc = drop_sentinels(p)) != MGTA_OK || (rc = emit(p, sorted, sorted == a ? b : a)) != MGTA_OK) return rc;
            }
            publish_last(p.b_lo, p.b_hi, p.rec, p.n_edges, p.tips, p.n_tips, p.first, p.large, p.n_large);   // (an empty range names no records)
            if (acc && p.n_items > 0) append_to_stream(p);
            S.n_edges += (int64_t)p.n_edges; S.n_large += (int64_t)p.n_large; S.n_tips += (int64_t)p.n_tips;
            if ((rc = deliver_pass(p)) != MGTA_OK) return rc;
            b_lo = p.b_hi;
        }
        if (acc) publish_last(bucket_begin, bucket_end, ctx->acc_rec.p, ctx->acc_n_rec, ctx->acc_tips.p, ctx->acc_n_tips, nullptr,
                              ctx->acc_has_large ? ctx->acc_large.p : nullptr, ctx->acc_n_large);
        ctx->acc_valid = acc;
        S.ms_total = t_all.stop();
        for (const Timer &t : log.scatter) S.ms_sort_scatter += t.ms();
        S.bytes_peak = ctx->peak_bytes;
        S.n_split_levels = ctx->split_levels;
        return MGTA_OK;
    }

    // stats, memory budget, the whole-stream hand-off and the scan's fixed arguments
    int start() {
        words_per_tip = (2 * k + 31) / 32;                             // sdbg_multi_io.h:63
        n_blocks = (rd->n_reads + kReadsPerBlock - 1) / kReadsPerBlock;
        // the scan kernels run one workgroup of kScanBlock threads per kReadsPerBlock reads: a dispatch holds fewer than 2^32 work-items
        if (n_blocks * (uint64_t)kScanBlock >= (1ull << 32)) { set_error("too many reads for one launch (%llu)", (unsigned long long)rd->n_reads); return MGTA_EUNSUPPORTED; }
        S.k = k; S.words_per_key = W; S.words_per_tip = words_per_tip; S.n_reads = (int64_t)rd->n_reads;
        ctx->peak_bytes = ctx->live_bytes;
        ctx->split_levels = 0;
        ctx->emit_fused_passes = 0;
        size_t free_b = 0, total_b = 0;
        MGTA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        // what the build may hold: the explicit limit, else 90 % of (free + what our pool already holds)
        const uint64_t avail = (uint64_t)free_b + pool_bytes(ctx);
        budget = ctx->mem_limit ? std::min<uint64_t>(ctx->mem_limit, avail) : (uint64_t)(avail * 0.9);
        acc = ctx->keep_stream != 0;           // (of a bucket sub-range too: the shard a rank hands to the all-gather)
        ctx->acc_valid = false; ctx->acc_n_rec = 0; ctx->acc_n_tips = 0;
        ctx->acc_n_large = 0; ctx->acc_has_large = acc && ctx->keep_multiplicity;   // (the large words stay with a kept stream only on request)
        if (acc) ctx->acc_items.assign(MGTA_NUM_BUCKETS, 0);
        point_scans_at_pool();
        uint64_t *d_small = pool_get<uint64_t>(ctx, S_SMALL, 4096);   // [0] total, [1] kmers, [2..4] emit totals, [5] sentinels (the digit totals of the sort: S_DIGIT_TOTALS)
        d_total = d_small; d_kmers = d_small + 1; d_tot3 = d_small + 2; d_sentinel = d_small + 5;
        sa.packed = rd->d_packed; sa.n_words = rd->n_words; sa.start = rd->d_start; sa.n_reads = rd->n_reads; sa.k = k; sa.n_short = n_short;
        sa.n_kmers = (unsigned long long *)d_kmers; sa.n_sentinel = (unsigned long long *)d_sentinel;
        return MGTA_OK;
    }
    void point_scans_at_pool() {               // the scans' per-workgroup counts and offsets
        sa.block_count = pool_get<uint32_t>(ctx, S_BLOCK_COUNT, std::max<uint64_t>(1, n_blocks) * 4);
        sa.block_base = d_block_base = pool_get<uint64_t>(ctx, S_BLOCK_BASE, std::max<uint64_t>(1, n_blocks) * 8);
    }

    // min_count >= 2: the stage-1 verdicts the scans honour
    int solid_from_stage1() {
        if (min_count <= 1) return MGTA_OK;
        unsigned long long *sol = nullptr;
        int nk1 = 0;
        t_ph.start();
        const int rc = run_stage1<W>(ctx, rd, n_short, k, min_count, need_mercy, budget, modes.side, &sol, &nk1);
        if (rc != MGTA_OK) return rc;
        S.ms_stage1 = t_ph.stop();
        sa.is_solid = sol; sa.num_k1_per_read = nk1;
        point_scans_at_pool();                 // run_stage1 may have re-grown pool slots
        return MGTA_OK;
    }

    // ---- 1./2. items per workgroup and their prefix sum: the closed form, the counting scan, or the row of a scan that counted
    // every range ahead; the first pass also totals the (k+1)-mers
    void count_pass(Pass &p) {
        const bool first_pass = S.n_passes == 0;
        t_ph.start();
        sa.b_lo = p.b_lo; sa.b_hi = p.b_hi;
        sa.n_kmers = first_pass ? (unsigned long long *)d_kmers : nullptr;
        if (first_pass) MGTA_HIP_CHECK(hipMemsetAsync(d_kmers, 0, 8, stream));
        uint64_t *d_scan_tmp = pool_get<uint64_t>(ctx, S_SCAN_TMP, scan_tmp_elems(std::max<uint64_t>(n_blocks, 1024)) * 8);
        static_assert(kReadsPerBlock == 64, "item_count_closed_kernel: one lane per read of a workgroup");
        p.closed_form = !sa.is_solid && p.b_lo == 0 && p.b_hi == (uint32_t)MGTA_NUM_BUCKETS && !ctx->force_full_lsd;
        const uint32_t *counts = sa.block_count;
        sa.multi_n = 0; sa.multi_width = 0; sa.multi_magic = 0;
        // the k-mer total of the first pass comes from the read lengths alone, for the scans too: one atomic per wave of the scan on
        // ONE address (6.25 M of them at 100 M reads) kept the count scan at 80 ms where the write scan, which does more, takes 52
        if (n_blocks && (p.closed_form || sa.n_kmers))
            hipLaunchKernelGGL(item_count_closed_kernel, dim3((unsigned)((n_blocks + 63) / 64)), dim3(256), 0, stream, sa.start, sa.n_reads, n_blocks, k,
                               p.closed_form ? sa.block_count : nullptr, sa.n_kmers);
        if (n_blocks && !p.closed_form) {
            sa.n_kmers = nullptr;
            // several equally wide ranges ahead (memory-bound passes): one scan counts them all
            const uint32_t width = p.width, b_lo = p.b_lo, ranges_left = (bucket_end - b_lo + width - 1) / width;
            if (multi_n && (width != multi_width || b_lo < multi_lo || (b_lo - multi_lo) % width != 0 || (b_lo - multi_lo) / width >= multi_n)) multi_n = 0;
            if (!multi_n && ranges_left > 1 && ranges_left <= (uint32_t)kMaxCountRanges) {
                d_multi_count = pool_get<uint32_t>(ctx, S_MULTI_COUNT, (uint64_t)ranges_left * n_blocks * 4);
                ScanArgs sm = sa;
                sm.block_count = d_multi_count; sm.b_hi = bucket_end; sm.multi_width = width; sm.multi_n = ranges_left; sm.multi_magic = ((1ull << 32) + width - 1) / width;
                fz_table = nullptr;
                if (plan_ahead(sm, b_lo, width, ranges_left)) {
                    fz_table = sm.fz_hist = pool_get<uint64_t>(ctx, S_FUSED_HIST, fused_table_bytes(ranges_left));
                    if constexpr (W >= 2)      // (plan_ahead refuses keys of one word: no such kernels are built)
                        hipLaunchKernelGGL((item_scan_kernel<W, false, true>), dim3((unsigned)n_blocks), dim3(kScanBlock), 0, stream, sm);
                } else
                    hipLaunchKernelGGL((item_scan_kernel<W, false>), dim3((unsigned)n_blocks), dim3(kScanBlock), 0, stream, sm);
                multi_n = ranges_left; multi_width = width; multi_lo = b_lo;
            }
            if (multi_n) counts = d_multi_count + (uint64_t)((b_lo - multi_lo) / width) * n_blocks;
            else hipLaunchKernelGGL((item_scan_kernel<W, false>), dim3((unsigned)n_blocks), dim3(kScanBlock), 0, stream, sa);
        }
        exclusive_scan_u32(stream, counts, n_blocks, d_block_base, d_scan_tmp, d_total);
        MGTA_HIP_CHECK(hipMemcpyAsync(&p.n_items, d_total, 8, hipMemcpyDeviceToHost, stream));
        S.ms_count += t_ph.stop();
        if (first_pass) {
            unsigned long long km = 0;
            MGTA_HIP_CHECK(hipMemcpy(&km, d_kmers, 8, hipMemcpyDeviceToHost));
            S.n_kmers = (int64_t)km;
        }
    }

    int max_top() const { return (2 * k + 4 + 7) / 8 > 1 ? std::min(4, (32 * W - 8) / 8) : 0; }
    // the global passes of a sort of n_items keys of the buckets [b_lo, b_hi)
    TopPlan top_plan(uint64_t n_items, uint32_t b_lo, uint32_t b_hi) const {
        const double frac = (double)(b_hi - b_lo) / MGTA_NUM_BUCKETS;
        const TopPlan tp = choose_top_plan(ctx, n_items, max_top(), frac, b_lo, b_hi, modes.bias);
        if (!kWideFits<W> || ctx->force_full_lsd) return tp;
        return widen_top_plan(tp, n_items, max_top(), frac, b_lo, b_hi, modes.bias, modes.wide);
    }
    uint64_t fused_table_bytes(uint32_t ranges) const { return (uint64_t)ranges * 256 * std::max<uint64_t>(1, n_blocks) * 8; }

    // The plan of every range the count scan is about to count (see fz_plan), into the scan's arguments.  False: count without the
    // digits -- no estimate (first attempt of the build), too many ranges, keys of one word (flags share word 0 with the digit), no
    // range with a global pass, or a table that would not fit the budget next to a pass of the estimated size.
    bool plan_ahead(ScanArgs &sm, uint32_t b_lo, uint32_t width, uint32_t ranges) {
        for (FusedAhead &f : fz_plan) f = FusedAhead{};
        if (modes.fused <= 0 || W < 2 || !wide_nb || ranges > (uint32_t)kMaxFusedRanges) return false;
        bool any = false;
        int max_width = 8;
        uint64_t est_max = 0;
        for (uint32_t g = 0; g < ranges; ++g) {
            const uint32_t lo = b_lo + g * width, hi = std::min<uint32_t>(bucket_end, lo + width);
            const uint64_t est = (uint64_t)((double)wide_items * (double)(hi - lo) / (double)wide_nb);
            const TopPlan tp = top_plan(est, lo, hi);
            est_max = std::max(est_max, est);
            max_width = std::max(max_width, tp.max_width());
            sm.fz_bias[g] = 0; sm.fz_shift[g] = 0;
            if (tp.P < 1 || tp.T() > 32) continue;
            fz_plan[g] = FusedAhead{true, tp};
            sm.fz_bias[g] = tp.bias; sm.fz_shift[g] = (uint32_t)(32 - tp.T());
            any = true;
        }
        if (!any) return false;
        uint64_t key_b = 0;
        const uint64_t need = pass_need(est_max, &key_b, max_width) + fused_table_bytes(ranges);
        return need + need / 8 <= avail_bytes();
    }

    // device bytes of a pass of n_items (two key buffers, the second doubles as emit scratch, + census + outputs (estimate) + the range
    // lists of the oversized segments, sized for the worst case)
    // max_width: of the global passes' digits (side entries of 2 bytes and a census row per value of a digit wider than 8 bits)
    uint64_t pass_need(uint64_t n_items, uint64_t *key_b, int max_width) const {
        const uint64_t n_tiles = (n_items + kBlockTile - 1) / kBlockTile;
        // either key buffer may end up as the emitter's scratch (11 bytes per key: run start u64, record u16, info u8), whichever
        // the last sort pass leaves idle: both hold >= 12 bytes per key
        *key_b = std::max<uint64_t>(n_items * sizeof(Key<W>), n_items * 12) + 4096;
        return 2 * *key_b + n_tiles * ((uint64_t)8 << max_width) + n_items * 2 + n_items * (max_width > 8 ? 2 : 1) /* side digits */ + split_list_bytes<W>(n_items) +
               (8u << 20);
    }
    uint64_t avail_bytes() const {
        uint64_t other = ctx->live_bytes - pool_bytes(ctx);
        if (acc) {     // room for the stream the passes leave behind: ~0.6 edges of 2 bytes per (k+1)-mer, tips, slack
            const double range_frac = (double)(bucket_end - bucket_begin) / (double)MGTA_NUM_BUCKETS;
            const uint64_t est = (uint64_t)((double)S.n_kmers * 1.5 * range_frac) + (64ull << 20);
            const uint64_t have = ctx->acc_rec.bytes + ctx->acc_tips.bytes;
            other += est > have ? est - have : 0;
        }
        return budget - std::min<uint64_t>(budget, other);
    }

    // Does the pass fit?  0: it does, else the number of passes to split the buckets into instead (narrower bucket ranges: CX1's
    // lv1 loop, cx1.h:494).  The table of a fused first pass counts as long as the pool holds it; where the pass only fits without,
    // the table goes and the ranges it covered take the plain route.
    int admit_pass(Pass &p, int n_pass) {
        p.n_tiles = (p.n_items + kBlockTile - 1) / kBlockTile;
        uint64_t need = pass_need(p.n_items, &p.key_b, top_plan(p.n_items, p.b_lo, p.b_hi).max_width());
        const uint64_t avail = avail_bytes();
        if ((int)ctx->pool.size() > S_FUSED_HIST && ctx->pool[S_FUSED_HIST].bytes) {
            const uint64_t with = need + ctx->pool[S_FUSED_HIST].bytes;
            if (with + with / 8 <= avail) need = with;
            else if (need + need / 8 <= avail) { ctx->pool[S_FUSED_HIST].release(); fz_table = nullptr; }   // (else refused either way)
        }
        if (need + need / 8 <= avail || p.width <= 1) return 0;
        const double ratio = (double)(need + need / 8) / (double)std::max<uint64_t>(avail, 1) * 1.03;
        return std::max(n_pass + 1, (int)std::ceil((double)n_pass * ratio));
    }

    // the one plan of the pass's sort, for the key writer and the sort
    SortJob<W> plan_sort(const Pass &p, Key<W> *a, Key<W> *b) const {
        SortJob<W> job{a, b, p.n_items, top_plan(p.n_items, p.b_lo, p.b_hi)};
        job.low = low_digit_plan(k, W, job.top.T());
        job.side_mode = modes.side;
        job.emit_k = modes.emit_fused > 0 ? k : 0;
        // closed form + at least one global sort pass: the key writer works tile by tile of that pass and leaves its census behind;
        // the general writer leaves that pass's digit of every key in the side array instead
        job.census_done = p.closed_form && job.top.P >= 1 && p.n_tiles <= 0x7FFFFFFFull;
        job.side_done = !p.closed_form && job.uses_side();
        // the count scan counted this range's first global pass ahead, and for the plan the real count gives: the writer does that pass
        // (and leaves the side digits of the next one)
        if (!p.closed_form && fz_table && multi_n && p.width == multi_width && p.b_lo >= multi_lo && (p.b_lo - multi_lo) % p.width == 0) {
            const uint32_t g = (p.b_lo - multi_lo) / p.width;
            if (g < multi_n && g < (uint32_t)kMaxFusedRanges) {
                const FusedAhead &f = fz_plan[g];
                job.first_pass_done = f.on && job.top.P >= 1 && f.top.same_digits(job.top);
            }
        }
        return job;
    }

    // ---- 3. the keys, into job.a
    void write_keys(const Pass &p, const SortJob<W> &job) {
        t_ph.start();
        sa.out = job.a;
        if (p.closed_form) MGTA_HIP_CHECK(hipMemsetAsync(d_sentinel, 0, 8, stream));
        const int shift = 32 - job.top.T();    // of the first global pass's digit in key word 0
        if (job.census_done) {
            uint64_t *d_hist = pool_get<uint64_t>(ctx, S_HIST, job.hist_bytes());   // the buffer the sort uses
            hipLaunchKernelGGL((item_write_tiled_kernel<W>), dim3((unsigned)p.n_tiles), dim3(kScanBlock), 0, stream, sa, n_blocks, p.n_items,
                               shift, p.n_tiles, d_hist);
        } else if (p.closed_form)
            hipLaunchKernelGGL((item_write_closed_kernel<W>), dim3((unsigned)n_blocks), dim3(kScanBlock), 0, stream, sa);
        else if (job.first_pass_done) {
            // the range's table -> row offsets and digit totals, as for a scatter whose tiles are the scan's workgroups
            uint64_t *tab = fz_table + (uint64_t)((p.b_lo - multi_lo) / p.width) * 256 * n_blocks;
            uint64_t *d_totals = digit_totals(ctx);
            hipLaunchKernelGGL(radix_rowscan_kernel, dim3(256), dim3(1024), 0, stream, tab, n_blocks, d_totals);
            sa.fz_hist = tab; sa.fz_totals = d_totals; sa.fz_n = p.n_items;
            sa.fz_bias[0] = job.top.bias; sa.fz_shift[0] = (uint32_t)shift;
            if (job.side_done) {               // the digit of the pass that now runs first: the 8 to 10 bits above
                sa.side = pool_get<uint8_t>(ctx, S_SIDE, job.side_bytes());
                sa.side_shift = shift + 8;
                sa.side_bias = job.top.bias;
                sa.side_bits = job.top.P >= 2 ? job.top.width[job.top.P - 2] : 8;
            }
            if constexpr (W >= 2)
                hipLaunchKernelGGL((item_write_fused_kernel<W>), dim3((unsigned)n_blocks), dim3(kScanBlock), 0, stream, sa);
            sa.side = nullptr; sa.fz_hist = nullptr; sa.fz_totals = nullptr;
            S.n_fused_passes++;
            if (modes.fused >= 2) {            // (test aid)
                uint32_t *d_bad = reinterpret_cast<uint32_t *>(pool_get<uint64_t>(ctx, S_SMALL, 4096) + 320);
                uint32_t bad[2] = {0, 0};
                MGTA_HIP_CHECK(hipMemsetAsync(d_bad, 0, 8, stream));
                const unsigned grid = (unsigned)std::min<uint64_t>((p.n_items + kScanBlock - 1) / kScanBlock, (uint64_t)ctx->num_cus * 16);
                hipLaunchKernelGGL((fused_check_kernel<W>), dim3(grid), dim3(kScanBlock), 0, stream, job.a, p.n_items, d_totals, job.top.bias, (uint32_t)shift, d_bad);
                MGTA_HIP_CHECK(hipMemcpyAsync(bad, d_bad, 8, hipMemcpyDeviceToHost, stream));
                MGTA_HIP_CHECK(hipStreamSynchronize(stream));
                if (bad[0] || bad[1]) fz_check_failed = true;
            }
        } else {
            if (job.side_done) {
                sa.side = pool_get<uint8_t>(ctx, S_SIDE, job.side_bytes());
                sa.side_shift = shift;
                sa.side_bias = job.top.bias;
                sa.side_bits = 8;
            }
            hipLaunchKernelGGL((item_scan_kernel<W, true>), dim3((unsigned)n_blocks), dim3(kScanBlock), 0, stream, sa);
            sa.side = nullptr;
        }
        S.ms_gen += t_ph.stop();
    }

    // ---- 4. sort: P global passes on the most significant bytes, then the segment-local finish in LDS
    Key<W> *sort_keys(const SortJob<W> &job) {
        t_ph.start();
        Key<W> *sorted = device_sort(ctx, job, &log, &sorted_info);
        if (sorted) S.ms_sort += t_ph.stop();
        return sorted;
    }

    // sentinel keys (rc slots of palindromic (k+1)-mers of a closed-form pass, k+1 even) sort behind every real key: the emitter stops before them
    int drop_sentinels(Pass &p) {
        if (!p.closed_form || ((k + 1) & 1)) return MGTA_OK;
        unsigned long long n_sent = 0;
        MGTA_HIP_CHECK(hipMemcpy(&n_sent, d_sentinel, 8, hipMemcpyDeviceToHost));
        if (n_sent >= p.n_items) { set_error("internal: %llu sentinel keys among %llu items", n_sent, (unsigned long long)p.n_items); return MGTA_EINTERNAL; }
        p.n_items -= n_sent;
        S.n_items -= (int64_t)n_sent;
        return MGTA_OK;
    }

    // ---- 5. the edges of the `sorted` keys; the other key buffer is scratch
    int emit(Pass &p, const Key<W> *sorted, Key<W> *scratch_keys) {
        const uint64_t n_items = p.n_items;
        t_ph.start();
        char *scratch = reinterpret_cast<char *>(scratch_keys);
        uint64_t e_tiles = (n_items + kEmitTile - 1) / kEmitTile;
        uint64_t *d_scan_tmp = pool_get<uint64_t>(ctx, S_SCAN_TMP, scan_tmp_elems(std::max<uint64_t>(std::max(n_blocks, e_tiles), n_items / kDecideTile + 1)) * 8);
        // run descriptors, compacted in key order in one read of the keys (chained scan over the tiles).  Scratch layout for up to
        // n_items runs (<= 7.01 bytes per key of a >= 12-byte-per-key buffer): start u32 | rec u16 (three-step route) | info u8, on a
        // 16-byte boundary | full start u64 per 1024 runs
        if (e_tiles > 0xFFFFFFFFull) { set_error("too many emit tiles"); return MGTA_EUNSUPPORTED; }
        unsigned long long *d_chain = pool_get<unsigned long long>(ctx, S_TILE_BASE, (e_tiles + 4) * 8);
        RunStarts sub_start;
        sub_start.lo = reinterpret_cast<uint32_t *>(scratch);
        uint16_t *rec = reinterpret_cast<uint16_t *>(scratch + n_items * 4);
        const uint64_t info_at = (n_items * 6 + 15) & ~15ull;
        uint8_t *info = reinterpret_cast<uint8_t *>(scratch + info_at);
        sub_start.base = reinterpret_cast<uint64_t *>(scratch + ((info_at + n_items + 15) & ~15ull));
        unsigned long long *d_dollar = reinterpret_cast<unsigned long long *>(pool_get<uint64_t>(ctx, S_SMALL, 4096) + 64);   // [kDollarSlots]
        // from the info bytes the sort left behind where it did (MGTA_EMIT_FUSED), else from the keys; returns the number of runs and
        // how many of them have a = $
        auto compact = [&](const uint8_t *key_info, RunStarts st, uint8_t *st_info, uint64_t *m_out, uint64_t *n_dollar_out) {
            unsigned long long chain_out[3] = {0, 0, 0};           // total, ticket, error
            unsigned long long dollar[kDollarSlots];
            const uint64_t tiles = key_info ? (n_items + kInfoTile - 1) / kInfoTile : e_tiles;   // (<= e_tiles: the chain's buffer holds either)
            EmitChain chain;
            chain.state = d_chain; chain.total = d_chain + tiles; chain.dollar = d_dollar;
            chain.ticket = reinterpret_cast<uint32_t *>(d_chain + tiles + 1); chain.error = reinterpret_cast<uint32_t *>(d_chain + tiles + 2);
            for (int attempt = 0; attempt < 2; ++attempt) {
                MGTA_HIP_CHECK(hipMemsetAsync(d_chain, 0, (tiles + 4) * 8, stream));
                MGTA_HIP_CHECK(hipMemsetAsync(d_dollar, 0, sizeof(dollar), stream));
                const bool ticket = !(attempt == 0 && !ctx->force_full_lsd);
                const dim3 grid((unsigned)tiles), block(kEmitThreads);
                if (key_info && !ticket)
                    hipLaunchKernelGGL((emit_compact_info_kernel<false>), grid, block, 0, stream, key_info, n_items, chain, (uint32_t)tiles, st, st_info);
                else if (key_info)
                    hipLaunchKernelGGL((emit_compact_info_kernel<true>), grid, block, 0, stream, key_info, n_items, chain, (uint32_t)tiles, st, st_info);
                else if (!ticket)
                    hipLaunchKernelGGL((emit_compact_kernel<W, false>), grid, block, 0, stream, sorted, n_items, k, chain, (uint32_t)tiles, st, st_info);
                else
                    hipLaunchKernelGGL((emit_compact_kernel<W, true>), grid, block, 0, stream, sorted, n_items, k, chain, (uint32_t)tiles, st, st_info);
                MGTA_HIP_CHECK(hipMemcpyAsync(chain_out, d_chain + tiles, 24, hipMemcpyDeviceToHost, stream));
                MGTA_HIP_CHECK(hipMemcpyAsync(dollar, d_dollar, sizeof(dollar), hipMemcpyDeviceToHost, stream));
                MGTA_HIP_CHECK(hipStreamSynchronize(stream));
                if ((uint32_t)chain_out[2] == 0) break;
            }
            if ((uint32_t)chain_out[2] != 0) { set_error("internal: chained scan of the emitter timed out"); return MGTA_EINTERNAL; }
            *m_out = chain_out[0];
            *n_dollar_out = 0;
            for (unsigned long long d : dollar) *n_dollar_out += d;
            return MGTA_OK;
        };
        uint64_t m = 0, n_dollar = 0;
        if (int rc = compact(sorted_info, sub_start, info, &m, &n_dollar)) return rc;
        if (sorted_info) {
            ctx->emit_fused_passes++;
            if (modes.emit_fused >= 2) {       // (test aid) the same from the keys, into the part of the scratch that is still idle
                RunStarts ref;
                uint8_t *ref_info = reinterpret_cast<uint8_t *>(rec);          // (the records are written by emit_decide_kernel)
                char *behind = reinterpret_cast<char *>(sub_start.base + (n_items >> kRunBaseStepLog) + 1);
                ref.lo = reinterpret_cast<uint32_t *>(behind);                 // <= 11.02 bytes per key in all
                ref.base = reinterpret_cast<uint64_t *>(behind + ((n_items * 4 + 7) & ~7ull));
                if ((uint64_t)(reinterpret_cast<char *>(ref.base + (n_items >> kRunBaseStepLog) + 1) - scratch) > p.key_b) {
                    set_error("internal: no room to check the emitter's info bytes");
                    return MGTA_EINTERNAL;
                }
                uint64_t m_ref = 0, n_dollar_ref = 0;
                if (int rc = compact(nullptr, ref, ref_info, &m_ref, &n_dollar_ref)) return rc;
                if (n_dollar_ref != n_dollar) { set_error("internal: the info bytes of the sort give %llu runs with a = $, the keys %llu",
                                                          (unsigned long long)n_dollar, (unsigned long long)n_dollar_ref); return MGTA_EINTERNAL; }
                uint32_t *d_bad = reinterpret_cast<uint32_t *>(pool_get<uint64_t>(ctx, S_SMALL, 4096) + 320);
                uint32_t bad[2] = {0, 0};
                MGTA_HIP_CHECK(hipMemsetAsync(d_bad, 0, 8, stream));
                const uint64_t m_min = std::min(m, m_ref);
                if (m_min > 0) {
                    const unsigned grid = (unsigned)std::min<uint64_t>((m_min + 255) / 256, (uint64_t)ctx->num_cus * 16);
                    hipLaunchKernelGGL(emit_check_kernel, dim3(grid), dim3(256), 0, stream, sub_start.lo, info, ref.lo, ref_info, m_min, d_bad);
                }
                MGTA_HIP_CHECK(hipMemcpyAsync(bad, d_bad, 8, hipMemcpyDeviceToHost, stream));
                MGTA_HIP_CHECK(hipStreamSynchronize(stream));
                if (m != m_ref || bad[0] || bad[1]) {
                    set_error("internal: the info bytes of the sort give %llu runs, the keys %llu; %u starts and %u info bytes differ",
                              (unsigned long long)m, (unsigned long long)m_ref, bad[0], bad[1]);
                    return MGTA_EINTERNAL;
                }
            }
        }
        // the runs decided and their records written: by one kernel, by the three steps, or by both (MGTA_EMIT_CHAIN)
        struct Out { uint16_t *rec = nullptr, *large = nullptr; uint32_t *tips = nullptr; int64_t *first = nullptr; uint64_t tot[3] = {0, 0, 0}; };
        DevBuf t_rec, t_large, t_tips, t_first;                    // MGTA_EMIT_CHAIN=2: what the three steps write, next to the pass's own output
        auto room = [&](bool pooled, int slot, DevBuf &tmp, uint64_t bytes) -> void * {
            if (pooled) return pool_get<char>(ctx, slot, bytes);
            tmp.alloc(bytes, &ctx->live_bytes, &ctx->peak_bytes);
            return tmp.p;
        };
        const uint64_t first_b = (uint64_t)MGTA_NUM_BUCKETS * 3 * 8;
        // E3 per-tile counts, three scans, the totals to the host to size the outputs, E5
        auto three_steps = [&](bool pooled, Out &o) -> int {
            const uint64_t d_tiles = (m + kDecideTile - 1) / kDecideTile;
            uint32_t *ce = pool_get<uint32_t>(ctx, S_CNT, d_tiles * 4 * 3), *cl = ce + d_tiles, *ct = cl + d_tiles;
            uint64_t *be = pool_get<uint64_t>(ctx, S_BASE, d_tiles * 8 * 3), *bl = be + d_tiles, *bt = bl + d_tiles;
            o.first = static_cast<int64_t *>(room(pooled, S_FIRST, t_first, first_b));
            MGTA_HIP_CHECK(hipMemsetAsync(o.first, 0xFF, (uint64_t)p.nb() * 3 * 8, stream));
            hipLaunchKernelGGL(emit_decide_kernel, dim3((unsigned)d_tiles), dim3(kDecideThreads), 0, stream, sub_start, info, m, n_items,
                               rec, ce, cl, ct);
            exclusive_scan_u32(stream, ce, d_tiles, be, d_scan_tmp, d_tot3);
            exclusive_scan_u32(stream, cl, d_tiles, bl, d_scan_tmp, d_tot3 + 1);
            exclusive_scan_u32(stream, ct, d_tiles, bt, d_scan_tmp, d_tot3 + 2);
            MGTA_HIP_CHECK(hipMemcpyAsync(o.tot, d_tot3, 24, hipMemcpyDeviceToHost, stream));
            MGTA_HIP_CHECK(hipStreamSynchronize(stream));
            o.rec = static_cast<uint16_t *>(room(pooled, S_OUT_REC, t_rec, o.tot[0] * 2));
            o.large = static_cast<uint16_t *>(room(pooled, S_OUT_LARGE, t_large, o.tot[1] * 2));
            o.tips = static_cast<uint32_t *>(room(pooled, S_OUT_TIPS, t_tips, o.tot[2] * words_per_tip * 4));
            hipLaunchKernelGGL((emit_write_kernel<W>), dim3((unsigned)d_tiles), dim3(kDecideThreads), 0, stream, sorted, sub_start, info, rec, m,
                               n_items, be, bl, bt, words_per_tip, p.b_lo, o.rec, o.large, o.tips, o.first);
            return MGTA_OK;
        };
        // One kernel.  The outputs are sized before the totals are known: at most m records (the planner's n_items * 2 bytes of output
        // cover them), a run above 254 holds at least 255 keys, and a tip is a run whose a is $.
        auto chained = [&](Out &o) -> int {
            if ((m >> kChainTipBits) != 0 || ((n_items / 255) >> (62 - kChainTipBits)) != 0) {
                set_error("too many runs (%llu) or keys (%llu) for the emitter's chained scan", (unsigned long long)m, (unsigned long long)n_items);
                return MGTA_EUNSUPPORTED;
            }
            const uint64_t tiles = (m + kChainTile - 1) / kChainTile;                  // (2 tiles + 2 <= e_tiles + 4 words of d_chain)
            DecideChain dc;
            dc.state_e = d_chain; dc.state_lt = d_chain + tiles; dc.totals = d_tot3;
            dc.ticket = reinterpret_cast<uint32_t *>(d_chain + 2 * tiles); dc.error = reinterpret_cast<uint32_t *>(d_chain + 2 * tiles + 1);
            o.rec = pool_get<uint16_t>(ctx, S_OUT_REC, m * 2);
            o.large = pool_get<uint16_t>(ctx, S_OUT_LARGE, (n_items / 255 + 1) * 2);
            o.tips = pool_get<uint32_t>(ctx, S_OUT_TIPS, n_dollar * words_per_tip * 4);
            o.first = pool_get<int64_t>(ctx, S_FIRST, first_b);
            unsigned long long err = 0;
            for (int attempt = 0; attempt < 2; ++attempt) {
                MGTA_HIP_CHECK(hipMemsetAsync(d_chain, 0, (2 * tiles + 2) * 8, stream));
                MGTA_HIP_CHECK(hipMemsetAsync(d_tot3, 0, 24, stream));
                MGTA_HIP_CHECK(hipMemsetAsync(o.first, 0xFF, (uint64_t)p.nb() * 3 * 8, stream));
                const dim3 grid((unsigned)tiles), block(kDecideThreads);
                if (attempt == 0 && !ctx->force_full_lsd)
                    hipLaunchKernelGGL((emit_decide_write_kernel<W, false>), grid, block, 0, stream, sorted, sub_start, info, m, n_items, dc, (uint32_t)tiles,
                                       words_per_tip, p.b_lo, o.rec, o.large, o.tips, o.first);
                else
                    hipLaunchKernelGGL((emit_decide_write_kernel<W, true>), grid, block, 0, stream, sorted, sub_start, info, m, n_items, dc, (uint32_t)tiles,
                                       words_per_tip, p.b_lo, o.rec, o.large, o.tips, o.first);
                MGTA_HIP_CHECK(hipMemcpyAsync(o.tot, d_tot3, 24, hipMemcpyDeviceToHost, stream));
                MGTA_HIP_CHECK(hipMemcpyAsync(&err, d_chain + 2 * tiles + 1, 8, hipMemcpyDeviceToHost, stream));
                MGTA_HIP_CHECK(hipStreamSynchronize(stream));
                if ((uint32_t)err == 0) break;
            }
            if ((uint32_t)err != 0) { set_error("internal: chained scan of the emitter's records timed out"); return MGTA_EINTERNAL; }
            if (o.tot[0] > m || o.tot[1] > n_items / 255 + 1 || o.tot[2] > n_dollar) {
                set_error("internal: the emitter wrote %llu records, %llu large counts and %llu tips into room for %llu, %llu and %llu", (unsigned long long)o.tot[0],
                          (unsigned long long)o.tot[1], (unsigned long long)o.tot[2], (unsigned long long)m, (unsigned long long)(n_items / 255 + 1), (unsigned long long)n_dollar);
                return MGTA_EINTERNAL;
            }
            return MGTA_OK;
        };
        Out out, ref;
        if (modes.emit_chain <= 0) {
            if (int rc = three_steps(true, out)) return rc;
        } else {
            if (modes.emit_chain >= 2)
                if (int rc = three_steps(false, ref)) return rc;
            if (int rc = chained(out)) return rc;
        }
        if (modes.emit_chain >= 2) {           // (test aid) every output of the one kernel against the three steps'
            uint32_t *d_bad = reinterpret_cast<uint32_t *>(pool_get<uint64_t>(ctx, S_SMALL, 4096) + 320);
            uint32_t bad[4] = {0, 0, 0, 0};
            MGTA_HIP_CHECK(hipMemsetAsync(d_bad, 0, 16, stream));
            const bool same_totals = out.tot[0] == ref.tot[0] && out.tot[1] == ref.tot[1] && out.tot[2] == ref.tot[2];
            auto grid_of = [&](uint64_t n) { return dim3((unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->num_cus * 16)); };
            if (same_totals) {
                const uint64_t n_tw = out.tot[2] * words_per_tip, n_f = (uint64_t)p.nb() * 3;
                if (out.tot[0]) hipLaunchKernelGGL((emit_equal_kernel<uint16_t>), grid_of(out.tot[0]), dim3(256), 0, stream, out.rec, ref.rec, out.tot[0], d_bad);
                if (out.tot[1]) hipLaunchKernelGGL((emit_equal_kernel<uint16_t>), grid_of(out.tot[1]), dim3(256), 0, stream, out.large, ref.large, out.tot[1], d_bad + 1);
                if (n_tw) hipLaunchKernelGGL((emit_equal_kernel<uint32_t>), grid_of(n_tw), dim3(256), 0, stream, out.tips, ref.tips, n_tw, d_bad + 2);
                hipLaunchKernelGGL((emit_equal_kernel<int64_t>), grid_of(n_f), dim3(256), 0, stream, out.first, ref.first, n_f, d_bad + 3);
            }
            MGTA_HIP_CHECK(hipMemcpyAsync(bad, d_bad, 16, hipMemcpyDeviceToHost, stream));
            MGTA_HIP_CHECK(hipStreamSynchronize(stream));
            if (!same_totals || bad[0] || bad[1] || bad[2] || bad[3]) {
                set_error("internal: one emit kernel gives %llu records, %llu large, %llu tips, the three steps %llu, %llu, %llu; %u records, %u large counts, "
                          "%u tip words and %u bucket entries differ", (unsigned long long)out.tot[0], (unsigned long long)out.tot[1], (unsigned long long)out.tot[2],
                          (unsigned long long)ref.tot[0], (unsigned long long)ref.tot[1], (unsigned long long)ref.tot[2], bad[0], bad[1], bad[2], bad[3]);
                return MGTA_EINTERNAL;
            }
        }
        p.rec = out.rec; p.large = out.large; p.tips = out.tips; p.first = out.first;
        p.n_edges = out.tot[0]; p.n_large = out.tot[1]; p.n_tips = out.tot[2];
        S.ms_emit += t_ph.stop();
        return MGTA_OK;
    }

    // what mgta_sdbg_load_resident / mgta_sdbg_export_records_device find of the build on the context
    void publish_last(uint32_t lo, uint32_t hi, const void *rec, uint64_t n_rec, const void *tips, uint64_t n_tips, const void *first,
                      const void *large, uint64_t n_large) {
        ctx->last_large = large; ctx->last_n_large = n_large;
        ctx->last_rec = rec; ctx->last_n_rec = n_rec; ctx->last_bucket_lo = lo; ctx->last_bucket_hi = hi;
        ctx->last_tips = tips; ctx->last_n_tips = n_tips; ctx->last_first = first; ctx->last_k = k; ctx->last_words_per_tip = words_per_tip;
    }

    // the pass appended to the whole-stream buffers (device to device); capacity from the share of the buckets done so far
    void append_to_stream(const Pass &p) {
        const uint64_t tip_b = words_per_tip * 4;
        auto ensure = [&](DevBuf &buf, uint64_t used, uint64_t add) {
            if (used + add <= buf.bytes) return;
            const double done = (double)(p.b_hi - bucket_begin) / (double)(bucket_end - bucket_begin);
            uint64_t want = (uint64_t)((double)(used + add) / std::max(done, 1e-3) * 1.1) + (1u << 20);
            want = std::max<uint64_t>(want, used + add);
            DevBuf bigger;
            bigger.alloc(want, &ctx->live_bytes, &ctx->peak_bytes);
            if (used) MGTA_HIP_CHECK(hipMemcpyAsync(bigger.p, buf.p, used, hipMemcpyDeviceToDevice, stream));
            MGTA_HIP_CHECK(hipStreamSynchronize(stream));
            buf = std::move(bigger);
        };
        ensure(ctx->acc_rec, ctx->acc_n_rec * 2, p.n_edges * 2);
        ensure(ctx->acc_tips, ctx->acc_n_tips * tip_b, p.n_tips * tip_b);
        if (ctx->acc_has_large) {
            ensure(ctx->acc_large, ctx->acc_n_large * 2, p.n_large * 2);
            if (p.n_large) MGTA_HIP_CHECK(hipMemcpyAsync(ctx->acc_large.as<char>() + ctx->acc_n_large * 2, p.large, p.n_large * 2, hipMemcpyDeviceToDevice, stream));
        }
        if (p.n_edges) MGTA_HIP_CHECK(hipMemcpyAsync(ctx->acc_rec.as<char>() + ctx->acc_n_rec * 2, p.rec, p.n_edges * 2, hipMemcpyDeviceToDevice, stream));
        if (p.n_tips) MGTA_HIP_CHECK(hipMemcpyAsync(ctx->acc_tips.as<char>() + ctx->acc_n_tips * tip_b, p.tips, p.n_tips * tip_b, hipMemcpyDeviceToDevice, stream));
        h_first.resize((size_t)p.nb() * 3);
        MGTA_HIP_CHECK(hipMemcpyAsync(h_first.data(), p.first, (size_t)p.nb() * 3 * 8, hipMemcpyDeviceToHost, stream));
        MGTA_HIP_CHECK(hipStreamSynchronize(stream));
        int64_t nxt = (int64_t)p.n_edges;
        for (int64_t b = (int64_t)p.nb() - 1; b >= 0; --b) {
            int64_t f = h_first[(size_t)b * 3];
            if (f < 0) f = nxt;
            ctx->acc_items[(size_t)p.b_lo + (size_t)b] = nxt - f;
            nxt = f;
        }
        ctx->acc_n_rec += p.n_edges; ctx->acc_n_tips += p.n_tips; ctx->acc_n_large += p.n_large;
    }

    // ---- device -> host and the sink.  keep_stream 2: records and tip labels stay on the device only (the caller takes the whole
    // stream afterwards, mgta_sdbg_stream_detach / mgta_stream_download); the sink still gets the counts and the large multiplicities
    int deliver_pass(const Pass &p) {
        if (!sink) return MGTA_OK;
        const bool to_host = ctx->keep_stream != 2;
        const uint64_t n_tip_words = p.n_tips * words_per_tip;
        h_items.assign((size_t)p.nb() * 3, 0);
        if (p.n_items > 0) {
            t_ph.start();
            h_rec.resize(to_host ? p.n_edges : 0); h_large.resize(p.n_large); h_tips.resize(to_host ? n_tip_words : 0);
            h_first.resize((size_t)p.nb() * 3);
            if (p.n_edges && to_host) MGTA_HIP_CHECK(hipMemcpyAsync(h_rec.data(), p.rec, p.n_edges * 2, hipMemcpyDeviceToHost, stream));
            if (p.n_large) MGTA_HIP_CHECK(hipMemcpyAsync(h_large.data(), p.large, p.n_large * 2, hipMemcpyDeviceToHost, stream));
            if (p.n_tips && to_host) MGTA_HIP_CHECK(hipMemcpyAsync(h_tips.data(), p.tips, n_tip_words * 4, hipMemcpyDeviceToHost, stream));
            MGTA_HIP_CHECK(hipMemcpyAsync(h_first.data(), p.first, (size_t)p.nb() * 3 * 8, hipMemcpyDeviceToHost, stream));
            S.ms_d2h += t_ph.stop();
            // bucket boundaries -> counts; untouched entries (-1) are empty buckets
            int64_t nxt[3] = {(int64_t)p.n_edges, (int64_t)p.n_large, (int64_t)p.n_tips};
            for (int64_t b = (int64_t)p.nb() - 1; b >= 0; --b)
                for (int c = 0; c < 3; ++c) {
                    int64_t f = h_first[(size_t)b * 3 + c];
                    if (f < 0) f = nxt[c];
                    h_items[(size_t)b * 3 + c] = nxt[c] - f;
                    nxt[c] = f;
                }
        } else { h_rec.clear(); h_large.clear(); h_tips.clear(); }
        const int rc = sink(user, (int32_t)p.b_lo, (int32_t)p.b_hi, h_items.data(), to_host ? h_rec.data() : nullptr, (int64_t)p.n_edges,
                            h_large.data(), (int64_t)p.n_large, to_host ? h_tips.data() : nullptr, (int64_t)n_tip_words);
        if (rc != 0) { set_error("edge sink returned %d", rc); return MGTA_ESINK; }
        return MGTA_OK;
    }
};

// f(std::integral_constant<int, W>{}) for the key width W = 1 .. 9 words
template <int W = 1, class F>
static int with_key_words(int words, F &&f) {
    if constexpr (W < 9) {
        if (words == W) return f(std::integral_constant<int, W>{});
        return with_key_words<W + 1>(words, f);
    } else
        return f(std::integral_constant<int, W>{});
}

}  // namespace mgta

using namespace mgta;

extern "C" {

int mgta_reads_upload(mgta_ctx *ctx, const uint32_t *packed, uint64_t n_words, const uint64_t *start_idx, uint64_t n_reads,
                      mgta_reads **out) {
    if (!ctx || !packed || !start_idx || !out) { set_error("mgta_reads_upload: null argument"); return MGTA_EINVAL; }
    return guarded("mgta_reads_upload", [&] {
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        auto r = std::make_unique<mgta_reads>();
        r->ctx = ctx; r->n_words = n_words; r->n_reads = n_reads;
        r->own_packed.alloc((n_words + 16) * 4, &ctx->live_bytes, &ctx->peak_bytes);
        r->own_start.alloc((n_reads + 1) * 8, &ctx->live_bytes, &ctx->peak_bytes);
        MGTA_HIP_CHECK(hipMemsetAsync((char *)r->own_packed.p + n_words * 4, 0, 64, ctx->stream));
        MGTA_HIP_CHECK(hipMemcpyAsync(r->own_packed.p, packed, n_words * 4, hipMemcpyHostToDevice, ctx->stream));
        MGTA_HIP_CHECK(hipMemcpyAsync(r->own_start.p, start_idx, (n_reads + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        MGTA_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        r->d_packed = r->own_packed.as<uint32_t>();
        r->d_start = r->own_start.as<uint64_t>();
        ctx_retain(ctx);
        *out = r.release();
        return MGTA_OK;
    });
}

int mgta_reads_adopt_device(mgta_ctx *ctx, const uint32_t *d_packed, uint64_t n_words, const uint64_t *d_start, uint64_t n_reads,
                            mgta_reads **out) {
    if (!ctx || !d_packed || !d_start || !out) { set_error("mgta_reads_adopt_device: null argument"); return MGTA_EINVAL; }
    return guarded("mgta_reads_adopt_device", [&] {
        auto *r = new mgta_reads;
        r->ctx = ctx; r->d_packed = d_packed; r->d_start = d_start; r->n_words = n_words; r->n_reads = n_reads;
        ctx_retain(ctx);
        *out = r;
        return MGTA_OK;
    });
}

void mgta_reads_free(mgta_reads *r) {
    if (!r) return;
    mgta_ctx *c = r->ctx;
    delete r;
    ctx_release(c);
}

int mgta_sdbg_build_resident(mgta_ctx *ctx, const mgta_reads *rd, uint64_t n_short_reads, int k, int min_count, int need_mercy,
                             int32_t bucket_begin, int32_t bucket_end, mgta_edge_sink sink, void *user, mgta_build_stats *stats) {
    if (!ctx || !rd) { set_error("mgta_sdbg_build: null argument"); return MGTA_EINVAL; }
    if (k < 9 || k > 127) { set_error("k=%d out of range [9,127] (kMaxK, definitions.h:56)", k); return MGTA_EINVAL; }
    if (bucket_begin < 0 || bucket_end > MGTA_NUM_BUCKETS || bucket_begin >= bucket_end) {
        set_error("bucket range [%d,%d) invalid", bucket_begin, bucket_end);
        return MGTA_EINVAL;
    }
    if (min_count < 1) { set_error("min_count must be >= 1"); return MGTA_EINVAL; }
    // (stage 1 always covers every bucket: its verdicts feed every stage-2 bucket; a stage-2 shard is fine)
    return guarded("mgta_sdbg_build", [&] {
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        return with_key_words((2 * k + 4 + 31) / 32, [&](auto w) {   // words_per_substring, s2.cpp:331
            Build<decltype(w)::value> B(ctx);
            B.rd = rd; B.n_short = n_short_reads; B.k = k; B.min_count = min_count; B.need_mercy = need_mercy;
            B.bucket_begin = (uint32_t)bucket_begin; B.bucket_end = (uint32_t)bucket_end; B.sink = sink; B.user = user;
            B.modes = SortModes::from_env();
            const int rc = B.run();
            if (rc == MGTA_OK && stats) *stats = B.S;
            return rc;
        });
    });
}

int mgta_sdbg_last_counting(mgta_ctx *ctx, int64_t *hist) {
    if (!ctx || !hist) { set_error("mgta_sdbg_last_counting: null argument"); return MGTA_EINVAL; }
    if (ctx->edge_counting.size() != 65536) { set_error("no stage-1 run (min_count > 1) on this context yet"); return MGTA_EINVAL; }
    std::copy(ctx->edge_counting.begin(), ctx->edge_counting.end(), hist);
    return MGTA_OK;
}

int mgta_sdbg_last_emit_fused(mgta_ctx *ctx, int64_t *n_passes) {
    if (!ctx || !n_passes) { set_error("mgta_sdbg_last_emit_fused: null argument"); return MGTA_EINVAL; }
    *n_passes = ctx->emit_fused_passes;
    return MGTA_OK;
}

int mgta_sort_plan(uint64_t n_items, int words_per_key, uint32_t bucket_begin, uint32_t bucket_end, int *n_passes, int *skip_bits) {
    if (!n_passes || !skip_bits || words_per_key < 2 || bucket_end > (uint32_t)MGTA_NUM_BUCKETS || bucket_begin >= bucket_end) {
        set_error("mgta_sort_plan: bad argument");
        return MGTA_EINVAL;
    }
    const TopPlan tp = choose_top_plan(nullptr, n_items, std::min(4, (32 * words_per_key - 8) / 8), (double)(bucket_end - bucket_begin) / MGTA_NUM_BUCKETS,
                                       bucket_begin, bucket_end, SortModes::from_env().bias);
    *n_passes = tp.P;
    *skip_bits = tp.skip;
    return MGTA_OK;
}

int mgta_sort_plan_wide(uint64_t n_items, int words_per_key, uint32_t bucket_begin, uint32_t bucket_end, int *n_passes, int *skip_bits, int *widths) {
    if (!n_passes || !skip_bits || !widths || words_per_key < 2 || bucket_end > (uint32_t)MGTA_NUM_BUCKETS || bucket_begin >= bucket_end) {
        set_error("mgta_sort_plan_wide: bad argument");
        return MGTA_EINVAL;
    }
    const SortModes modes = SortModes::from_env();
    const int max_top = std::min(4, (32 * words_per_key - 8) / 8);
    const double frac = (double)(bucket_end - bucket_begin) / MGTA_NUM_BUCKETS;
    TopPlan tp = choose_top_plan(nullptr, n_items, max_top, frac, bucket_begin, bucket_end, modes.bias);
    const bool fits = with_key_words(words_per_key, [&](auto w) { return (int)kWideFits<decltype(w)::value>; }) > 0;
    if (fits) tp = widen_top_plan(tp, n_items, max_top, frac, bucket_begin, bucket_end, modes.bias, modes.wide);
    *n_passes = tp.P;
    *skip_bits = tp.skip;
    for (int i = 0; i < kMaxTop; ++i) widths[i] = i < tp.P ? tp.width[tp.P - 1 - i] : 0;
    return MGTA_OK;
}

int mgta_sdbg_export_records_device(mgta_ctx *ctx, void *d_dst, uint64_t capacity_bytes, uint64_t *n_records) {
    if (!ctx || !n_records) { set_error("mgta_sdbg_export_records_device: null argument"); return MGTA_EINVAL; }
    *n_records = ctx->last_n_rec;
    if (ctx->last_k == 0 || (!ctx->last_rec && ctx->last_n_rec)) { set_error("no device-resident build output"); return MGTA_EINVAL; }
    if (!d_dst) return MGTA_OK;                                    // size query
    if (capacity_bytes < ctx->last_n_rec * 2) { set_error("destination too small"); return MGTA_EINVAL; }
    return guarded("mgta_sdbg_export_records_device", [&] {
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        if (ctx->last_n_rec) MGTA_HIP_CHECK(hipMemcpyAsync(d_dst, ctx->last_rec, ctx->last_n_rec * 2, hipMemcpyDeviceToDevice, ctx->stream));
        MGTA_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return MGTA_OK;
    });
}

int mgta_sdbg_build(mgta_ctx *ctx, const uint32_t *packed, uint64_t n_words, const uint64_t *start_idx, uint64_t n_reads,
                    uint64_t n_short_reads, int k, int min_count, int need_mercy, mgta_edge_sink sink, void *user,
                    mgta_build_stats *stats) {
    mgta_reads *rd = nullptr;
    int rc = mgta_reads_upload(ctx, packed, n_words, start_idx, n_reads, &rd);
    if (rc != MGTA_OK) return rc;
    rc = mgta_sdbg_build_resident(ctx, rd, n_short_reads, k, min_count, need_mercy, 0, MGTA_NUM_BUCKETS, sink, user, stats);
    mgta_reads_free(rd);
    return rc;
}

}  // extern "C"
