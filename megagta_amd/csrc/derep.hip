// derep.hip — the unique, non-contained sequences of a set (mgta_seqs_derep): the first thing the reference's bin/post_proc.sh:50-55
// does with a gene's contigs ("get the unique merged contigs": `Clustering.jar derep`, then `ReadSeq.jar rm-dupseq -d`).
//
// The rule (include/megagta_hip.h) is exact: sequences are byte strings, a DUPLICATE equals an earlier sequence, a CONTAINED first
// occurrence is a substring of a longer sequence, everything else is KEPT.  Hashes only choose what is compared; every equality and
// every containment that decides a status is confirmed letter by letter, so a collision costs comparisons and never an answer
// (mgta_ctx_set_derep_hash_bits cuts both hashes down to a few bits to show that).
//
// Duplicates.  A group of 8 lanes owns a sequence and reads it 16 bytes per lane.  The whole sequence is hashed to 64 bits; an
// open-addressing table holds ONE slot per distinct sequence: a slot is the number of a member of its class, claimed by a 32-bit
// compare-and-swap, and a sequence that meets an occupied slot compares itself with that member -- key and length first, then the
// letters -- and either joins it (atomicMin keeps the lowest number, atomicAdd counts the copies) or probes on.  Equal sequences walk
// the same probe sequence and slots never empty, so a class ends in exactly one slot whatever the timing.
//
// Containment, over the first occurrences only, their letters packed back to back (fewer than 2^32).  With the anchor length
// A = min(16, shortest non-empty first occurrence) every A-letter window is hashed into a second table: a slot holds the key (64-bit
// compare-and-swap), the number of windows with that key and the head of their list; window i links itself with
// next[i] = atomicExch(&head, i).  A query that is a substring of t has EVERY window of its own in t, so it is enough to walk the list
// of one window: the rarest (ties: the leftmost -- the choice is a function of the input).  A count of 1 is the query's own window:
// kept without a comparison.  The order of a list depends on timing; the answer is "any entry matches", which does not.  Queries are
// handed out longest list first from one atomic head.  Worst case: sequences made of one repeated window (low complexity) put
// (letters of the set) entries into one list, and each of them walks it: quadratic, as the problem is for such input.
#include <algorithm>
#include <vector>

#include "seq_dp.hpp"

namespace mgta {
namespace {

constexpr int kDerepThreads = 256;        // 4 waves = 32 groups of 8 lanes
constexpr int kDerepGroups = kDerepThreads / 8;
constexpr uint32_t kNil = 0xFFFFFFFFu;
constexpr uint64_t kEmptyKey = ~0ull;
constexpr int kMaxAnchor = 16;            // one 16-byte load holds a window

__device__ __forceinline__ uint64_t mix64(uint64_t x) {                   // the finaliser of splitmix64
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// 16 bytes from any address (the buffers end in 16 spare bytes); the bytes from `n` on read as zero
__device__ __forceinline__ void load16(const uint8_t *p, uint32_t n, uint64_t &lo, uint64_t &hi) {
    uint4 v;
    __builtin_memcpy(&v, p, 16);
    lo = (uint64_t)v.x | ((uint64_t)v.y << 32);
    hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
    if (n < 16) {
        if (n <= 8) { hi = 0; lo = n == 8 ? lo : (lo & ((1ull << (8 * n)) - 1)); }
        else hi &= (1ull << (8 * (n - 8))) - 1;
    }
}

// the 8 lanes of a group run the same control flow, so they are active together wherever one of them is
__device__ __forceinline__ bool grp_any(bool x) { return ((__ballot(x) >> (lane_id() & ~7)) & 0xFFull) != 0; }
__device__ __forceinline__ uint64_t grp_sum64(uint64_t v) {
    v += __shfl_xor(v, 1, 8); v += __shfl_xor(v, 2, 8); v += __shfl_xor(v, 4, 8);
    return v;
}
__device__ __forceinline__ uint64_t grp_min64(uint64_t v) {
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) { const uint64_t o = __shfl_xor(v, d, 8); v = o < v ? o : v; }
    return v;
}

// a[0, len) == b[0, len), 16 bytes per lane and step
__device__ __forceinline__ bool grp_equal(const uint8_t *a, const uint8_t *b, uint32_t len, int sub) {
    for (uint32_t base = 0; base < len; base += 128) {
        const uint32_t p = base + (uint32_t)sub * 16;
        bool diff = false;
        if (p < len) {
            const uint32_t nv = min(16u, len - p);
            uint64_t al, ah, bl, bh;
            load16(a + p, nv, al, ah);
            load16(b + p, nv, bl, bh);
            diff = ((al ^ bl) | (ah ^ bh)) != 0;
        }
        if (grp_any(diff)) return false;
    }
    return true;
}

__device__ __forceinline__ uint64_t cut_key(uint64_t h, uint64_t mask) {
    h &= mask;
    return h == kEmptyKey ? 0 : h;                                        // (two keys become one: a collision like any other)
}

// ---- duplicates --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDerepThreads) void derep_hash_kernel(const uint8_t *s, const uint64_t *off, uint32_t n, uint64_t mask, uint64_t *hkey) {
    const int sub = threadIdx.x & 7;
    const uint32_t stride = gridDim.x * kDerepGroups;
    for (uint32_t i = blockIdx.x * kDerepGroups + (threadIdx.x >> 3); i < n; i += stride) {
        const uint8_t *a = s + off[i];
        const uint32_t len = (uint32_t)(off[i + 1] - off[i]);
        uint64_t acc = 0;
        for (uint32_t p = (uint32_t)sub * 16; p < len; p += 128) {
            uint64_t lo, hi;
            load16(a + p, min(16u, len - p), lo, hi);
            const uint64_t c = (uint64_t)(p >> 4) * 2 + 1;
            acc += mix64(lo ^ (c * 0x9E3779B97F4A7C15ull)) + mix64(hi ^ ((c + 1) * 0xC2B2AE3D27D4EB4Full));
        }
        acc = mix64(grp_sum64(acc) ^ ((uint64_t)len * 0xD6E8FEB86659FD93ull));
        if (sub == 0) hkey[i] = cut_key(acc, mask);
    }
}

// counters: [1] letter comparisons
__global__ __launch_bounds__(kDerepThreads) void derep_class_kernel(const uint8_t *s, const uint64_t *off, uint32_t n, const uint64_t *hkey, uint32_t *tab, uint32_t *cnt,
                                                                    uint64_t n_slots, uint32_t *slot_of, unsigned long long *counters) {
    const int sub = threadIdx.x & 7;
    const uint32_t stride = gridDim.x * kDerepGroups;
    uint32_t compares = 0;
    for (uint32_t i = blockIdx.x * kDerepGroups + (threadIdx.x >> 3); i < n; i += stride) {
        const uint8_t *a = s + off[i];
        const uint32_t len = (uint32_t)(off[i + 1] - off[i]);
        const uint64_t key = hkey[i];
        uint64_t slot = mix64(key) & (n_slots - 1);
        for (;;) {
            uint32_t r = __hip_atomic_load(&tab[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r = __shfl(r, 0, 8);
            if (r == kNil) {
                uint32_t prev = 0;
                if (sub == 0) prev = atomicCAS(&tab[slot], kNil, i);
                prev = __shfl(prev, 0, 8);
                if (prev == kNil) break;                                  // the class is new and this is its slot
                r = prev;
            }
            // r is a member of the slot's class (any member has the class's letters)
            if (hkey[r] == key && (uint32_t)(off[r + 1] - off[r]) == len) {
                ++compares;
                if (grp_equal(a, s + off[r], len, sub)) {
                    if (sub == 0) atomicMin(&tab[slot], i);
                    break;
                }
            }
            slot = (slot + 1) & (n_slots - 1);
        }
        if (sub == 0) {
            slot_of[i] = (uint32_t)slot;
            atomicAdd(&cnt[slot], 1u);
        }
    }
    const uint32_t c = wave_sum(sub == 0 ? compares : 0u);
    if (lane_id() == 0 && c) atomicAdd(&counters[1], (unsigned long long)c);
}

__global__ __launch_bounds__(256) void derep_resolve_kernel(uint32_t n, const uint32_t *tab, const uint32_t *cnt, const uint32_t *slot_of, uint32_t *rep, uint32_t *copies) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = slot_of[i], r = tab[slot];
    rep[i] = r;
    copies[i] = r == i ? cnt[slot] : 0u;
}

// ---- the window table over the first occurrences -----------------------------------------------------------------------------------
// first occurrence f = input orig[f]; its letters go to fl[foff[f], foff[f + 1]) and every one of them learns its owner
__global__ __launch_bounds__(kDerepThreads) void derep_pack_kernel(const uint8_t *s, const uint64_t *off, const uint32_t *orig, const uint32_t *foff, uint32_t n_first,
                                                                   uint8_t *fl, uint32_t *owner) {
    const int sub = threadIdx.x & 7;
    const uint32_t stride = gridDim.x * kDerepGroups;
    for (uint32_t f = blockIdx.x * kDerepGroups + (threadIdx.x >> 3); f < n_first; f += stride) {
        const uint8_t *a = s + off[orig[f]];
        const uint32_t b = foff[f], len = foff[f + 1] - b;
        for (uint32_t p = (uint32_t)sub * 16; p < len; p += 128) {
            const uint32_t nv = min(16u, len - p);
            if (nv == 16) {
                uint4 v;
                __builtin_memcpy(&v, a + p, 16);
                __builtin_memcpy(fl + b + p, &v, 16);
            } else
                for (uint32_t j = 0; j < nv; ++j) fl[b + p + j] = a[p + j];
            for (uint32_t j = 0; j < nv; ++j) owner[b + p + j] = f;
        }
    }
}

__device__ __forceinline__ uint64_t window_key(const uint8_t *p, uint32_t anchor, uint64_t mask) {
    uint64_t lo, hi;
    load16(p, anchor, lo, hi);
    return cut_key(mix64(lo ^ 0x9E3779B97F4A7C15ull) + mix64(hi ^ 0xC2B2AE3D27D4EB4Full), mask);
}

// one thread per letter: the window that starts there, when it fits its sequence
__global__ __launch_bounds__(256) void derep_windows_kernel(const uint8_t *fl, const uint32_t *owner, const uint32_t *foff, uint64_t n_letters, uint32_t anchor, uint64_t mask,
                                                            unsigned long long *keys, uint32_t *counts, uint32_t *heads, uint64_t n_slots, uint32_t *next) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_letters; i += stride) {
        const uint32_t f = owner[i];
        if (i + anchor > (uint64_t)foff[f + 1]) continue;
        const uint64_t key = window_key(fl + i, anchor, mask);
        uint64_t slot = mix64(key) & (n_slots - 1);
        for (;;) {
            unsigned long long k = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k == kEmptyKey) k = atomicCAS(&keys[slot], (unsigned long long)kEmptyKey, (unsigned long long)key);
            if (k == kEmptyKey || k == key) break;
            slot = (slot + 1) & (n_slots - 1);
        }
        atomicAdd(&counts[slot], 1u);
        next[i] = atomicExch(&heads[slot], (uint32_t)i);
    }
}

// the table is final: the slot of a key that is in it
__device__ __forceinline__ uint64_t window_slot(const unsigned long long *keys, uint64_t n_slots, uint64_t key) {
    uint64_t slot = mix64(key) & (n_slots - 1);
    while (keys[slot] != key) slot = (slot + 1) & (n_slots - 1);
    return slot;
}

// per non-empty first occurrence: its rarest window (ties: the leftmost) -> position, count and list head
__global__ __launch_bounds__(kDerepThreads) void derep_anchor_kernel(const uint8_t *fl, const uint32_t *foff, uint32_t n_first, uint32_t anchor, uint64_t mask,
                                                                     const unsigned long long *keys, const uint32_t *counts, const uint32_t *heads, uint64_t n_slots,
                                                                     uint32_t *a_pos, uint32_t *a_cnt, uint32_t *a_head) {
    const int sub = threadIdx.x & 7;
    const uint32_t stride = gridDim.x * kDerepGroups;
    for (uint32_t f = blockIdx.x * kDerepGroups + (threadIdx.x >> 3); f < n_first; f += stride) {
        const uint32_t b = foff[f], len = foff[f + 1] - b;
        if (len < anchor) {                                               // (the empty sequence: the host decides)
            if (sub == 0) { a_pos[f] = 0; a_cnt[f] = 0; a_head[f] = kNil; }
            continue;
        }
        const uint32_t n_win = len - anchor + 1;
        uint64_t best = ~0ull;
        for (uint32_t p = (uint32_t)sub; p < n_win; p += 8) {
            const uint64_t slot = window_slot(keys, n_slots, window_key(fl + b + p, anchor, mask));
            const uint64_t v = ((uint64_t)counts[slot] << 32) | p;
            best = v < best ? v : best;
        }
        best = grp_min64(best);
        if (sub == 0) {
            const uint32_t p = (uint32_t)best;
            a_pos[f] = p;
            a_cnt[f] = (uint32_t)(best >> 32);
            a_head[f] = heads[window_slot(keys, n_slots, window_key(fl + b + p, anchor, mask))];
        }
    }
}

// counters: [0] queue head, [1] letter comparisons
__global__ __launch_bounds__(kDerepThreads) void derep_verify_kernel(const uint8_t *fl, const uint32_t *owner, const uint32_t *foff, const uint32_t *next,
                                                                     const uint32_t *jobs, uint32_t n_jobs, const uint32_t *a_pos, const uint32_t *a_head,
                                                                     uint8_t *contained, unsigned long long *counters) {
    const int sub = threadIdx.x & 7;
    uint32_t compares = 0;
    for (;;) {
        unsigned long long j = 0;
        if (sub == 0) j = atomicAdd(&counters[0], 1ull);
        j = __shfl(j, 0, 8);
        if (j >= n_jobs) break;
        const uint32_t q = jobs[j];
        const uint32_t qb = foff[q], qlen = foff[q + 1] - qb, pa = a_pos[q];
        bool found = false;
        for (uint32_t w = a_head[q]; w != kNil && !found; w = next[w]) {
            const uint32_t t = owner[w];
            const uint32_t tb = foff[t], tlen = foff[t + 1] - tb, pt = w - tb;
            // the query laid over t with the two windows on each other: it has to fit on both sides, and t has to be longer
            if (tlen <= qlen || pt < pa || (uint64_t)(pt - pa) + qlen > tlen) continue;
            ++compares;
            found = grp_equal(fl + qb, fl + tb + (pt - pa), qlen, sub);
        }
        if (sub == 0) contained[q] = found ? 1 : 0;
    }
    const uint32_t c = wave_sum(sub == 0 ? compares : 0u);
    if (lane_id() == 0 && c) atomicAdd(&counters[1], (unsigned long long)c);
}

uint64_t pow2_at_least(uint64_t x) {
    uint64_t p = 64;
    while (p < x) p <<= 1;
    return p;
}

unsigned group_blocks(const mgta_ctx *ctx, uint64_t n_groups) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_groups + kDerepGroups - 1) / kDerepGroups, (uint64_t)ctx->num_cus * 8));
}

}  // namespace
}  // namespace mgta

using namespace mgta;

extern "C" {

int mgta_ctx_set_derep_hash_bits(mgta_ctx *ctx, int bits) {
    if (!ctx) { set_error("mgta_ctx_set_derep_hash_bits: ctx must not be NULL"); return MGTA_EINVAL; }
    if (bits < 1 || bits > 64) { set_error("mgta_ctx_set_derep_hash_bits: bits = %d (1 .. 64)", bits); return MGTA_EINVAL; }
    ctx->derep_hash_bits = bits;
    return MGTA_OK;
}

int mgta_seqs_derep(mgta_ctx *ctx, const char *seqs, const uint64_t *offsets, int64_t n, uint8_t *status, int64_t *rep, uint32_t *copies, mgta_derep_stats *stats) {
    if (!ctx) { set_error("mgta_seqs_derep: ctx must not be NULL"); return MGTA_EINVAL; }
    if (n < 0) { set_error("mgta_seqs_derep: n = %lld must not be negative", (long long)n); return MGTA_EINVAL; }
    if (!check_seq_count("mgta_seqs_derep", kSequences, n)) return MGTA_EINVAL;
    if (n > 0 && !offsets) { set_error("mgta_seqs_derep: offsets must not be NULL"); return MGTA_EINVAL; }
    if (n > 0 && (!status || !rep || !copies)) { set_error("mgta_seqs_derep: status, rep and copies must not be NULL"); return MGTA_EINVAL; }
    if (!check_seq_offsets("mgta_seqs_derep", kSequences, offsets, n, 0xFFFFFFFFull, "letters", "< 2^32 letters in the first occurrences")) return MGTA_EINVAL;
    if (!check_seq_letters("mgta_seqs_derep", kSequences, seqs, n > 0 ? offsets[n] - offsets[0] : 0)) return MGTA_EINVAL;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return MGTA_OK;
    return guarded("mgta_seqs_derep", [&]() {
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        uint64_t *live = &ctx->live_bytes, *peak = &ctx->peak_bytes;
        const uint32_t nn = (uint32_t)n;
        const uint64_t n_letters = offsets[n] - offsets[0];
        const uint64_t mask = ctx->derep_hash_bits >= 64 ? ~0ull : (1ull << ctx->derep_hash_bits) - 1;
        Timer t_dups(st), t_table(st), t_verify(st);
        DevBuf d_cnt;                                                     // [0] queue head, [1] letter comparisons
        d_cnt.alloc(64, live, peak);
        MGTA_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 64, st));

        // ---- duplicates: one table slot per distinct sequence
        DevBuf d_all, d_off, d_rep, d_cop;
        d_all.alloc(n_letters + 32, live, peak);
        d_off.alloc((size_t)(nn + 1) * 8, live, peak);
        d_rep.alloc((size_t)nn * 4, live, peak);
        d_cop.alloc((size_t)nn * 4, live, peak);
        const std::vector<uint64_t> rel = rel_offsets(offsets, n);
        if (n_letters) MGTA_HIP_CHECK(hipMemcpyAsync(d_all.p, seqs + offsets[0], n_letters, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemsetAsync(d_all.as<uint8_t>() + n_letters, 0, 32, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_off.p, rel.data(), (size_t)(nn + 1) * 8, hipMemcpyHostToDevice, st));
        std::vector<uint32_t> h_rep(nn), h_cop(nn);
        {
            DevBuf d_hkey, d_tab, d_tcnt, d_slot;
            const uint64_t n_slots = pow2_at_least(2ull * nn);
            d_hkey.alloc((size_t)nn * 8, live, peak);
            d_tab.alloc(n_slots * 4, live, peak);
            d_tcnt.alloc(n_slots * 4, live, peak);
            d_slot.alloc((size_t)nn * 4, live, peak);
            MGTA_HIP_CHECK(hipMemsetAsync(d_tab.p, 0xFF, n_slots * 4, st));
            MGTA_HIP_CHECK(hipMemsetAsync(d_tcnt.p, 0, n_slots * 4, st));
            const unsigned blocks = group_blocks(ctx, nn);
            t_dups.start();
            hipLaunchKernelGGL(derep_hash_kernel, dim3(blocks), dim3(kDerepThreads), 0, st, d_all.as<uint8_t>(), d_off.as<uint64_t>(), nn, mask, d_hkey.as<uint64_t>());
            hipLaunchKernelGGL(derep_class_kernel, dim3(blocks), dim3(kDerepThreads), 0, st, d_all.as<uint8_t>(), d_off.as<uint64_t>(), nn, d_hkey.as<uint64_t>(),
                               d_tab.as<uint32_t>(), d_tcnt.as<uint32_t>(), n_slots, d_slot.as<uint32_t>(), d_cnt.as<unsigned long long>());
            hipLaunchKernelGGL(derep_resolve_kernel, dim3((nn + 255) / 256), dim3(256), 0, st, nn, d_tab.as<uint32_t>(), d_tcnt.as<uint32_t>(), d_slot.as<uint32_t>(),
                               d_rep.as<uint32_t>(), d_cop.as<uint32_t>());
            MGTA_HIP_CHECK(hipGetLastError());
            t_dups.end();
            MGTA_HIP_CHECK(hipMemcpyAsync(h_rep.data(), d_rep.p, (size_t)nn * 4, hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipMemcpyAsync(h_cop.data(), d_cop.p, (size_t)nn * 4, hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
        }
        d_rep.release(); d_cop.release();

        // ---- the first occurrences, packed: their numbers, where their letters start, the anchor length
        std::vector<uint32_t> orig, foff(1, 0);
        uint64_t n_fl = 0, n_windows = 0;
        uint32_t shortest = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < nn; ++i) {
            if (h_rep[i] != i) continue;
            const uint64_t len = rel[i + 1] - rel[i];
            n_fl += len;
            if (n_fl >= (1ull << 32)) {
                set_error("mgta_seqs_derep: the first occurrences hold %llu letters or more (the limit is < 2^32 letters in the first occurrences)", (unsigned long long)n_fl);
                return (int)MGTA_EINVAL;
            }
            orig.push_back(i);
            foff.push_back((uint32_t)n_fl);
            if (len) shortest = std::min(shortest, (uint32_t)len);
        }
        const uint32_t n_first = (uint32_t)orig.size();
        const uint32_t anchor = n_fl ? std::min<uint32_t>(kMaxAnchor, shortest) : 0;
        std::vector<uint8_t> h_contained(n_first, 0);
        double ms_table = 0, ms_verify = 0;
        if (n_fl && n_first > 1) {
            for (uint32_t f = 0; f < n_first; ++f) {
                const uint32_t len = foff[f + 1] - foff[f];
                if (len) n_windows += len - anchor + 1;
            }
            DevBuf d_orig, d_foff, d_fl, d_owner, d_next, d_keys, d_counts, d_heads, d_apos, d_acnt, d_ahead, d_jobs, d_cont;
            d_orig.alloc((size_t)n_first * 4, live, peak);
            d_foff.alloc((size_t)(n_first + 1) * 4, live, peak);
            d_fl.alloc(n_fl + 32, live, peak);
            d_owner.alloc(n_fl * 4, live, peak);
            MGTA_HIP_CHECK(hipMemcpyAsync(d_orig.p, orig.data(), (size_t)n_first * 4, hipMemcpyHostToDevice, st));
            MGTA_HIP_CHECK(hipMemcpyAsync(d_foff.p, foff.data(), (size_t)(n_first + 1) * 4, hipMemcpyHostToDevice, st));
            MGTA_HIP_CHECK(hipMemsetAsync(d_fl.as<uint8_t>() + n_fl, 0, 32, st));
            const unsigned blocks = group_blocks(ctx, n_first);
            t_table.start();
            hipLaunchKernelGGL(derep_pack_kernel, dim3(blocks), dim3(kDerepThreads), 0, st, d_all.as<uint8_t>(), d_off.as<uint64_t>(), d_orig.as<uint32_t>(),
                               d_foff.as<uint32_t>(), n_first, d_fl.as<uint8_t>(), d_owner.as<uint32_t>());
            MGTA_HIP_CHECK(hipGetLastError());
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
            d_all.release(); d_off.release(); d_orig.release();           // the input's letters are no longer needed: room for the table
            const uint64_t n_slots = pow2_at_least(2 * n_windows);
            d_next.alloc(n_fl * 4, live, peak);
            d_keys.alloc(n_slots * 8, live, peak);
            d_counts.alloc(n_slots * 4, live, peak);
            d_heads.alloc(n_slots * 4, live, peak);
            MGTA_HIP_CHECK(hipMemsetAsync(d_keys.p, 0xFF, n_slots * 8, st));
            MGTA_HIP_CHECK(hipMemsetAsync(d_counts.p, 0, n_slots * 4, st));
            MGTA_HIP_CHECK(hipMemsetAsync(d_heads.p, 0xFF, n_slots * 4, st));
            hipLaunchKernelGGL(derep_windows_kernel, dim3((unsigned)std::min<uint64_t>((n_fl + 255) / 256, (uint64_t)ctx->num_cus * 32)), dim3(256), 0, st,
                               d_fl.as<uint8_t>(), d_owner.as<uint32_t>(), d_foff.as<uint32_t>(), n_fl, anchor, mask, d_keys.as<unsigned long long>(), d_counts.as<uint32_t>(),
                               d_heads.as<uint32_t>(), n_slots, d_next.as<uint32_t>());
            MGTA_HIP_CHECK(hipGetLastError());
            t_table.end();

            // ---- the rarest window of every query, then the walk of its list, longest list first
            d_apos.alloc((size_t)n_first * 4, live, peak);
            d_acnt.alloc((size_t)n_first * 4, live, peak);
            d_ahead.alloc((size_t)n_first * 4, live, peak);
            d_cont.alloc(n_first, live, peak);
            MGTA_HIP_CHECK(hipMemsetAsync(d_cont.p, 0, n_first, st));
            t_verify.start();
            hipLaunchKernelGGL(derep_anchor_kernel, dim3(blocks), dim3(kDerepThreads), 0, st, d_fl.as<uint8_t>(), d_foff.as<uint32_t>(), n_first, anchor, mask,
                               d_keys.as<unsigned long long>(), d_counts.as<uint32_t>(), d_heads.as<uint32_t>(), n_slots, d_apos.as<uint32_t>(), d_acnt.as<uint32_t>(),
                               d_ahead.as<uint32_t>());
            MGTA_HIP_CHECK(hipGetLastError());
            std::vector<uint32_t> a_cnt(n_first), jobs;
            MGTA_HIP_CHECK(hipMemcpyAsync(a_cnt.data(), d_acnt.p, (size_t)n_first * 4, hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
            for (uint32_t f = 0; f < n_first; ++f)
                if (a_cnt[f] > 1) jobs.push_back(f);                      // a count of 1 is the query's own window: kept
            std::stable_sort(jobs.begin(), jobs.end(), [&](uint32_t x, uint32_t y) { return a_cnt[x] > a_cnt[y]; });
            const uint32_t nj = (uint32_t)jobs.size();
            if (nj) {
                // workgroups of the walk a CU holds at once: what its registers allow (never assumed)
                int blocks_per_cu = 0;
                MGTA_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, derep_verify_kernel, kDerepThreads, 0));
                blocks_per_cu = std::max(1, blocks_per_cu);
                d_jobs.alloc((size_t)nj * 4, live, peak);
                MGTA_HIP_CHECK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)nj * 4, hipMemcpyHostToDevice, st));
                const unsigned vb = (unsigned)std::min<uint64_t>((uint64_t)ctx->num_cus * (uint64_t)blocks_per_cu, ((uint64_t)nj + kDerepGroups - 1) / kDerepGroups);
                hipLaunchKernelGGL(derep_verify_kernel, dim3(vb), dim3(kDerepThreads), 0, st, d_fl.as<uint8_t>(), d_owner.as<uint32_t>(), d_foff.as<uint32_t>(),
                                   d_next.as<uint32_t>(), d_jobs.as<uint32_t>(), nj, d_apos.as<uint32_t>(), d_ahead.as<uint32_t>(), d_cont.as<uint8_t>(),
                                   d_cnt.as<unsigned long long>());
                MGTA_HIP_CHECK(hipGetLastError());
            }
            t_verify.end();
            MGTA_HIP_CHECK(hipMemcpyAsync(h_contained.data(), d_cont.p, n_first, hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
            ms_table = t_table.ms();
            ms_verify = t_verify.ms();
            // the empty sequence is a substring of every other one
            for (uint32_t f = 0; f < n_first; ++f)
                if (foff[f + 1] == foff[f]) h_contained[f] = 1;
        }
        unsigned long long cnt[2] = {0, 0};
        MGTA_HIP_CHECK(hipMemcpyAsync(cnt, d_cnt.p, 16, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));

        int64_t n_contained = 0;
        for (uint32_t i = 0, f = 0; i < nn; ++i) {
            if (h_rep[i] != i) { status[i] = 1; rep[i] = (int64_t)h_rep[i]; copies[i] = 0; continue; }
            const bool c = h_contained[f++] != 0;
            n_contained += c;
            status[i] = c ? 2 : 0;
            rep[i] = c ? -1 : (int64_t)i;
            copies[i] = h_cop[i];
        }
        if (stats) {
            stats->n_seqs = n; stats->n_letters = (int64_t)n_letters; stats->n_first = n_first; stats->n_duplicates = n - (int64_t)n_first;
            stats->n_contained = n_contained; stats->n_kept = (int64_t)n_first - n_contained; stats->n_windows = (int64_t)n_windows;
            stats->anchor_len = anchor; stats->n_compares = (int64_t)cnt[1];
            stats->ms_dups = t_dups.ms(); stats->ms_table = ms_table; stats->ms_verify = ms_verify;
        }
        return (int)MGTA_OK;
    });
}

}  // extern "C"
