// phase.hip — which alleles of a contig's variant positions travel together on one fragment: per site the fragments per allele, per
// tabled pair of sites the 4 x 4 table of the fragments that show an allele at both (mgta_reads_phase; the rule is this project's own
// and is stated in include/megagta_hip.h).  No graph: the inputs are the packed reads, their placements (mgta_reads_pileup's per_read)
// and the sites.
//
// One kernel.  A group of 8 lanes owns a fragment slot (32 groups per workgroup, slots from one atomic head): a pair of mates in a
// paired library, one read anywhere else.  The slot's library comes from a binary search in the library table (a copy in LDS), the
// sites a usable read covers from two binary searches in its contig's positions.  Nothing is staged: the allele of a fragment at a site
// is recomputed from the one or two placement records wherever it is needed, one packed-word load per read that covers the site.  Pass
// one shares the sites of the fragment among the lanes and adds the alleles; pass two, for a fragment with at least two alleles, goes
// through the sites one by one and shares each site's partners inside max_span among the lanes.  The sites between two mates that
// neither covers are walked and give nothing.  All adds are integer atomicAdds, so no order matters; every loop is bounded by a site
// count, a library count or the chunk; no workgroup waits for another.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "device_utils.hpp"
#include "walk.hpp"

namespace mgta {
namespace {

constexpr uint32_t kPhaseMaxRead = 65535;
constexpr int kPhaseMaxLibs = 256;
constexpr int32_t kPhaseSpan = 1000;

enum { HC_HEAD, HC_USABLE, HC_FRAG, HC_MATE, HC_FRAG_ALLELE, HC_FRAG_LINKED, HC_ALLELES, HC_CONFLICTS, HC_PAIR_ADDS, HC_NUM };

struct PhaseLib {                     // library s takes the slots [slot0, slot0 of s + 1): entry n_libs closes the table
    uint64_t slot0, first, end;       // its reads [first, end)
    uint64_t paired;
};

struct PhaseArgs {
    const uint32_t *packed;
    const uint64_t *start;
    int reversed;
    uint32_t chunk;
    const mgta_read_place *place;
    const PhaseLib *libs;             // [n_libs + 1]
    int n_libs;
    uint64_t n_slots;
    const uint64_t *coff;             // [n + 1]
    const uint64_t *site_off;         // [n + 1]
    const uint32_t *site_pos;         // [S]
    const uint64_t *pair_off;         // [S + 1]
    uint32_t *site_counts;            // [S][4]
    uint32_t *joint;                  // [n_pairs][16]
    unsigned long long *counters;
};

struct PhaseRead {                    // a usable read: what its letters at the sites [lo, hi) of the call need
    uint64_t s0;
    uint32_t len, comp, contig;
    int same, orient;
    int64_t d;
    uint32_t lo, hi;                  // lo == hi: it covers no site
    bool ok;
};

// the first site of [a, b) at or behind position x (b when there is none)
__device__ __forceinline__ uint32_t phase_lower(const uint32_t *pos, uint32_t a, uint32_t b, int64_t x) {
    while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if ((int64_t)pos[m] < x) a = m + 1; else b = m;
    }
    return a;
}

__device__ __forceinline__ PhaseRead phase_read(const PhaseArgs &A, uint64_t r) {
    PhaseRead R{};
    const mgta_read_place pr = A.place[r];
    R.ok = pr.n_placed == 1;
    if (!R.ok) return R;
    R.s0 = A.start[r];
    R.len = (uint32_t)(A.start[r + 1] - R.s0);
    R.contig = (uint32_t)pr.contig;
    R.orient = pr.orient ? 1 : 0;
    R.same = R.orient == (A.reversed ? 1 : 0);                                // the stored order, complemented when reversed, is orientation `reversed`
    R.comp = R.orient ? 3u : 0u;
    R.d = pr.diag;
    const int64_t clen = (int64_t)(A.coff[R.contig + 1] - A.coff[R.contig]);
    const int64_t x0 = R.d > 0 ? R.d : 0, x1 = R.d + (int64_t)R.len < clen ? R.d + (int64_t)R.len : clen;
    const uint32_t sa = (uint32_t)A.site_off[R.contig], sb = (uint32_t)A.site_off[R.contig + 1];
    if (x1 > x0) {
        R.lo = phase_lower(A.site_pos, sa, sb, x0);
        R.hi = phase_lower(A.site_pos, R.lo, sb, x1);
    }
    return R;
}

// the fragment's allele 0..3 at site u, -1 where it has none; conflict is set where both reads cover u and differ
__device__ __forceinline__ int phase_allele(const PhaseArgs &A, const PhaseRead &R0, const PhaseRead &R1, bool two, uint32_t u, bool &conflict) {
    const bool in0 = u >= R0.lo && u < R0.hi, in1 = two && u >= R1.lo && u < R1.hi;
    conflict = false;
    if (!in0 && !in1) return -1;
    const int64_t x = (int64_t)A.site_pos[u];
    int b0 = -1, b1 = -1;
    if (in0) b0 = (int)pile_base(A.packed, R0.s0, R0.len, R0.same, R0.comp, (uint32_t)(x - R0.d)) - 1;
    if (in1) b1 = (int)pile_base(A.packed, R1.s0, R1.len, R1.same, R1.comp, (uint32_t)(x - R1.d)) - 1;
    if (in0 && in1 && b0 != b1) { conflict = true; return -1; }
    return in0 ? b0 : b1;
}

// One fragment.  All 8 lanes of the group run the same control flow on the same bounds.
__device__ __forceinline__ void phase_fragment(const PhaseArgs &A, const PhaseRead &R0, const PhaseRead &R1, bool two, int sub, uint32_t &n_frag_allele,
                                               uint32_t &n_frag_linked, uint32_t &n_alleles, uint32_t &n_conflicts, unsigned long long &n_adds) {
    uint32_t lo = R0.lo, hi = R0.hi;
    if (two && R1.lo < R1.hi) {
        if (lo < hi) { lo = min(lo, R1.lo); hi = max(hi, R1.hi); }
        else { lo = R1.lo; hi = R1.hi; }
    }
    if (lo >= hi) return;
    uint32_t mine = 0;
    for (uint32_t ub = lo; ub < hi; ub += 8) {                                // the lanes share the sites
        const uint32_t u = ub + (uint32_t)sub;
        if (u < hi) {
            bool conflict;
            const int a = phase_allele(A, R0, R1, two, u, conflict);
            if (a >= 0) { atomicAdd(&A.site_counts[(uint64_t)u * 4 + (uint32_t)a], 1u); ++mine; }
            if (conflict) ++n_conflicts;
        }
        if (hi - ub <= 8) break;                                              // (ub + 8 may wrap at the last sites of a call of 2^32 - 1)
    }
    n_alleles += mine;
    uint32_t all = mine;                                                      // the fragment's alleles, in every lane of the group
    all += __shfl_xor(all, 1, 8);
    all += __shfl_xor(all, 2, 8);
    all += __shfl_xor(all, 4, 8);
    if (sub == 0 && all >= 1) ++n_frag_allele;
    if (sub == 0 && all >= 2) ++n_frag_linked;
    if (all < 2) return;
    for (uint32_t u = lo; u + 1 < hi; ++u) {                                  // site by site; the lanes share its partners
        bool conflict;
        const int au = phase_allele(A, R0, R1, two, u, conflict);
        if (au < 0) continue;
        const uint64_t p0 = A.pair_off[u], n_part = A.pair_off[u + 1] - p0;   // the partners are the sites u + 1 .. u + n_part
        const uint64_t v_end = min((uint64_t)hi, (uint64_t)u + 1 + n_part);
        for (uint64_t v = (uint64_t)u + 1 + (uint64_t)sub; v < v_end; v += 8) {
            const int av = phase_allele(A, R0, R1, two, (uint32_t)v, conflict);
            if (av >= 0) { atomicAdd(&A.joint[(p0 + (v - u - 1)) * 16 + (uint32_t)(au * 4 + av)], 1u); ++n_adds; }
        }
    }
}

__global__ __launch_bounds__(kCovThreads) void phase_scan_kernel(PhaseArgs A) {
    __shared__ PhaseLib s_lib[kPhaseMaxLibs + 1];
    __shared__ unsigned long long s_cnt[HC_NUM];
    if (threadIdx.x < HC_NUM) s_cnt[threadIdx.x] = 0;
    for (int s = threadIdx.x; s <= A.n_libs; s += kCovThreads) s_lib[s] = A.libs[s];
    __syncthreads();
    const int sub = threadIdx.x & 7;
    uint32_t n_usable = 0, n_frag = 0, n_mate = 0, n_frag_allele = 0, n_frag_linked = 0, n_alleles = 0, n_conflicts = 0;
    unsigned long long n_adds = 0;
    for (;;) {
        const unsigned long long first = grp_next_chunk(&A.counters[HC_HEAD], A.chunk, sub);
        if (first >= A.n_slots) break;
        const uint64_t slot_end = min((unsigned long long)A.n_slots, first + A.chunk);
        for (uint64_t slot = first; slot < slot_end; ++slot) {
            int a = 0, b = A.n_libs;                                          // the last library whose slot0 is at or in front of the slot
            while (b - a > 1) {
                const int m = (a + b) >> 1;
                if (s_lib[m].slot0 <= slot) a = m; else b = m;
            }
            const PhaseLib lib = s_lib[a];
            const uint64_t r0 = lib.first + (lib.paired ? 2 * (slot - lib.slot0) : slot - lib.slot0);
            const bool has1 = lib.paired && r0 + 1 < lib.end;
            const PhaseRead R0 = phase_read(A, r0);
            PhaseRead R1{};
            if (has1) R1 = phase_read(A, r0 + 1);
            if (sub == 0) n_usable += (R0.ok ? 1u : 0u) + (R1.ok ? 1u : 0u);
            if (R0.ok && R1.ok && R0.contig == R1.contig && R0.orient != R1.orient) {
                if (sub == 0) { ++n_frag; ++n_mate; }
                phase_fragment(A, R0, R1, true, sub, n_frag_allele, n_frag_linked, n_alleles, n_conflicts, n_adds);
            } else {
                if (R0.ok) {
                    if (sub == 0) ++n_frag;
                    phase_fragment(A, R0, R0, false, sub, n_frag_allele, n_frag_linked, n_alleles, n_conflicts, n_adds);
                }
                if (R1.ok) {
                    if (sub == 0) ++n_frag;
                    phase_fragment(A, R1, R1, false, sub, n_frag_allele, n_frag_linked, n_alleles, n_conflicts, n_adds);
                }
            }
        }
    }
    if (n_usable) atomicAdd(&s_cnt[HC_USABLE], (unsigned long long)n_usable);
    if (n_frag) atomicAdd(&s_cnt[HC_FRAG], (unsigned long long)n_frag);
    if (n_mate) atomicAdd(&s_cnt[HC_MATE], (unsigned long long)n_mate);
    if (n_frag_allele) atomicAdd(&s_cnt[HC_FRAG_ALLELE], (unsigned long long)n_frag_allele);
    if (n_frag_linked) atomicAdd(&s_cnt[HC_FRAG_LINKED], (unsigned long long)n_frag_linked);
    if (n_alleles) atomicAdd(&s_cnt[HC_ALLELES], (unsigned long long)n_alleles);
    if (n_conflicts) atomicAdd(&s_cnt[HC_CONFLICTS], (unsigned long long)n_conflicts);
    if (n_adds) atomicAdd(&s_cnt[HC_PAIR_ADDS], n_adds);
    __syncthreads();
    if (threadIdx.x > 0 && threadIdx.x < HC_NUM && s_cnt[threadIdx.x]) atomicAdd(&A.counters[threadIdx.x], s_cnt[threadIdx.x]);
}

// the site lists of n contigs -> pair_off[S + 1]; false with the error set when a list is not in order
bool phase_pair_offsets(const char *who, const uint64_t *site_off, const uint32_t *site_pos, int64_t n, int32_t max_span, std::vector<uint64_t> &pair_off) {
    if (n < 0 || !site_off) { set_error("%s: bad contig count or site_off", who); return false; }
    if (n > 0x7FFFFFFFll) { set_error("%s: %lld contigs (n < 2^31 is supported)", who, (long long)n); return false; }
    if (max_span < 0) { set_error("%s: max_span = %d (must not be negative)", who, max_span); return false; }
    if (site_off[0] != 0) { set_error("%s: site_off[0] = %llu (0 is expected)", who, (unsigned long long)site_off[0]); return false; }
    for (int64_t i = 0; i < n; ++i)
        if (site_off[i + 1] < site_off[i]) { set_error("%s: contig %lld: site_off must ascend", who, (long long)i); return false; }
    const uint64_t S = site_off[n];
    if (S >= 0xFFFFFFFFull) { set_error("%s: %llu sites in the call (S < 2^32 - 1 is supported)", who, (unsigned long long)S); return false; }
    if (S && !site_pos) { set_error("%s: site_pos must not be NULL", who); return false; }
    const uint64_t span = max_span ? (uint64_t)max_span : (uint64_t)kPhaseSpan;
    pair_off.assign((size_t)S + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t a = site_off[i], b = site_off[i + 1];
        uint64_t v = a;                                                       // the first site behind u that is too far from it
        for (uint64_t u = a; u < b; ++u) {
            if (u > a && site_pos[u] <= site_pos[u - 1]) {
                set_error("%s: contig %lld: its sites must ascend (site %llu at %u follows %u)", who, (long long)i, (unsigned long long)(u - a), site_pos[u], site_pos[u - 1]);
                return false;
            }
            if (v <= u) v = u + 1;
            while (v < b && site_pos[v] > site_pos[v - 1] && (uint64_t)site_pos[v] - site_pos[u] < span) ++v;
            pair_off[(size_t)u + 1] = v - u - 1;
        }
    }
    for (uint64_t u = 0; u < S; ++u) pair_off[(size_t)u + 1] += pair_off[(size_t)u];
    return true;
}

}  // namespace
}  // namespace mgta

using namespace mgta;

extern "C" {

int mgta_ctx_set_phase_chunk(mgta_ctx *ctx, uint32_t slots) {
    if (!ctx) { set_error("mgta_ctx_set_phase_chunk: ctx must not be NULL"); return MGTA_EINVAL; }
    ctx->phase_chunk = slots;
    return MGTA_OK;
}

int mgta_phase_pairs(const uint64_t *site_off, const uint32_t *site_pos, int64_t n, int32_t max_span, uint64_t *pair_off) {
    if (!pair_off) { set_error("mgta_phase_pairs: pair_off must not be NULL"); return MGTA_EINVAL; }
    return guarded("mgta_phase_pairs", [&]() {
        std::vector<uint64_t> po;
        if (!phase_pair_offsets("mgta_phase_pairs", site_off, site_pos, n, max_span, po)) return (int)MGTA_EINVAL;
        std::copy(po.begin(), po.end(), pair_off);
        return (int)MGTA_OK;
    });
}

int mgta_reads_phase(const mgta_reads *reads, int reads_reversed, const mgta_read_place *place, const uint64_t *lib_end, const uint8_t *lib_paired, int n_libs,
                     const uint64_t *offsets, int64_t n, const uint64_t *site_off, const uint32_t *site_pos, const mgta_phase_params *params, uint32_t *site_counts,
                     uint64_t *pair_off, uint32_t *joint, uint64_t joint_cap, mgta_phase_stats *stats) {
    const char *who = "mgta_reads_phase";
    if (!reads) { set_error("%s: the reads must not be NULL", who); return MGTA_EINVAL; }
    if (!lib_end || !lib_paired) { set_error("%s: lib_end and lib_paired must not be NULL", who); return MGTA_EINVAL; }
    if (n_libs < 1 || n_libs > kPhaseMaxLibs) { set_error("%s: n_libs = %d (1 .. %d are supported)", who, n_libs, kPhaseMaxLibs); return MGTA_EINVAL; }
    for (int s = 1; s < n_libs; ++s)
        if (lib_end[s] < lib_end[s - 1]) { set_error("%s: lib_end[%d] = %llu is below lib_end[%d] = %llu", who, s, (unsigned long long)lib_end[s], s - 1, (unsigned long long)lib_end[s - 1]); return MGTA_EINVAL; }
    const uint64_t n_reads = lib_end[n_libs - 1];
    if (n_reads > reads->n_reads) {
        set_error("%s: lib_end[%d] = %llu, the library holds %llu reads", who, n_libs - 1, (unsigned long long)n_reads, (unsigned long long)reads->n_reads);
        return MGTA_EINVAL;
    }
    if (n < 0 || !offsets || !site_off) { set_error("%s: bad contig count, offsets or site_off", who); return MGTA_EINVAL; }
    if (!pair_off) { set_error("%s: pair_off must not be NULL", who); return MGTA_EINVAL; }
    if (n_reads && !place) { set_error("%s: place must not be NULL", who); return MGTA_EINVAL; }
    mgta_phase_params par{0};
    if (params) par = *params;
    return guarded(who, [&]() {
        std::vector<uint64_t> po;
        if (!phase_pair_offsets(who, site_off, site_pos, n, par.max_span, po)) return (int)MGTA_EINVAL;
        const uint64_t S = site_off[n], n_pairs = po[(size_t)S];
        for (int64_t i = 0; i < n; ++i) {
            if (offsets[i + 1] < offsets[i]) { set_error("%s: contig %lld: offsets must ascend", who, (long long)i); return (int)MGTA_EINVAL; }
            const uint64_t len = offsets[i + 1] - offsets[i];
            if (site_off[i + 1] > site_off[i] && (uint64_t)site_pos[site_off[i + 1] - 1] >= len) {
                set_error("%s: contig %lld: site at %u, the contig has %llu letters (a site lies below the contig's length)", who, (long long)i, site_pos[site_off[i + 1] - 1],
                          (unsigned long long)len);
                return (int)MGTA_EINVAL;
            }
        }
        for (uint64_t r = 0; r < n_reads; ++r)
            if (place[r].n_placed == 1 && (place[r].contig < 0 || (int64_t)place[r].contig >= n)) {
                set_error("%s: place[%llu].contig = %d, the call has %lld contigs (contig < n)", who, (unsigned long long)r, place[r].contig, (long long)n);
                return (int)MGTA_EINVAL;
            }
        if (S && !site_counts) { set_error("%s: site_counts must not be NULL", who); return (int)MGTA_EINVAL; }
        if (joint_cap < n_pairs) {
            set_error("%s: joint_cap = %llu, the sites give %llu tabled pairs (joint_cap >= %llu is needed)", who, (unsigned long long)joint_cap, (unsigned long long)n_pairs,
                      (unsigned long long)n_pairs);
            return (int)MGTA_EINVAL;
        }
        if (n_pairs && !joint) { set_error("%s: joint must not be NULL", who); return (int)MGTA_EINVAL; }
        auto zero_outputs = [&]() {
            if (stats) memset(stats, 0, sizeof(*stats));
            if (S) memset(site_counts, 0, S * 16);
            if (n_pairs) memset(joint, 0, n_pairs * 64);
            std::copy(po.begin(), po.end(), pair_off);
        };
        if (n == 0 || S == 0) { zero_outputs(); return (int)MGTA_OK; }
        mgta_ctx *ctx = reads->ctx;
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        uint64_t live = 0, peak = 0;                                          // the buffers of this call
        DevBuf d_cnt;
        d_cnt.alloc(256, &live, &peak);
        MGTA_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 256, st));
        unsigned long long *cnt_scan = d_cnt.as<unsigned long long>(), *cnt_len = cnt_scan + 24;
        unsigned long long max_len = 0;
        if (n_reads) {
            hipLaunchKernelGGL(pile_maxlen_kernel, dim3((unsigned)std::min<uint64_t>((n_reads + 255) / 256, (uint64_t)ctx->num_cus * 8)), dim3(256), 0, st, reads->d_start, n_reads,
                               cnt_len);
            MGTA_HIP_CHECK(hipGetLastError());
            MGTA_HIP_CHECK(hipMemcpyAsync(&max_len, cnt_len, 8, hipMemcpyDeviceToHost, st));
            MGTA_HIP_CHECK(hipStreamSynchronize(st));
        }
        if (max_len > kPhaseMaxRead) {
            set_error("%s: a read of %llu bases (reads of at most %u bases are supported)", who, max_len, kPhaseMaxRead);
            return (int)MGTA_EINVAL;
        }
        // the library table: a slot is a pair of mates in a paired library (the odd last read has a slot of its own), a read elsewhere
        std::vector<PhaseLib> libs((size_t)n_libs + 1);
        uint64_t n_slots = 0;
        for (int s = 0; s < n_libs; ++s) {
            const uint64_t first = s ? lib_end[s - 1] : 0, cnt = lib_end[s] - first;
            libs[(size_t)s] = PhaseLib{n_slots, first, lib_end[s], lib_paired[s] ? 1ull : 0ull};
            n_slots += lib_paired[s] ? (cnt + 1) / 2 : cnt;
        }
        libs[(size_t)n_libs] = PhaseLib{n_slots, n_reads, n_reads, 0};
        DevBuf d_place, d_libs, d_coff, d_soff, d_spos, d_poff, d_counts, d_joint;
        d_place.alloc((size_t)n_reads * sizeof(mgta_read_place), &live, &peak);
        d_libs.alloc(libs.size() * sizeof(PhaseLib), &live, &peak);
        d_coff.alloc(((size_t)n + 1) * 8, &live, &peak);
        d_soff.alloc(((size_t)n + 1) * 8, &live, &peak);
        d_spos.alloc((size_t)S * 4, &live, &peak);
        d_poff.alloc(((size_t)S + 1) * 8, &live, &peak);
        d_counts.alloc((size_t)S * 16, &live, &peak);
        d_joint.alloc((size_t)n_pairs * 64, &live, &peak);
        Timer t_up(st), t_scan(st);
        t_up.start();
        if (n_reads) MGTA_HIP_CHECK(hipMemcpyAsync(d_place.p, place, (size_t)n_reads * sizeof(mgta_read_place), hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_libs.p, libs.data(), libs.size() * sizeof(PhaseLib), hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_coff.p, offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_soff.p, site_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_spos.p, site_pos, (size_t)S * 4, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(d_poff.p, po.data(), ((size_t)S + 1) * 8, hipMemcpyHostToDevice, st));
        MGTA_HIP_CHECK(hipMemsetAsync(d_counts.p, 0, (size_t)S * 16, st));
        if (n_pairs) MGTA_HIP_CHECK(hipMemsetAsync(d_joint.p, 0, (size_t)n_pairs * 64, st));
        t_up.end();
        const QueueLaunch q = queue_launch(ctx, queue_per_cu(phase_scan_kernel), n_slots, 256, 16, ctx->phase_chunk);
        t_scan.start();
        if (n_slots) {
            PhaseArgs A;
            A.packed = reads->d_packed; A.start = reads->d_start; A.reversed = reads_reversed ? 1 : 0; A.chunk = q.chunk; A.place = d_place.as<mgta_read_place>();
            A.libs = d_libs.as<PhaseLib>(); A.n_libs = n_libs; A.n_slots = n_slots; A.coff = d_coff.as<uint64_t>(); A.site_off = d_soff.as<uint64_t>();
            A.site_pos = d_spos.as<uint32_t>(); A.pair_off = d_poff.as<uint64_t>(); A.site_counts = d_counts.as<uint32_t>(); A.joint = d_joint.as<uint32_t>();
            A.counters = cnt_scan;
            hipLaunchKernelGGL(phase_scan_kernel, dim3(q.blocks), dim3(kCovThreads), 0, st, A);
        }
        MGTA_HIP_CHECK(hipGetLastError());
        t_scan.end();
        // into buffers of the call first: an error up to here has written nothing
        std::vector<uint32_t> h_counts((size_t)S * 4), h_joint((size_t)n_pairs * 16);
        unsigned long long cnt[HC_NUM] = {0};
        MGTA_HIP_CHECK(hipMemcpyAsync(h_counts.data(), d_counts.p, (size_t)S * 16, hipMemcpyDeviceToHost, st));
        if (n_pairs) MGTA_HIP_CHECK(hipMemcpyAsync(h_joint.data(), d_joint.p, (size_t)n_pairs * 64, hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipMemcpyAsync(cnt, d_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
        MGTA_HIP_CHECK(hipStreamSynchronize(st));
        if (ctx->live_bytes + peak > ctx->peak_bytes) ctx->peak_bytes = ctx->live_bytes + peak;
        const double ms_up = t_up.ms(), ms_scan = t_scan.ms();
        std::copy(h_counts.begin(), h_counts.end(), site_counts);
        std::copy(h_joint.begin(), h_joint.end(), joint);
        std::copy(po.begin(), po.end(), pair_off);
        if (stats) {
            stats->n_reads = (int64_t)n_reads; stats->n_usable = (int64_t)cnt[HC_USABLE]; stats->n_fragments = (int64_t)cnt[HC_FRAG];
            stats->n_mate_fragments = (int64_t)cnt[HC_MATE]; stats->n_fragments_allele = (int64_t)cnt[HC_FRAG_ALLELE];
            stats->n_fragments_linked = (int64_t)cnt[HC_FRAG_LINKED]; stats->n_alleles = (int64_t)cnt[HC_ALLELES]; stats->n_conflicts = (int64_t)cnt[HC_CONFLICTS];
            stats->n_pair_adds = (int64_t)cnt[HC_PAIR_ADDS]; stats->n_sites = (int64_t)S; stats->n_pairs = (int64_t)n_pairs; stats->peak_bytes = peak;
            stats->ms_upload = ms_up; stats->ms_scan = ms_scan; stats->ms_total = ms_up + ms_scan;
        }
        return (int)MGTA_OK;
    });
}

}  // extern "C"
