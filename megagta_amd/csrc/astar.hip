// astar.hip — batched HMM-guided A* over the device-resident succinct de Bruijn graph (gfx950): host side + C ABI.
//
// Replaces the OMP seed loop of search() (search.cpp:184-189) and, per seed and direction,
// HMMGraphSearch::astarSearch (hmm_graph_search.h:132-343) with NodeEnumerator::enumerateNodes
// (node_enumerator.h:65-246), AStarNode ordering (a_star_node.h:34-82) and the result walk
// getHighestScoreNode / partialResultFromGoal (hmm_graph_search.h:83-110,345-356).
// The kernel and its data structures are in astar_kernel.hpp.  Scores are IEEE fp64, compiled with -ffp-contract=off:
// path log-probabilities are bit-identical to the x86-64 reference, fval = (int)(10000*(score+2h)) truncates identically.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <string>
#include <thread>

#include "astar_kernel.hpp"
#include "scan.hpp"

using namespace mgta;

static const char kCodonAA[65] = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF";   // codon.h:9-106

namespace {
// the result strings of a batch, packed: side sid's `len[sid]` characters move from its fixed-size slot to packed[off[sid] ...) (a
// million-seed batch has 5 GB of slots for 0.7 GB of text: the slots never cross the bus)
__global__ __launch_bounds__(256) void pack_results_kernel(const char *slots, uint32_t slot_bytes, const uint32_t *len, const uint64_t *off, uint64_t n_sides,
                                                           char *packed) {
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    const int lane = threadIdx.x & 63;
    for (uint64_t sid = wave; sid < n_sides; sid += n_waves) {
        const uint32_t n = len[sid];
        const char *src = slots + sid * slot_bytes;
        char *dst = packed + off[sid];
        for (uint32_t i = (uint32_t)lane; i < n; i += 64) dst[i] = src[i];
    }
}
struct Events {                  // RAII: the events also go on the early-return and throw paths
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    Events() { for (auto &x : e) MGTA_HIP_CHECK(hipEventCreate(&x)); }
    ~Events() { for (auto &x : e) if (x) (void)hipEventDestroy(x); }
};

template <int G>
void launch_astar(const mgta::AstarArgs &a, int blocks, size_t lds_bytes, bool use_lds, hipStream_t st) {
    using namespace mgta;
    if (use_lds) {
        MGTA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(astar_kernel<G, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        hipLaunchKernelGGL((astar_kernel<G, true>), dim3(blocks), dim3(kAstarThreads), lds_bytes, st, a);
    } else {
        MGTA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(astar_kernel<G, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        hipLaunchKernelGGL((astar_kernel<G, false>), dim3(blocks), dim3(kAstarThreads), lds_bytes, st, a);
    }
    MGTA_HIP_CHECK(hipGetLastError());
}
template <int G> size_t lds_fixed() {
    return (size_t)mgta::kAstarWaves * mgta::Grp<G>::kGroups * (mgta::Grp<G>::kLdsHeap * sizeof(mgta::HeapEnt) + mgta::kPtWords * sizeof(uint32_t) + mgta::kStage * sizeof(mgta::HeapEnt));
}
}  // namespace

extern "C" {

int mgta_hmm_load(mgta_ctx *ctx, int M, int A, const double *msc, const double *tsc, const double *max_match, const double *h,
                  const int32_t *alpha, mgta_hmm **out) {
    if (!ctx || !msc || !tsc || !max_match || !h || !alpha || !out || M < 1 || M > 30000 || A < 1 || A > 64) {
        set_error("mgta_hmm_load: bad argument");
        return MGTA_EINVAL;
    }
    return guarded("mgta_hmm_load", [&]() -> int {
        MGTA_HIP_CHECK(hipSetDevice(ctx->device));
        auto hm = std::make_unique<mgta_hmm>();
        hm->ctx = ctx; hm->M = M; hm->A = A;
        size_t M1 = (size_t)M + 1;
        hm->n_doubles = M1 * (A + 11);
        std::vector<double> host(hm->n_doubles);
        std::copy(msc, msc + M1 * A, host.begin());
        for (size_t j = 0; j < (size_t)A; ++j) host[j] = -INFINITY;                // msc(0, .) = -inf (profile_hmm.h:58-64)
        std::copy(tsc, tsc + 7 * M1, host.begin() + M1 * A);
        std::copy(max_match, max_match + M1, host.begin() + M1 * (A + 7));
        std::copy(h, h + 3 * M1, host.begin() + M1 * (A + 8));
        hm->tab.alloc(hm->n_doubles * 8, &ctx->live_bytes, &ctx->peak_bytes);
        MGTA_HIP_CHECK(hipMemcpy(hm->tab.p, host.data(), hm->n_doubles * 8, hipMemcpyHostToDevice));
        for (int c = 0; c < 64; ++c) {
            int c1 = c >> 4, c2 = (c >> 2) & 3, c3 = c & 3;
            char f = kCodonAA[c], r = kCodonAA[(3 - c3) * 16 + (3 - c2) * 4 + (3 - c1)];   // rc_codonTable, codon.h:108-209
            hm->col[0][c] = (int8_t)(f == '*' ? -1 : alpha[(int)f]);
            hm->col[1][c] = (int8_t)(r == '*' ? -1 : alpha[(int)r]);
            if ((f != '*' && alpha[(int)f] < 0) || (r != '*' && alpha[(int)r] < 0)) {
                set_error("mgta_hmm_load: amino acid without a column in the model alphabet");
                return MGTA_EINVAL;
            }
        }
        hm->d_col.alloc(128, &ctx->live_bytes, &ctx->peak_bytes);
        MGTA_HIP_CHECK(hipMemcpy(hm->d_col.p, hm->col, 128, hipMemcpyHostToDevice));
        for (int c = 0; c < 128; ++c) hm->alpha[c] = (int8_t)(c < 127 && alpha[c] >= 0 && alpha[c] < A ? alpha[c] : -1);
        hm->d_alpha.alloc(128, &ctx->live_bytes, &ctx->peak_bytes);
        MGTA_HIP_CHECK(hipMemcpy(hm->d_alpha.p, hm->alpha, 128, hipMemcpyHostToDevice));
        ctx_retain(ctx);
        *out = hm.release();
        return MGTA_OK;
    });
}

void mgta_hmm_free(mgta_hmm *h) {
    if (!h) return;
    mgta_ctx *c = h->ctx;
    delete h;
    ctx_release(c);
}


int mgta_ctx_set_search_arena(mgta_ctx *ctx, int log2_base_nodes, uint64_t pool_bytes) {
    if (!ctx || (log2_base_nodes != 0 && (log2_base_nodes < 7 || log2_base_nodes > 20))) { set_error("mgta_ctx_set_search_arena: bad argument"); return MGTA_EINVAL; }
    ctx->astar_log_b0 = log2_base_nodes;
    ctx->astar_pool_bytes = pool_bytes;
    return MGTA_OK;
}

int mgta_ctx_set_search_page_limit(mgta_ctx *ctx, int pages) {
    if (!ctx || pages < 0 || pages > kMaxPages) { set_error("mgta_ctx_set_search_page_limit: 0 <= pages <= %d", kMaxPages); return MGTA_EINVAL; }
    ctx->search_page_limit = pages;
    return MGTA_OK;
}

int mgta_ctx_set_search_share(mgta_ctx *ctx, int num, int den) {
    if (!ctx || num < 1 || den < num) { set_error("mgta_ctx_set_search_share: 1 <= num <= den"); return MGTA_EINVAL; }
    ctx->search_share_num = num; ctx->search_share_den = den;
    return MGTA_OK;
}

int mgta_astar_batch(mgta_sdbg *g, const mgta_hmm *fwd, const mgta_hmm *rev, const char *kmers, const int32_t *start_state, int64_t n,
                     int prune_len, double low_cov_penalty, int cache_mode, mgta_contig_sink sink, void *user, mgta_astar_stats *stats) {
    return mgta_astar_batch_on(g ? g->ctx : nullptr, g, fwd, rev, kmers, start_state, n, prune_len, low_cov_penalty, cache_mode, sink, user, stats);
}

}  // extern "C"

namespace {
struct PackedOut {               // mgta_astar_batch_packed: the contigs written straight into one malloc'd buffer
    char **contigs;
    uint64_t *offsets;           // [n + 1]
    mgta_astar_side *sides;      // [2 n] or null
};
// One call of mgta_astar_batch: its inputs, what is chosen for it once, its device buffers and the searches still to run.
// astar_batch_impl hands it to the stages below in the order they are defined.
struct Batch {
    mgta_ctx *ctx; mgta_sdbg *g; hipStream_t st; const mgta_hmm *hm[2];
    const char *kmers; const int32_t *start_state; int64_t n; int klen;
    int cache_mode;              // 0 = cold, B >= 1 = shared caches with window B
    bool free_share, gated;      // shared caches without any ordering (cache_mode -1 of the API); seeds start in order behind the commit frontier
    int G = 16; int64_t spb = 0;                 // lanes per search, search slots per workgroup
    bool use_lds = false; size_t lds_bytes = 0;  // the HMM tables sit in LDS
    uint64_t slot_bytes = 0;     // base arena of a search slot
    AstarArgs a;
    DevBuf d_kmers, d_ss, d_sn, d_exit, d_queue, d_sides, d_out, d_len, d_status, d_prof, d_tmark, d_todo[2];
    DevBuf d_cache[2], d_start_limit, d_run_seed, d_run_progress;
    std::vector<int64_t> todo[2];           // seeds to run per direction
    std::vector<int32_t> h_status;          // [2n] SearchStatus, as of the last pass
    std::vector<char> over_limit_seen;      // [2n] kSearchOverLimit reported (once, however many passes the batch takes)
};
// start edges: the k-mer (right search) and its reverse complement (left search), hmm_graph_search.h:163-186
int encode_start_edges(mgta_sdbg *g, const char *kmers, int64_t n, int klen, std::vector<int64_t> &start_node) {
    std::vector<uint8_t> seqs((size_t)n * 2 * klen);
    for (int64_t s = 0; s < n; ++s) {
        const char *km = kmers + s * klen;
        for (int i = 0; i < klen; ++i) {
            char c = km[i];
            int b = (c == 'A' || c == 'a') ? 1 : (c == 'C' || c == 'c') ? 2 : (c == 'G' || c == 'g' || c == 'N' || c == 'n') ? 3
                    : (c == 'T' || c == 't') ? 4 : 0;                           // dna_map, hmm_graph_search.h:54-58
            seqs[(size_t)(2 * s) * klen + i] = (uint8_t)b;
            seqs[(size_t)(2 * s + 1) * klen + (klen - 1 - i)] = (uint8_t)(b ? 5 - b : 0);
        }
    }
    start_node.resize((size_t)n * 2);
    return mgta_sdbg_index_edges(g, seqs.data(), n * 2, start_node.data());
}
// lanes per search: 16 (four searches per wavefront, 8192 in flight) beat 64 at every size measured with the small windows + cost term
// `megagta search` uses (profiles/r02/e2e_window_sweep.log).  Eight (16 384 in flight, two walk passes) pay where the batch is large and
// independent (cold, 120 000 seeds on the 100 M-read graph: 46.6 -> 43.6 s) and lose where single searches bound the run (profiles/r03/astar_ab.md),
// except in ordered batches of 65 536 seeds and more on graphs of up to 2 G edges (profiles/r05/trials_*_lanes*.log).  MGTA_ASTAR_GROUP overrides.
int lanes_per_search(const Batch &b) {
    int G = (b.cache_mode == 0 && b.n >= 32768) ? 8 : 16;
    if (b.gated && b.n >= 65536 && b.g->dev.size <= (2ll << 30)) G = 8;
    if (const char *e = getenv("MGTA_ASTAR_GROUP")) { int v = atoi(e); if (v == 8 || v == 16 || v == 32 || v == 64) G = v; }
    return G;
}
// the batch's device buffers, its inputs on the device, and the launch arguments every pass shares
void upload_batch(Batch &b, const std::vector<int64_t> &start_node, int prune_len, double low_cov_penalty, mgta_astar_stats &ST) {
    const int64_t n = b.n; const hipStream_t st = b.st;
    const double lcp = -std::log(low_cov_penalty);                              // node_enumerator.h:42
    std::vector<double> exit_prob(3000);
    for (int i = 0; i < 3000; ++i) exit_prob[i] = std::log(2.0 / (i + 2)) * 2;  // hmm_graph_search.h:48-52
    const uint32_t out_cap = (uint32_t)(3 * (2 * std::max(b.hm[0]->M, b.hm[1]->M) + 64));
    b.d_kmers.alloc((size_t)n * b.klen); b.d_ss.alloc(n * 4); b.d_sn.alloc(n * 16); b.d_exit.alloc(3000 * 8); b.d_queue.alloc(16);
    b.d_sides.alloc((size_t)n * 2 * sizeof(mgta_astar_side)); b.d_out.alloc((size_t)n * 2 * out_cap); b.d_len.alloc(n * 8);
    b.d_status.alloc(n * 8);
    MGTA_HIP_CHECK(hipMemcpyAsync(b.d_kmers.p, b.kmers, (size_t)n * b.klen, hipMemcpyHostToDevice, st));
    MGTA_HIP_CHECK(hipMemcpyAsync(b.d_ss.p, b.start_state, n * 4, hipMemcpyHostToDevice, st));
    MGTA_HIP_CHECK(hipMemcpyAsync(b.d_sn.p, start_node.data(), n * 16, hipMemcpyHostToDevice, st));
    MGTA_HIP_CHECK(hipMemcpyAsync(b.d_exit.p, exit_prob.data(), 3000 * 8, hipMemcpyHostToDevice, st));
    MGTA_HIP_CHECK(hipMemsetAsync(b.d_status.p, 0, n * 8, st));
    AstarArgs &a = b.a;
    memset(&a, 0, sizeof(a));
    a.g = b.g->dev;
    size_t tab_bytes = 0;
    for (int d = 0; d < 2; ++d) {
        a.hm[d].tab = b.hm[d]->tab.as<double>(); a.hm[d].M = b.hm[d]->M; a.hm[d].A = b.hm[d]->A;
        a.hm[d].col_fwd = b.hm[d]->d_col.as<int8_t>(); a.hm[d].col_enum = b.hm[d]->d_col.as<int8_t>() + 64 * d;
        tab_bytes = std::max(tab_bytes, b.hm[d]->n_doubles * 8);
    }
    a.kmers = b.d_kmers.as<char>(); a.start_state = b.d_ss.as<int32_t>(); a.start_node = b.d_sn.as<int64_t>();
    a.n_seeds = n; a.klen = b.klen; a.prune = prune_len; a.low_cov_penalty = lcp; a.log2v = std::log(2.0);
    a.exit_prob = b.d_exit.as<double>(); a.queue = b.d_queue.as<unsigned long long>();
    a.sides = b.d_sides.as<mgta_astar_side>(); a.out_seq = b.d_out.as<char>(); a.out_cap = out_cap; a.out_len = b.d_len.as<uint32_t>();
    a.status = b.d_status.as<int32_t>();
    b.d_prof.alloc(128);
    MGTA_HIP_CHECK(hipMemsetAsync(b.d_prof.p, 0, 128, st));
    b.d_tmark.alloc(32);
    a.prof = b.d_prof.as<unsigned long long>(); a.tmark = b.d_tmark.as<unsigned long long>();
    const size_t lds_fix = b.G == 8 ? lds_fixed<8>() : b.G == 16 ? lds_fixed<16>() : b.G == 32 ? lds_fixed<32>() : lds_fixed<64>();
    b.use_lds = lds_fix + tab_bytes + 1024 <= 160 * 1024;                      // heap tops + level tables + HMM tables
    b.lds_bytes = lds_fix + (b.use_lds ? tab_bytes : 0);
    ST.hmm_in_lds = b.use_lds ? 1 : 0;
    const mgta_ctx *ctx = b.ctx;
    a.window = b.cache_mode; a.cache_probe_limit = 256;
    a.cost_rate = b.gated ? ctx->search_cost_rate : 0;
    a.cost_knee = a.cost_rate > 0 ? ctx->search_cost_knee : 0;
    a.cost_rate2 = a.cost_knee ? ctx->search_cost_rate2 : 0;
    // base arena of a slot: 8192 nodes (1 MB with its heap slots and hash table); beyond it a search takes 2 MB pages, three at least.  The bytes
    // searches hold bound how many run: with 4096 nodes the 5-50 k-node bulk of a 2 M-read run held 6 MB each for 1.5 used (21.0 s, not 17.1)
    a.base_off = 0; a.log_b0 = ctx->astar_log_b0 ? ctx->astar_log_b0 : 13;
    b.slot_bytes = 128ull << a.log_b0;                                         // per node of the base arena: 64 B + 2 heap slots + 2 hash entries of 16 B
    a.slot_bytes = b.slot_bytes; a.gate = b.gated; a.free_share = b.free_share;
    a.page_limit = (uint32_t)(ctx->search_page_limit ? ctx->search_page_limit : kMaxPages);
    // The order is HELD by default, whatever it costs (advisor r4: giving it up silently made the contigs of large inputs depend on timing and
    // on the rank count).  MEGAGTA_SEARCH_ALLOW_UNORDERED=1 opts into the last resort: a batch whose searches in flight have outgrown the
    // pool (thousands of refused requests) goes on WITHOUT the order, says so on stderr and in mgta_astar_stats.order_abandoned.
    a.auto_unorder = b.gated && getenv("MEGAGTA_SEARCH_ALLOW_UNORDERED") && atoi(getenv("MEGAGTA_SEARCH_ALLOW_UNORDERED")) ? 1 : 0;
}
// Independent searches (cold) may be taken in any order, and a batch cannot end before its longest search does (one expansion of one
// search is a chain of dependent line fetches: tens of microseconds, whatever else the device is doing).  The searches that promise the
// most work -- the most model columns still to cover on their side -- are therefore started FIRST (longest processing time first), so that the
// long ones run beside the bulk instead of after it.  Results are per seed and do not depend on the order.  MGTA_ASTAR_LPT=0 keeps the seed
// order.  (Shared-cache batches: the order IS the semantics, never touched.)
void longest_first(Batch &b) {
    if (b.cache_mode != 0) return;
    const char *e = getenv("MGTA_ASTAR_LPT");
    if (e && atoi(e) == 0) return;
    const int32_t *start_state = b.start_state; const int klen = b.klen;
    for (int d = 0; d < 2; ++d) {
        const int Md = b.hm[d]->M;
        std::stable_sort(b.todo[d].begin(), b.todo[d].end(), [&](int64_t x, int64_t y) {
            const int cx = d == 0 ? Md - start_state[x] - klen / 3 : start_state[x], cy = d == 0 ? Md - start_state[y] - klen / 3 : start_state[y];
            return cx > cy;
        });
    }
}
// shared term_nodes caches: one open-addressing table per direction, sized for the entries the searches can insert (one per
// node of a result path: about the model length per search), never more than a quarter of the free memory each; an insert
// that finds the neighbourhood of its slot full is dropped and counted (a missed cache entry costs expansions, never correctness).
// Beside them the launch's control words (CtlWord); `free_b` is counted again after.
void alloc_caches(Batch &b, size_t &free_b) {
    mgta_ctx *ctx = b.ctx; AstarArgs &a = b.a;
    for (int d = 0; d < 2; ++d) {
        // (one entry per DISTINCT node of the result paths: up to 1 GB the table holds "every seed a path of its own" twice over; beyond,
        // the paths of one gene copy's seeds share theirs and an eighth is generous -- 2 x 36 GB of tables took a fifth of the device at 50 M reads)
        uint64_t want = 2ull * (uint64_t)b.n * ((uint64_t)b.hm[d]->M + 64), cap = 1024;
        const uint64_t gb = (1ull << 30) / sizeof(CacheEnt);                     // tables below 1 GB keep the worst-case size
        if (want > gb) want = std::max(gb, want / 8);
        while (cap < want) cap <<= 1;
        while (cap > 1024 && cap * sizeof(CacheEnt) > free_b / 8) cap >>= 1;
        b.d_cache[d].alloc(cap * sizeof(CacheEnt), &ctx->live_bytes, &ctx->peak_bytes);
        MGTA_HIP_CHECK(hipMemsetAsync(b.d_cache[d].p, 0, cap * sizeof(CacheEnt), b.st));
        a.cache[d] = b.d_cache[d].as<CacheEnt>(); a.cache_mask[d] = cap - 1;
    }
    b.d_start_limit.alloc(kCtlWords * sizeof(unsigned long long));
    a.start_limit = b.d_start_limit.as<unsigned long long>(); a.pool.rbump = a.start_limit + kCtlReserve;
    size_t total_b = 0; MGTA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
}
// what one pass launches with
struct PassPlan {
    int64_t blocks, blocks_dir0;
    uint64_t slots, base;        // search slots of the grid, and their base arenas at the start of the pool
    uint64_t dyn, reserve;       // behind them: what the searches grow into, then the lowest running search's reserve
    uint64_t pool_bytes, soft_limit;
    uint32_t active_slots, ramp_base;
};
// Ordered launches (window B >= 1) never re-run single searches: a search that starves yields its memory and starts again in place
// (astar_kernel.hpp), so the result stays a function of (seed order, B, rate), and the lowest running search -- the one every later seed
// waits for -- has a RESERVE of its own behind the pool.  Only when that search has used up the reserve as well does the pass give up.
// Everything that has ended by then is final (a seed only ever started once nothing unfinished could still become visible to it), so the
// next pass RESUMES behind the commit frontier: results, caches and statuses stay, the seeds that have not ended run again in their order,
// with a larger share of the memory in the reserve (1/8, 1/2, 7/8; the last pass one search per direction at a time with everything).
// The reference has no such limit to hit: PoolST / HashMapST grow until the host is out of memory (pool_st.h:43, hash_table_st.h:559-568).
// The plan of pass `attempt` (0..3) for the seeds in `todo`, `free_b` bytes free on the device beside the pool `held`: arithmetic only.
PassPlan plan_pass(const Batch &b, int attempt, const std::vector<int64_t> todo[2], uint64_t free_b, const DevBuf &held) {
    const mgta_ctx *ctx = b.ctx; const int64_t work = (int64_t)std::max(todo[0].size(), todo[1].size()), spb = b.spb;
    PassPlan p;
    // persistent grid: one workgroup per CU and direction pair, fewer when there is little work; a pass that re-runs the
    // searches the pool could not hold runs fewer at a time
    const int64_t per_device = (int64_t)ctx->num_cus * (b.use_lds ? 1 : 2);
    int64_t blocks = std::min<int64_t>(per_device, 2 * ((work + spb - 1) / spb));
    // a context that shares the device with another batch (two genes searched side by side) takes its share of the CUs
    blocks = std::min<int64_t>(blocks, std::max<int64_t>(2, per_device * ctx->search_share_num / ctx->search_share_den));
    if (!b.gated && attempt == 2) blocks = std::max<int64_t>(2, blocks / 8);
    if (attempt == 3) blocks = 2;
    blocks = std::max<int64_t>(2, blocks + (blocks & 1));
    p.blocks = blocks; p.slots = (uint64_t)blocks * spb; p.base = p.slots * b.slot_bytes;
    // the two directions share the workgroups by the work their seeds promise, between a quarter and three quarters each: a forward search
    // from model position s has M - s - (k+1)/3 columns to cover, a reverse one s (with halves, half the device idled for half of a 50 M-read run)
    double w_dir[2] = {0, 0};
    for (int d = 0; d < 2; ++d)
        for (int64_t sd : todo[d]) {
            const double cols = d == 0 ? (double)(b.hm[0]->M - b.start_state[sd] - b.klen / 3) : (double)b.start_state[sd];
            w_dir[d] += std::max(1.0, cols);
        }
    int64_t blocks0 = (int64_t)std::llround((double)blocks * w_dir[0] / std::max(1.0, w_dir[0] + w_dir[1]));
    blocks0 = std::max<int64_t>(std::max<int64_t>(1, blocks / 4), std::min<int64_t>(blocks - std::max<int64_t>(1, blocks / 4), blocks0));
    if (todo[0].empty()) blocks0 = 1;
    if (todo[1].empty()) blocks0 = blocks - 1;
    p.blocks_dir0 = blocks0;
    // pool = the slots' base arenas + what the searches grow into (+ the reserve).  Device memory beyond the first ~24 GB of a process costs
    // 20-90 ms/GB to obtain (profiles/r02/vmm_probe.log), so the pool follows the job: at least 4 GB; 24 MB per search in flight (196 GB
    // for a full grid) for independent searches -- at 100 M reads they average 29 k expansions and hold 62 GB together -- and 8 MB per slot
    // where the searches share their paths and most end after a few hundred; 16 MB for a million searches and more or on graphs of billions
    // of edges, where they run longer, 24 MB at two million (50 M-read multi-k graphs: a gene copy's first searches reach 150-500 MB each).
    const uint64_t n_search = (uint64_t)work * 2;
    const uint64_t per_slot = b.cache_mode == 0 ? (24ull << 20) : (n_search >= (1ull << 20) || b.g->dev.size > (3ll << 30)) ? (n_search >= (1ull << 21) ? (24ull << 20) : (16ull << 20)) : (8ull << 20);
    uint64_t dyn = ctx->astar_pool_bytes ? ctx->astar_pool_bytes : std::max<uint64_t>(4ull << 30, std::min<uint64_t>(p.slots, n_search) * per_slot);
    const uint64_t avail = (uint64_t)((double)(free_b + held.bytes) * 0.8);
    const uint64_t room = avail > p.base ? avail - p.base : 0;
    uint64_t reserve = 0;
    if (b.gated) {
        // dyn is what the searches share, the reserve comes on top in the first pass (an eighth of it, at least 1 GB where the
        // pool is sized by the job); a pass that resumes takes all the memory there is and moves the border
        static const int kShare8[4] = {1, 4, 7, 0};                         // eighths of the whole in the reserve
        if (ctx->astar_pool_bytes) {                                        // (tests: pool_bytes is the whole)
            reserve = attempt < 3 ? dyn * kShare8[attempt] / 8 : 0;
            dyn -= reserve;
        } else if (attempt == 0) {
            reserve = std::max<uint64_t>(dyn / 8, 1ull << 30);
            if (dyn + reserve > room) { const uint64_t whole = std::min(dyn + reserve, room); reserve = whole / 8; dyn = whole - reserve; }
        } else {
            reserve = attempt < 3 ? room / 8 * kShare8[attempt] : 0;
            dyn = room - reserve;
        }
    } else {
        // the first re-run has the pool of the first pass to itself with a fraction of the searches; only the later ones ask for
        // everything that is free (obtaining 200 GB takes seconds)
        if (attempt == 1 && !ctx->astar_pool_bytes && held.bytes > p.base) dyn = std::max<uint64_t>(dyn, held.bytes - p.base);
        if (attempt > 1 && !ctx->astar_pool_bytes) dyn = avail;
        dyn = std::min<uint64_t>(dyn, room);
    }
    // a pool of nearly that size is there (the previous gene's, sized from a slightly different count of free bytes): keep it
    // rather than obtain 100+ GB again for a few per cent more
    if (attempt == 0 && !ctx->astar_pool_bytes && held.p && held.bytes > p.base + reserve &&
        held.bytes - p.base - reserve >= dyn - dyn / 4 && held.bytes - p.base - reserve < dyn)
        dyn = held.bytes - p.base - reserve;
    p.dyn = dyn & ~((1ull << kUnitLog) - 1); p.reserve = reserve & ~((1ull << kUnitLog) - 1);
    p.pool_bytes = p.base + p.dyn + p.reserve;
    // admission: no new search starts while HALF of the pool is in use, so that the searches that run keep room to grow (and a small pool
    // costs searches in flight, not failures).  More pays at 50 M reads and is past a cliff at 100 M reads (75 %: nirK not done after 900 s,
    // 391 s with half); where the cliff lies depends on how much the searches in flight still have to grow, which nothing knows when they
    // are admitted (profiles/r06/soft_limit/).
    p.soft_limit = p.dyn / 2;
    p.active_slots = attempt == 3 ? 1u : (uint32_t)spb;
    p.ramp_base = (uint32_t)std::max<uint64_t>(64, p.slots / 16);              // an eighth of a direction's slots
    return p;
}
// the pool as the plan wants it, and its free lists: one stack per class, as many entries as chunks of that class fit into the pool (capped)
void upload_pool(Batch &b, const PassPlan &p) {
    mgta_ctx *ctx = b.ctx; AstarArenas &ar = ctx->astar;
    if (ar.pool.bytes < p.pool_bytes || !ar.pool.p) { ar.pool.release(); ar.pool.alloc(p.pool_bytes, &ctx->live_bytes, &ctx->peak_bytes); }
    std::vector<uint32_t> meta(2 * kNumClasses);
    uint64_t stack_words = 0;
    for (int c = 0; c < kNumClasses; ++c) {
        const uint64_t fit = std::min<uint64_t>((p.dyn >> (c + kUnitLog)) + 1, 1ull << 20);
        meta[c] = (uint32_t)stack_words; meta[kNumClasses + c] = (uint32_t)fit;
        stack_words += fit;
    }
    const size_t meta_bytes = (kMetaStack + stack_words) * 4 + 64;
    if (ar.meta.bytes < meta_bytes) ar.meta.alloc(meta_bytes, &ctx->live_bytes, &ctx->peak_bytes);
    uint32_t *w = ar.meta.as<uint32_t>();
    MGTA_HIP_CHECK(hipMemsetAsync(w, 0, kMetaMeta * 4, b.st));
    MGTA_HIP_CHECK(hipMemcpyAsync(w + kMetaMeta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, b.st));
    const unsigned long long bump0 = p.base;
    MGTA_HIP_CHECK(hipMemcpyAsync(w + kMetaBump, &bump0, 8, hipMemcpyHostToDevice, b.st));
    PoolDev &pool = b.a.pool;
    pool.base = ar.pool.as<char>(); pool.bytes = p.base + p.dyn; pool.reserve_off = p.base + p.dyn; pool.reserve_bytes = p.reserve;
    pool.bump = reinterpret_cast<unsigned long long *>(w + kMetaBump); pool.stat = reinterpret_cast<unsigned long long *>(w + kMetaStat);
    pool.lock = w + kMetaLock; pool.cnt = w + kMetaCnt; pool.meta = w + kMetaMeta; pool.stack = w + kMetaStack;
    pool.soft_limit = p.soft_limit;
}
// MGTA_ASTAR_MONITOR=<seconds>: while the launch runs, a line on stderr every so often -- where the queues are, how many slots
// hold a search, the lowest running seed and how far it is, the memory in use.  Copies on a stream of their own: the words are
// written by atomics performed at the memory side, so what the copy engine reads is recent.
void monitor_launch(const Batch &b, const PassPlan &p, hipEvent_t done, const char *me) {
    const double every = std::max(1.0, atof(me));
    const int cache_mode = b.cache_mode; const uint64_t slots = p.slots;
    hipStream_t ms = nullptr; MGTA_HIP_CHECK(hipStreamCreateWithFlags(&ms, hipStreamNonBlocking));
    std::vector<long long> h_rs(cache_mode > 0 ? slots : 0);
    std::vector<unsigned long long> h_rp(cache_mode > 0 ? slots : 0);
    const auto t_start = std::chrono::steady_clock::now();
    double next = every;
    while (hipEventQuery(done) == hipErrorNotReady) {
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
        if (el < next) continue;
        next += every;
        unsigned long long q[2] = {0, 0}, lim[kCtlWords] = {0}; PoolHead pl{};
        (void)hipMemcpyAsync(q, b.d_queue.p, 16, hipMemcpyDeviceToHost, ms);
        (void)hipMemcpyAsync(&pl, b.ctx->astar.meta.p, sizeof(pl), hipMemcpyDeviceToHost, ms);
        if (cache_mode > 0) {
            (void)hipMemcpyAsync(lim, b.d_start_limit.p, sizeof(lim), hipMemcpyDeviceToHost, ms);
            (void)hipMemcpyAsync(h_rs.data(), b.d_run_seed.p, slots * 8, hipMemcpyDeviceToHost, ms);
            (void)hipMemcpyAsync(h_rp.data(), b.d_run_progress.p, slots * 8, hipMemcpyDeviceToHost, ms);
        }
        (void)hipStreamSynchronize(ms);
        long long lo = -1, lo_dir = 0, busy = 0, big = -1, big_dir = 0;
        unsigned long long lo_prog = 0, big_prog = 0;
        for (size_t sl = 0; sl < h_rs.size(); ++sl)
            if (h_rs[sl] >= 0) {
                ++busy;
                const long long d = sl >= (size_t)p.blocks_dir0 * (size_t)b.spb ? 1 : 0;
                if (lo < 0 || h_rs[sl] * 2 + d < lo * 2 + lo_dir) { lo = h_rs[sl]; lo_dir = d; lo_prog = h_rp[sl]; }
                if (h_rp[sl] > big_prog) { big = h_rs[sl]; big_dir = d; big_prog = h_rp[sl]; }
            }
        if (big >= 0)
            fprintf(stderr, "[astar]          longest running search: seed %lld (direction %lld, start state %d) at >= %llu expansions, k-mer %.45s\n", big, big_dir,
                    b.start_state[big], big_prog, b.kmers + (size_t)big * b.klen);
        const long long q0 = (long long)std::min<unsigned long long>(q[0], b.todo[0].size()), q1 = (long long)std::min<unsigned long long>(q[1], b.todo[1].size());
        fprintf(stderr, "[astar] %6.0f s: seeds taken %lld + %lld of %zu + %zu; %lld slots hold a search; lowest running seed %lld (direction %lld) at >= %llu "
                "expansions%s%.45s; start limits %llu / %llu; pool %.1f GB in use (%.1f GB handed out once), reserve %.2f GB in use, owner %lld; %llu in-place restarts\n",
                el, q0, q1, b.todo[0].size(), b.todo[1].size(), busy, lo, lo_dir, lo_prog, lo >= 0 ? ", k-mer " : "", lo >= 0 ? b.kmers + (size_t)lo * b.klen : "",
                lim[kCtlLimit], lim[kCtlLimit + 1], pl.stat[kStatInUse] / 1e9, pl.bump / 1e9, lim[kCtlReserve + kReserveBump] / 1e9,
                (long long)lim[kCtlReserve + kReserveOwner] - 1, pl.stat[kStatRestarts]);
    }
    (void)hipStreamDestroy(ms);
}
// what a pass leaves behind besides the statuses (read into Batch::h_status)
struct PassOut {
    PoolHead pool;                                      // the pool's bump pointer and PoolStat words
    unsigned long long ctl[kCtlWords], tmark[4];        // the control words (all 0 in cold batches), AstarArgs::tmark
    uint32_t cnt[kNumClasses];                          // free chunks per class
    float ms;                                           // kernel time
};
// one launch over b.todo: its per-pass arguments, the launch, the wait, the read-back
PassOut run_pass(Batch &b, const PassPlan &p, bool unordered, Events &ev) {
    const hipStream_t st = b.st; AstarArgs &a = b.a;
    a.blocks_dir0 = (uint32_t)p.blocks_dir0; a.active_slots = p.active_slots; a.ramp_base = p.ramp_base;
    if (b.cache_mode > 0) {
        MGTA_HIP_CHECK(hipMemsetAsync(b.d_start_limit.p, 0, kCtlWords * 8, st));   // (limits are recomputed: a conservative restart of the gate)
        if (unordered) {                                                        // (a batch that gave its order up resumes without one)
            const unsigned long long one = 1;
            MGTA_HIP_CHECK(hipMemcpyAsync(b.d_start_limit.as<unsigned long long>() + kCtlUnordered, &one, 8, hipMemcpyHostToDevice, st));
        }
        b.d_run_seed.alloc(p.slots * 8); b.d_run_progress.alloc(p.slots * 8);
        MGTA_HIP_CHECK(hipMemsetAsync(b.d_run_seed.p, 0xFF, p.slots * 8, st));
        MGTA_HIP_CHECK(hipMemsetAsync(b.d_run_progress.p, 0, p.slots * 8, st));
        a.run_seed = b.d_run_seed.as<long long>(); a.run_progress = b.d_run_progress.as<unsigned long long>(); a.n_slots = (uint32_t)p.slots;
    }
    MGTA_HIP_CHECK(hipMemsetAsync(b.d_queue.p, 0, 16, st));
    for (int d = 0; d < 2; ++d) {
        b.d_todo[d].alloc(std::max<size_t>(1, b.todo[d].size()) * 8);
        if (!b.todo[d].empty()) MGTA_HIP_CHECK(hipMemcpyAsync(b.d_todo[d].p, b.todo[d].data(), b.todo[d].size() * 8, hipMemcpyHostToDevice, st));
        a.todo[d] = b.d_todo[d].as<int64_t>(); a.n_todo[d] = (int64_t)b.todo[d].size();
    }
    MGTA_HIP_CHECK(hipEventRecord(ev.e[2], st));
    MGTA_HIP_CHECK(hipMemsetAsync(b.d_tmark.p, 0xFF, 32, st));
    const int blocks = (int)p.blocks;
    if (b.G == 8) launch_astar<8>(a, blocks, b.lds_bytes, b.use_lds, st);
    else if (b.G == 16) launch_astar<16>(a, blocks, b.lds_bytes, b.use_lds, st);
    else if (b.G == 32) launch_astar<32>(a, blocks, b.lds_bytes, b.use_lds, st);
    else launch_astar<64>(a, blocks, b.lds_bytes, b.use_lds, st);
    MGTA_HIP_CHECK(hipEventRecord(ev.e[3], st));
    if (const char *me = getenv("MGTA_ASTAR_MONITOR")) monitor_launch(b, p, ev.e[3], me);
    PassOut o{};
    MGTA_HIP_CHECK(hipMemcpyAsync(b.h_status.data(), b.d_status.p, (size_t)b.n * 8, hipMemcpyDeviceToHost, st));
    MGTA_HIP_CHECK(hipMemcpyAsync(&o.pool, b.ctx->astar.meta.p, sizeof(o.pool), hipMemcpyDeviceToHost, st));
    MGTA_HIP_CHECK(hipMemcpyAsync(o.cnt, b.ctx->astar.meta.as<uint32_t>() + kMetaCnt, sizeof(o.cnt), hipMemcpyDeviceToHost, st));
    if (b.cache_mode > 0) MGTA_HIP_CHECK(hipMemcpyAsync(o.ctl, b.d_start_limit.p, sizeof(o.ctl), hipMemcpyDeviceToHost, st));
    MGTA_HIP_CHECK(hipMemcpyAsync(o.tmark, b.d_tmark.p, sizeof(o.tmark), hipMemcpyDeviceToHost, st));
    MGTA_HIP_CHECK(hipStreamSynchronize(st));
    MGTA_HIP_CHECK(hipGetLastError());
    MGTA_HIP_CHECK(hipEventElapsedTime(&o.ms, ev.e[2], ev.e[3]));
    return o;
}
// the stats and messages of a pass, and what runs again: b.todo becomes the seeds the next pass takes
int account_pass(Batch &b, int attempt, const PassPlan &p, const PassOut &o, mgta_astar_stats &ST) {
    const unsigned long long *stat = o.pool.stat; ST.ms_kernel += o.ms;
    if (attempt == 0 && o.tmark[0] != ~0ull) {                                // when the last seed of the batch was TAKEN: what follows is the tail
        double drained = 0;
        for (int d = 0; d < 2; ++d)
            if (o.tmark[1 + d] != ~0ull && o.tmark[1 + d] >= o.tmark[0]) drained = std::max(drained, (double)(o.tmark[1 + d] - o.tmark[0]) * 1e-5);
        ST.ms_queue_drained = drained;
    }
    ST.n_recycled += (int64_t)stat[kStatRecycled]; ST.n_rehash += (int64_t)stat[kStatRehash]; ST.n_grown += (int64_t)stat[kStatGrown];
    ST.n_retries += (int64_t)stat[kStatRestarts];                             // searches that started again in place
    ST.pool_bytes = p.pool_bytes; ST.reserve_bytes = p.reserve;
    ST.pool_used = std::max<uint64_t>(ST.pool_used, p.base + stat[kStatInUseHigh]);   // base arenas + most ever handed out at once
    const unsigned long long reserve_high = o.ctl[kCtlReserve + kReserveHigh], cache_drops = o.ctl[kCtlCacheDrops];
    ST.reserve_used = std::max<uint64_t>(ST.reserve_used, reserve_high); ST.n_cache_drops += (int64_t)cache_drops;
    if (o.ctl[kCtlUnordered] && !ST.order_abandoned) {
        ST.order_abandoned = 1;
        fprintf(stderr, "[megagta_amd] search: the searches in flight outgrew their pool (%.1f GB, %llu requests refused): the batch of %lld seeds gave up the ORDER of its "
                "cache sharing from there on -- every path is seen by every search as soon as it is found, as in the reference's multi-thread search "
                "(search.cpp:182-189); which of several equally good paths a later seed takes depends on timing (MEGAGTA_SEARCH_ALLOW_UNORDERED=1 asked for this).\n",
                p.pool_bytes / 1e9, stat[kStatRefused], (long long)b.n);
    }
    if (b.gated && cache_drops)
        fprintf(stderr, "[megagta_amd] search: %llu path entries found no room in the shared cache (%.1f GB per direction): later seeds may have searched "
                "where they could have followed a path -- which ones depends on timing\n", cache_drops, b.d_cache[0].bytes / 1e9);
    // A search that reached the page tables' limit is terminal at once (more memory or another pass cannot help, and the searches behind it
    // have seen nothing of it).  It is ONE seed's side: a failed search (ok = 0), named on stderr and counted in n_over_limit, while the batch
    // goes on -- a multi-k run of hours is not thrown away for it.  MEGAGTA_SEARCH_STRICT_LIMIT=1: the batch fails with MGTA_EOVERFLOW.
    for (int64_t s = 0; s < b.n * 2; ++s)
        if (b.h_status[(size_t)s] == kSearchOverLimit && !b.over_limit_seen[(size_t)s]) {
            b.over_limit_seen[(size_t)s] = 1;
            char msg[384];
            snprintf(msg, sizeof(msg), "search %lld (seed %lld, %s) outgrew the %s limit of %u pages of %d KB per array (~%.2f M nodes): the reference's pool has no "
                     "bound (pool_st.h:43), this build's page tables do", (long long)s, (long long)(s / 2), (s & 1) ? "left" : "right",
                     b.ctx->search_page_limit ? "context's" : "library's", b.a.page_limit, 1 << (kPageLog - 10),
                     (double)((uint64_t)b.a.page_limit << (kPageLog - 6)) / (1 << 20));
            const char *strict = getenv("MEGAGTA_SEARCH_STRICT_LIMIT");
            if (strict && atoi(strict) != 0) { set_error("%s", msg); return MGTA_EOVERFLOW; }
            fprintf(stderr, "[megagta_amd] search: %s -- this side of the seed is reported as a failed search, the batch goes on\n", msg);
            ++ST.n_over_limit;
        }
    size_t left = 0, starved_out = 0;
    for (int d = 0; d < 2; ++d) {
        std::vector<int64_t> again;
        for (int64_t s : b.todo[d]) {
            const int32_t v = b.h_status[(size_t)s * 2 + d];
            if (v == kSearchStarved) ++starved_out;
            if (v == kSearchStarved || (b.gated && v == kSearchPending)) again.push_back(s);   // (ordered: whatever has not ended runs again, in seed order)
        }
        b.todo[d].swap(again);
        left += b.todo[d].size();
    }
    if (getenv("MGTA_ASTAR_VERBOSE") != nullptr || (b.gated && left)) {
        std::string lists;
        for (int c = 0; c < kNumClasses; ++c)
            if (o.cnt[c]) { char t[48]; snprintf(t, sizeof(t), " %u x %s", o.cnt[c], c + kUnitLog >= 30 ? (std::to_string(1u << (c + kUnitLog - 30)) + " GB").c_str() : c + kUnitLog >= 20 ? (std::to_string(1u << (c + kUnitLog - 20)) + " MB").c_str() : (std::to_string(1u << (c + kUnitLog - 10)) + " KB").c_str()); lists += t; }
        fprintf(stderr, "[astar] pass %d: %lld workgroups, pool %.1f GB (reserve %.1f GB, %.1f GB of it used), handed out once %.1f GB, most in use %.1f GB, "
                "%llu chunks reused, %llu requests refused, %llu searches started again in place, %.0f ms, %zu searches to run again; free lists at the end:%s\n",
                attempt, (long long)p.blocks, p.pool_bytes / 1e9, p.reserve / 1e9, reserve_high / 1e9, o.pool.bump / 1e9, (p.base + stat[kStatInUseHigh]) / 1e9,
                stat[kStatRecycled], stat[kStatRefused], stat[kStatRestarts], o.ms, left, lists.empty() ? " none" : lists.c_str());
    }
    if (b.gated && left) {
        ++ST.n_resumes;
        fprintf(stderr, "[megagta_amd] search: %zu search(es) found no memory even as the lowest running seed with a reserve of %.1f GB (pool %.1f GB); "
                "the batch of %lld seeds resumes behind its commit frontier (%zu searches left) with a larger reserve\n", starved_out, p.reserve / 1e9,
                p.pool_bytes / 1e9, (long long)b.n, left);
        for (int d = 0; d < 2; ++d)                                          // (kSearchStarved -> kSearchPending: a search that is cut off again must not look starved)
            for (int64_t s : b.todo[d]) b.h_status[(size_t)s * 2 + d] = kSearchPending;
        MGTA_HIP_CHECK(hipMemcpyAsync(b.d_status.p, b.h_status.data(), (size_t)b.n * 8, hipMemcpyHostToDevice, b.st));
    } else {
        ST.n_retries += (int64_t)left;                                       // independent searches run again by the host
    }
    return MGTA_OK;
}
#ifdef MGTA_ASTAR_PROFILE
void profile_report(const Batch &b) {
    unsigned long long hp[16];
    MGTA_HIP_CHECK(hipMemcpy(hp, b.d_prof.p, 128, hipMemcpyDeviceToHost));
    // the clock the counts are in (s_memtime ticks per 10 ns of s_memrealtime); [3..8] are sums over the SEARCHES that expanded (per
    // expansion of one search), the rest per wave (see PROF_DECL in astar_kernel.hpp)
    const double mhz = hp[12] ? 100.0 * (double)hp[13] / (double)hp[12] : 0.0, exps = (double)(hp[10] ? hp[10] : 1), iters = (double)(hp[11] ? hp[11] : 1);
    const char *nm[10] = {"fetch", "gate", "start", "pop+closed", "grow", "cache+walk", "score+probe", "commit", "(run end)", "result+free"};
    double sum = 0;
    for (int q = 3; q <= 8; ++q) sum += (double)hp[q];
    fprintf(stderr, "[astar-prof] lanes per search %d; clock of the counts %.0f MHz; %llu expansions in %llu expanding wave iterations (%.2f of %d searches expanding in each); "
            "one expansion of one search: %.2f us\n", b.G, mhz, hp[10], hp[11], exps / iters, 64 / b.G, mhz > 0 ? sum / exps / mhz : 0.0);
    for (int q = 3; q <= 8; ++q)
        fprintf(stderr, "[astar-prof]   %-12s %6.2f %%  %8.3f us per expansion of one search\n", nm[q], 100.0 * hp[q] / (sum > 0 ? sum : 1), mhz > 0 ? (double)hp[q] / exps / mhz : 0.0);
    for (int q : {0, 1, 2, 9})
        fprintf(stderr, "[astar-prof]   %-12s %8.3f us per expanding wave iteration (wave-level)\n", nm[q], mhz > 0 ? (double)hp[q] / iters / mhz : 0.0);
    fprintf(stderr, "[astar-prof]   asleep (every running search of the wave waits for memory): %llu times, %.3f us per expanding wave iteration\n",
            hp[15], mhz > 0 ? (double)hp[14] / iters / mhz : 0.0);
}
#endif
struct Results {                 // per side (2 * seed + direction): its record, and its string at out[off .. off + len)
    std::vector<mgta_astar_side> sides; std::vector<uint32_t> len; std::vector<uint64_t> off;
    std::vector<char> out; uint64_t n_chars = 0;
};
// results: records and lengths as they are, the strings packed on the device first; the batch's totals into ST
int collect_results(const Batch &b, Events &ev, Results &r, mgta_astar_stats &ST) {
    const hipStream_t st = b.st; const uint64_t n_sides = (uint64_t)b.n * 2;
    r.sides.resize(n_sides); r.len.resize(n_sides); r.off.resize(n_sides);
    DevBuf d_off, d_scan_tmp, d_tot, d_packed;
    d_off.alloc(n_sides * 8); d_scan_tmp.alloc(scan_tmp_elems(n_sides) * 8); d_tot.alloc(64);
    exclusive_scan_u32(st, b.d_len.as<uint32_t>(), n_sides, d_off.as<uint64_t>(), d_scan_tmp.as<uint64_t>(), d_tot.as<uint64_t>());
    MGTA_HIP_CHECK(hipMemcpyAsync(&r.n_chars, d_tot.p, 8, hipMemcpyDeviceToHost, st));
    MGTA_HIP_CHECK(hipStreamSynchronize(st));
    d_packed.alloc(r.n_chars + 64);
    hipLaunchKernelGGL(pack_results_kernel, dim3((unsigned)std::min<uint64_t>((n_sides + 3) / 4, 1u << 16)), dim3(256), 0, st, b.d_out.as<char>(), b.a.out_cap,
                       b.d_len.as<uint32_t>(), d_off.as<uint64_t>(), n_sides, d_packed.as<char>());
    MGTA_HIP_CHECK(hipGetLastError());
    r.out.resize(r.n_chars + 1);
    MGTA_HIP_CHECK(hipMemcpyAsync(r.sides.data(), b.d_sides.p, r.sides.size() * sizeof(mgta_astar_side), hipMemcpyDeviceToHost, st));
    MGTA_HIP_CHECK(hipMemcpyAsync(r.len.data(), b.d_len.p, r.len.size() * 4, hipMemcpyDeviceToHost, st));
    MGTA_HIP_CHECK(hipMemcpyAsync(r.off.data(), d_off.p, r.off.size() * 8, hipMemcpyDeviceToHost, st));
    if (r.n_chars) MGTA_HIP_CHECK(hipMemcpyAsync(r.out.data(), d_packed.p, r.n_chars, hipMemcpyDeviceToHost, st));
    MGTA_HIP_CHECK(hipEventRecord(ev.e[1], st));
    MGTA_HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0;
    MGTA_HIP_CHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    ST.ms_total = ms;
    for (uint64_t s = 0; s < n_sides; ++s) {
        if (b.h_status[s] == kSearchBadSeed) {
            set_error("seed %lld: k-mer / model position outside the model (start_state %d)", (long long)(s / 2), b.start_state[s / 2]);
            return MGTA_EINVAL;
        }
        ST.n_expansions += r.sides[s].n_expanded;
        ST.n_opened += r.sides[s].n_opened;
        ST.max_search_nodes = std::max<int64_t>(ST.max_search_nodes, (uint32_t)r.sides[s].n_opened);
        ST.max_search_expansions = std::max<int64_t>(ST.max_search_expansions, (uint32_t)r.sides[s].n_expanded);
    }
    return MGTA_OK;
}
void rev_comp(char *dst, const char *l, uint32_t ll) {                         // RevComp, hmm_graph_search.h:362-398
    for (uint32_t i = 0; i < ll; ++i) { const char c = l[ll - 1 - i]; dst[i] = c == 'a' ? 't' : c == 'c' ? 'g' : c == 'g' ? 'c' : c == 't' ? 'a' : c; }
}
// the contigs to the caller: one malloc'd buffer (packed) or one call of the sink per seed
int deliver(const Batch &b, const Results &r, const PackedOut *packed, mgta_contig_sink sink, void *user) {
    const int64_t n = b.n; const int klen = b.klen;
    if (packed) {
        // contig i = left + lower-cased seed k-mer + right (hmm_graph_search.h:60-81), written once into its final place
        const uint64_t total = r.n_chars + (uint64_t)n * (uint64_t)klen;
        char *buf = static_cast<char *>(malloc(total + 1));
        if (!buf) { set_error("mgta_astar_batch_packed: out of host memory"); return MGTA_ENOMEM; }
        uint64_t at = 0;
        for (int64_t s = 0; s < n; ++s) {
            packed->offsets[s] = at;
            const uint32_t ll = r.len[(size_t)2 * s + 1], rl = r.len[(size_t)2 * s];
            rev_comp(buf + at, r.out.data() + r.off[(size_t)2 * s + 1], ll);
            at += ll;
            const char *km = b.kmers + (size_t)s * klen;
            for (int j = 0; j < klen; ++j) buf[at + j] = (char)tolower((unsigned char)km[j]);   // the seed k-mer, lower case (search.cpp:156)
            at += klen;
            memcpy(buf + at, r.out.data() + r.off[(size_t)2 * s], rl);
            at += rl;
        }
        packed->offsets[n] = at;
        buf[at] = 0;
        if (packed->sides) memcpy(packed->sides, r.sides.data(), r.sides.size() * sizeof(mgta_astar_side));
        *packed->contigs = buf;
    } else if (sink) {
        std::string left;
        for (int64_t s = 0; s < n; ++s) {
            const uint32_t ll = r.len[(size_t)2 * s + 1];
            left.assign(ll, ' ');
            rev_comp(&left[0], r.out.data() + r.off[(size_t)2 * s + 1], ll);
            int src = sink(user, s, left.data(), (int64_t)ll, r.out.data() + r.off[(size_t)2 * s], (int64_t)r.len[(size_t)2 * s], &r.sides[(size_t)2 * s], &r.sides[(size_t)2 * s + 1]);
            if (src != 0) { set_error("contig sink returned %d", src); return MGTA_ESINK; }
        }
    }
    return MGTA_OK;
}
int astar_batch_impl(mgta_ctx *ctx, mgta_sdbg *g, const mgta_hmm *fwd, const mgta_hmm *rev, const char *kmers, const int32_t *start_state,
                     int64_t n, int prune_len, double low_cov_penalty, int cache_mode, mgta_contig_sink sink, void *user,
                     mgta_astar_stats *stats, const PackedOut *packed) {
    if (!ctx || !g || !fwd || !rev || n < 0 || (n > 0 && (!kmers || !start_state))) { set_error("mgta_astar_batch: bad argument"); return MGTA_EINVAL; }
    if (cache_mode < -1) { set_error("cache_mode must be >= -1"); return MGTA_EINVAL; }
    const bool free_share = cache_mode == -1;          // shared caches without any ordering (timing-dependent results, like the reference's OMP run)
    if (free_share) cache_mode = 1;
    if (ctx->device != g->ctx->device) { set_error("mgta_astar_batch_on: the context and the graph live on different devices"); return MGTA_EINVAL; }
    const int klen = g->dev.k + 1;
    if (klen > kMaxKmer) { set_error("k too large"); return MGTA_EINVAL; }
    MGTA_HIP_CHECK(hipSetDevice(ctx->device));                                 // (throws from here on: both entry points below call this under guarded())
    mgta_astar_stats ST{};
    ST.n_seeds = n;
    Batch b{ctx, g, ctx->stream, {fwd, rev}, kmers, start_state, n, klen, cache_mode, free_share, cache_mode > 0 && !free_share};
    if (n == 0) {                                                          // (nothing runs; a packed call still gets its empty buffer)
        const int rc = deliver(b, Results{}, packed, sink, user);
        if (rc == MGTA_OK && stats) *stats = ST;
        return rc;
    }
    Events ev;
    MGTA_HIP_CHECK(hipEventRecord(ev.e[0], b.st));
    std::vector<int64_t> start_node;
    int rc = encode_start_edges(g, kmers, n, klen, start_node);
    if (rc != MGTA_OK) return rc;
    b.G = lanes_per_search(b); b.spb = (int64_t)kAstarWaves * (64 / b.G);
    upload_batch(b, start_node, prune_len, low_cov_penalty, ST);
    for (int d = 0; d < 2; ++d) { b.todo[d].resize(n); for (int64_t s = 0; s < n; ++s) b.todo[d][s] = s; }
    longest_first(b);
    b.h_status.resize((size_t)n * 2); b.over_limit_seen.resize((size_t)n * 2);
    size_t free_b = 0, total_b = 0;
    MGTA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (cache_mode > 0) alloc_caches(b, free_b);
    for (int attempt = 0; attempt < 4 && (!b.todo[0].empty() || !b.todo[1].empty()); ++attempt) {
        const PassPlan p = plan_pass(b, attempt, b.todo, free_b, ctx->astar.pool);
        upload_pool(b, p);
        const PassOut o = run_pass(b, p, ST.order_abandoned != 0, ev);
        rc = account_pass(b, attempt, p, o, ST);
        if (rc != MGTA_OK) return rc;
        MGTA_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    }
    if (!b.todo[0].empty() || !b.todo[1].empty()) {
        set_error("%zu searches do not fit the device memory left for them (pool of %llu bytes)", b.todo[0].size() + b.todo[1].size(),
                  (unsigned long long)ST.pool_bytes);
        return MGTA_EOVERFLOW;
    }
    for (int64_t s = 0; s < n * 2; ++s)
        if (b.h_status[(size_t)s] == kSearchGateTimeout || b.h_status[(size_t)s] == kSearchPending) {
            set_error("search %lld did not run (ordered-commit gate timed out)", (long long)s);
            return MGTA_EHIP;
        }
#ifdef MGTA_ASTAR_PROFILE
    profile_report(b);
#endif
    Results r;
    rc = collect_results(b, ev, r, ST);
    if (rc == MGTA_OK) rc = deliver(b, r, packed, sink, user);
    if (rc == MGTA_OK && stats) *stats = ST;
    return rc;
}
}  // namespace

extern "C" {
int mgta_astar_batch_on(mgta_ctx *ctx, mgta_sdbg *g, const mgta_hmm *fwd, const mgta_hmm *rev, const char *kmers, const int32_t *start_state,
                        int64_t n, int prune_len, double low_cov_penalty, int cache_mode, mgta_contig_sink sink, void *user,
                        mgta_astar_stats *stats) {
    return guarded("mgta_astar_batch", [&] {
        return astar_batch_impl(ctx, g, fwd, rev, kmers, start_state, n, prune_len, low_cov_penalty, cache_mode, sink, user, stats, nullptr);
    });
}
// The same batch with the results in flat arrays instead of one call-back per seed (a Python caller pays microseconds per call-back:
// minutes at millions of seeds): contig i = (*contigs)[offsets[i] .. offsets[i + 1]) = left + lower-cased k-mer + right, exactly the
// sequence line `search` writes (hmm_graph_search.h:60-81).
int mgta_astar_batch_packed(mgta_sdbg *g, const mgta_hmm *fwd, const mgta_hmm *rev, const char *kmers, const int32_t *start_state, int64_t n,
                            int prune_len, double low_cov_penalty, int cache_mode, char **contigs, uint64_t *offsets, mgta_astar_side *sides,
                            mgta_astar_stats *stats) {
    if (!g || !contigs || !offsets) { set_error("mgta_astar_batch_packed: bad argument"); return MGTA_EINVAL; }
    *contigs = nullptr;
    const PackedOut po{contigs, offsets, sides};
    const int rc = guarded("mgta_astar_batch_packed", [&] {
        return astar_batch_impl(g->ctx, g, fwd, rev, kmers, start_state, n, prune_len, low_cov_penalty, cache_mode, nullptr, nullptr, stats, &po);
    });
    if (rc != MGTA_OK && *contigs) { free(*contigs); *contigs = nullptr; }   // (a call that fails hands nothing over: the caller frees only what MGTA_OK gave it)
    return rc;
}
}  // extern "C"
