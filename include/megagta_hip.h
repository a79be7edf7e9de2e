/* megagta_hip.h — C ABI of libmegagta_hip.so: the MI355X (gfx950) implementation of MegaGTA's
 * HMM-guided succinct-de-Bruijn-graph assembly hot path.
 *
 * This is the in-process successor of the reference's dead GPU plug-point
 *     lv2_gpu_sort(uint32_t *lv2_substrings, uint32_t *permutation, int words_per_substring,
 *                  int64_t lv2_num_items, void *key1, void *key2, void *val1, void *val2)
 *     alloc_gpu_buffers(...) / free_gpu_buffers(...)
 * (call sites cx1_read2sdbg_s1.cpp:308,619-620,945 and cx1_read2sdbg_s2.cpp:391,697-698,926; the
 * functions themselves exist nowhere in the reference tree).  Instead of sorting one lv2 batch per
 * call, the whole read -> SdBG-edge pipeline, the graph and the A* search live on the device.
 *
 * Conventions: extern "C"; plain pointers and sizes; every function returns 0 on success and a
 * negative MGTA_E* code on failure (mgta_last_error() gives the message of the calling thread's
 * last failure); no exceptions cross the boundary; one mgta_ctx per GPU (thread-compatible).
 * There is NO CPU fallback: without a usable HIP device every entry point fails.
 */
#ifndef MEGAGTA_HIP_H_
#define MEGAGTA_HIP_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MGTA_OK 0
#define MGTA_EINVAL (-1)      /* bad argument */
#define MGTA_EHIP (-2)        /* HIP runtime error / no device */
#define MGTA_ENOMEM (-3)      /* device memory exhausted */
#define MGTA_EUNSUPPORTED (-4)/* feature of the reference not built yet (fails loudly, never silently) */
#define MGTA_ESINK (-5)       /* caller's sink returned non-zero */
#define MGTA_EOVERFLOW (-6)   /* per-search arena exhausted after all retries */
#define MGTA_EINTERNAL (-7)   /* a device-side protocol gave up (bounded wait expired); the call produced nothing */

#define MGTA_NUM_BUCKETS 65536 /* kNumBuckets, cx1_read2sdbg.h:64 (8-character key prefix) */

typedef struct mgta_ctx mgta_ctx;
typedef struct mgta_reads mgta_reads;
typedef struct mgta_sdbg mgta_sdbg;
typedef struct mgta_hmm mgta_hmm;

const char *mgta_last_error(void);
const char *mgta_version(void);

mgta_ctx *mgta_ctx_create(int device_id);            /* NULL on failure (see mgta_last_error) */
void mgta_ctx_destroy(mgta_ctx *);
/* memory the build may use on the device; 0 = 90 % of what is free (cf. --host_mem/--mem_flag, build_graph.cpp:40-47) */
int mgta_ctx_set_mem_limit(mgta_ctx *, uint64_t bytes);
int mgta_ctx_device_memory(mgta_ctx *, uint64_t *free_bytes, uint64_t *total_bytes);   /* of the context's device, now (either may be NULL) */
/* on: a build also leaves the WHOLE edge stream of its bucket range on the device when memory forces it into several bucket-range
 * passes (each pass is appended to a stream buffer), so that mgta_sdbg_load_resident can hand the graph of a whole-range build to
 * `denovo` / `search` without the disk or host round trip of `<prefix>.sdbg.*` (succinct_dbg.cpp:595-723) at any input size, and
 * mgta_sdbg_export_records_device hands a rank's shard (a bucket sub-range) to the all-gather in one piece.  off (default): only the
 * last pass stays.  Turning it off frees the buffer. */
int mgta_ctx_keep_stream(mgta_ctx *, int on);
/* on = 2: as 1, and the records and tip labels of a pass are NOT copied to the host for the sink (it is called with recs = tips = NULL,
 * counts and large multiplicities as usual): the caller takes the whole stream afterwards with the calls below.  `megagta buildgraph`
 * in the driver's worker: the graph is packed from the resident stream, the step ends, and a host thread downloads the stream and
 * writes PREFIX.sdbg.* (sdbg_multi_io.h:83-187) behind the step that follows.
 * mgta_sdbg_stream_detach: the whole stream of the last build leaves the context (which forgets it); it stays in device memory until
 * mgta_stream_free.  mgta_stream_download: records (uint16) and tip label words (uint32) into the caller's host memory, from any host
 * thread (a HIP stream and staging buffers of its own; nothing of the context is touched).  mgta_stream_free: on the context's thread. */
typedef struct mgta_stream mgta_stream;
int mgta_sdbg_stream_detach(mgta_ctx *, mgta_stream **out);
int mgta_stream_sizes(const mgta_stream *, uint64_t *n_recs, uint64_t *n_tip_words);
int mgta_stream_download(mgta_stream *, uint16_t *recs, uint32_t *tips);
void mgta_stream_free(mgta_stream *);
/* frees the grow-only work memory the context keeps between calls (build pool, search pool); a stream left in the build pool by a
 * single-pass build is dropped with it (one kept by mgta_ctx_keep_stream stays) */
int mgta_ctx_release_scratch(mgta_ctx *);
/* diagnostic switch (bit mask): 1 = sort every key with global LSD passes only (also the fallback for oversized segments);
 * 2 = the segment-local sort runs LSD passes over every remaining digit instead of finishing short runs by comparison
 *     (also the fallback for tiles whose runs are long) */
int mgta_ctx_set_full_lsd(mgta_ctx *, int on);
/* diagnostic, host only (no device needed): the global sort passes a build of `n_items` keys of `words_per_key` 32-bit words over the
 * buckets [bucket_begin, bucket_end) takes: *n_passes 8-bit digits taken below *skip_bits leading bits that every key of the range shares
 * once (bucket_begin << 16) is subtracted from key word 0 (0 for a whole-range build); the segment-local finish then sees segments of
 * equal leading 8 * n_passes + skip_bits bits.  Honours MGTA_SORT_BIAS. */
int mgta_sort_plan(uint64_t n_items, int words_per_key, uint32_t bucket_begin, uint32_t bucket_end, int *n_passes, int *skip_bits);
/* The plan the build really takes, wide digits included (MGTA_SORT_WIDE): widths[i] = bits of the i-th global pass to
 * run, i < *n_passes <= 4 (the first 8, later ones 8 or 9); the segment-local finish sees segments of equal leading
 * *skip_bits + sum(widths) bits.  Where wide digits save no pass this is mgta_sort_plan's answer with every width 8. */
int mgta_sort_plan_wide(uint64_t n_items, int words_per_key, uint32_t bucket_begin, uint32_t bucket_end, int *n_passes, int *skip_bits,
                        int *widths /* [4] */);
/* Shared-cache searches (mgta_astar_batch with cache_mode = B >= 1): the path found by seed j after c_j node expansions is seen by
 * exactly the seeds >= j + B + c_j / expansions_per_seed.  0 (default) = no cost term: seed i sees the seeds <= i - B, and every
 * later seed waits for the longest unfinished search.  > 0: a search that has already run r expansions cannot become visible to the
 * seeds below j + B + r / expansions_per_seed any more, so those start without waiting for it.  Either way the result is a function
 * of (seed order, B, expansions_per_seed) only, never of timing. */
int mgta_ctx_set_search_cost_rate(mgta_ctx *, int expansions_per_seed);   /* < 0 (down to -64): seeds per expansion, i.e. the path is
                                                                            * seen from seed j + B + c_j * |value| on */
/* The same with a CONCAVE cost term: c_j expansions delay the path of seed j by cost(c_j) = c_j / expansions_per_seed seeds while
 * c_j <= knee_expansions and by knee / expansions_per_seed + (c_j - knee) / expansions_per_seed_beyond seeds beyond (knee 0 = one rate;
 * expansions_per_seed_beyond >= expansions_per_seed >= 1).  The first search of a gene copy on a large graph runs for millions of
 * expansions: with one rate its path stayed invisible for as many seeds and every seed of that copy among them explored the copy cold
 * again; beyond the knee the delay grows slowly, the seeds right behind an ordinary search still start without waiting for it.  The
 * result is a function of (seed order, B, the three numbers) only.  (The reference has no such rule: its threads share term_nodes by
 * timing, search.cpp:182-189; B = 1 without a cost term is its one-thread run.) */
int mgta_ctx_set_search_cost_curve(mgta_ctx *, int expansions_per_seed, uint64_t knee_expansions, int expansions_per_seed_beyond);
/* Work memory of the searches.  The reference's node pool, open list and hash maps grow without bound (pool_st.h:43,
 * hash_table_st.h:559-568); here every search slot owns a base arena of 1 << log2_base_nodes nodes (0 = default 12; 7..20) and a search
 * that outgrows it takes further chunks from a device-side pool of pool_bytes (0 = sized from the number of searches in flight), its
 * hash table being re-built at twice the size when half full.  When the pool itself runs dry: an independent search (cache_mode 0 / -1)
 * that has waited in vain is run again by the host with fewer searches at a time (mgta_astar_stats.n_retries); under the ordered-commit
 * window (cache_mode B >= 1) a starved search gives its memory back and starts again IN PLACE -- its slot keeps holding the window, the
 * lowest running seed never yields and has a reserve of its own (an eighth of the memory on top of the pool; with an explicit pool_bytes
 * an eighth OF it) -- so the result stays a function of (seed order, B, cost rate) whatever starved when; only if the lowest seed outgrows
 * the reserve as well does the pass give up, and the batch RESUMES behind its commit frontier (everything that has ended is final; the
 * caches stay) with a larger share in the reserve: 1/2, then 7/8, then one search at a time (mgta_astar_stats.n_resumes, a note on
 * stderr).  Small values exercise these paths on small inputs (tests). */
int mgta_ctx_set_search_arena(mgta_ctx *, int log2_base_nodes, uint64_t pool_bytes);
/* Pages of 2 MB that one array of a search (its nodes, its heap, its hash table) may hold beyond its base arena: 1 .. 1024, 0 = the
 * library's 1024 (the default; ~33 M nodes).  A search that needs one more page ends as a failed side (mgta_astar_stats.n_over_limit).
 * Small values exercise that limit on small inputs (tests); the limit belongs to the context and holds until it is set again. */
int mgta_ctx_set_search_page_limit(mgta_ctx *, int pages);
/* on: the graphs this context loads FROM NOW ON also hold the full multiplicity of every edge (SuccinctDBG::EdgeMultiplicity,
 * succinct_dbg.h:133-147; LoadFromMultiFile(..., need_multiplicity = true), succinct_dbg.cpp:618-694): one byte per edge, min(mult, 255),
 * and for the edges stored as 255 their 16-bit counts in edge order, found by a rank over the 255s (8 bytes per 64 edges) -- the
 * reference's edge_multi_ + large_multi_h_ without the hash table.  What mgta_sdbg_edge_multiplicity and mgta_contig_coverage need.
 * off (default): a load allocates, packs and holds exactly what it did before the switch existed; it is never implied (1 byte per
 * edge is 6.3 GB on the graph of 100 M reads).  A build that runs while the switch is on also keeps the large multiplicities of a
 * kept multi-pass stream (mgta_ctx_keep_stream) beside its records.  A load that cannot keep the counts (mgta_sdbg_load of a stream
 * with records of 255: it is not given the large words; a kept stream built while the switch was off) fails with MGTA_EUNSUPPORTED. */
int mgta_ctx_keep_multiplicity(mgta_ctx *, int on);

/* ------------------------------------------------------------------------------------------------
 * Read ingestion (`megagta buildlib`: SequenceManager::ReadShortReads + WriteBinarySequences, sequence_manager.cpp:109-216,375-410;
 * base codes sequence_package.h:67-69).  `text` = the sequence characters of a batch of reads back to back (the host has inflated the
 * file and cut it into records), read i = text[offsets[i] .. offsets[i+1]).  bin_words receives the batch's share of PREFIX.bin: per
 * read uint32 length + ceil(length / 16) words, 2 bits per base (base j of a word at bits 30 - 2j, zero padded, forward orientation,
 * A0 C1 G2 T3, N -> G, any other byte -> A); *n_words_out = words written (sum of 1 + ceil(len / 16)).
 * ------------------------------------------------------------------------------------------------ */
int mgta_reads_pack_text(mgta_ctx *, const char *text, uint64_t n_bytes, const uint64_t *offsets /* [n_reads + 1] */, uint64_t n_reads,
                         uint32_t *bin_words, uint64_t capacity_words, uint64_t *n_words_out);

/* ------------------------------------------------------------------------------------------------
 * SdBG construction  (replaces CX1::run() with the s2 plug-ins: cx1.h:443-623,
 * s2_lv0_calc_bucket_size / s2_lv1_fill_offset / s2_lv2_extract_substr_ / lv2_cpu_radix_sort_st /
 * output_: cx1_read2sdbg_s2.cpp:252-315,475-677,742-835; lv2_cpu_sort.h:133-150)
 * ------------------------------------------------------------------------------------------------ */

/* One call per bucket range [bucket_begin,bucket_end), ranges ascending and disjoint: the logical
 * edge stream in bucket order, exactly the arguments SdbgWriter::write receives
 * (sdbg_multi_io.h:83-112).  recs[i] = w | last<<4 | tip<<5 | min(mult,255)<<8; `large` holds the
 * full 16-bit multiplicities of the records with mult > 254, `tips` words_per_tip words per tip
 * record, both in stream order.  Buffers are host memory owned by the library, valid during the call. */
typedef int (*mgta_edge_sink)(void *user, int32_t bucket_begin, int32_t bucket_end,
                              const int64_t *bucket_counts /* [bucket_end-bucket_begin][3]: records, large, tips */,
                              const uint16_t *recs, int64_t n_recs, const uint16_t *large, int64_t n_large,
                              const uint32_t *tips, int64_t n_tip_words);

typedef struct mgta_build_stats {
    int32_t k, words_per_key, words_per_tip, n_passes;
    int64_t n_reads, n_kmers;        /* n_kmers = sum max(0,len-k): (k+1)-mer occurrences fed to stage 2 */
    int64_t n_items;                 /* sort items generated */
    int64_t n_edges, n_tips, n_large;
    int64_t n_sort_launches;         /* launches of the dominant kernel (radix scatter) */
    double ms_total;                 /* device time, reads resident -> last record in device memory */
    double ms_count, ms_gen, ms_sort, ms_emit, ms_d2h;
    double ms_sort_scatter;          /* summed duration of the radix scatter launches (HIP events) */
    double ms_local_sort;            /* duration of the segment-local (LDS) finishing sort */
    int64_t n_big_segments;          /* key segments deferred by the tiled LDS sort (sorted alone in LDS, or by global passes) */
    int64_t n_lsd_tiles;             /* LDS tiles whose runs were too long to finish by comparison (LSD passes over every digit) */
    uint64_t bytes_peak;             /* device bytes allocated at the peak */
    double ms_stage1;                /* min_count >= 2: solid-edge counting + mercy edges, before (and not part of) ms_total */
    int64_t n_fused_passes;          /* passes whose key writer placed the keys by the first global sort digit (no scatter launch for it) */
    int64_t n_wide_passes;           /* radix scatter launches that sorted on a digit wider than 8 bits (MGTA_SORT_WIDE) */
    int64_t n_split_levels;          /* most levels any sort of the build split its oversized segments by (a digit per level, from the
                                        top of the bits the global passes left); 0: no segment was too long for an LDS tile */
} mgta_build_stats;

/* a1: packed reads as `buildgraph` holds them — every read REVERSED (cx1_read2sdbg_s1.cpp:97,117),
 * 2 bits/base, base j of word at bits 30-2j (sequence_package.h:126-129), reads concatenated;
 * start_idx[n_reads+1] in bases (sequence_package.h:44).  Copies host -> device. */
int mgta_reads_upload(mgta_ctx *, const uint32_t *packed_seq, uint64_t n_words, const uint64_t *start_idx,
                      uint64_t n_reads, mgta_reads **out);
/* adopt buffers that already live on this device (e.g. torch tensors); not freed by mgta_reads_free */
int mgta_reads_adopt_device(mgta_ctx *, const uint32_t *d_packed_seq, uint64_t n_words,
                            const uint64_t *d_start_idx, uint64_t n_reads, mgta_reads **out);
void mgta_reads_free(mgta_reads *);

/* a2-a7: reads resident -> edge stream.  min_count = 1 (reference `-m 1`): every position solid.  min_count >= 2 runs
 * stage 1 first (cx1_read2sdbg_s1.cpp: (k+1)-mer counting, solid marks; need_mercy adds mercy edges, s2.cpp:106-250).
 * n_short_reads: reads [n_short_reads, n_reads) are assist sequences (always solid, s2.cpp:276).
 * sink may be NULL (records stay on the device, e.g. for timing). */
int mgta_sdbg_build_resident(mgta_ctx *, const mgta_reads *, uint64_t n_short_reads, int k, int min_count,
                             int need_mercy, int32_t bucket_begin, int32_t bucket_end /* this GPU's share of the 65536 buckets */,
                             mgta_edge_sink sink, void *user, mgta_build_stats *stats);
/* (k+1)-mer multiplicity histogram of the last min_count >= 2 build: hist[i] = number of distinct (k+1)-mers seen i times
 * (i = 65535: that or more) — what s1_post_proc accumulates into PREFIX.counting (cx1_read2sdbg_s1.cpp:905-930). */
int mgta_sdbg_last_counting(mgta_ctx *, int64_t *hist /* [65536] */);
/* Passes of the last build on this context whose emitter compacted the info bytes their sort left behind and did not read the keys
 * again (MGTA_EMIT_FUSED); 0 before the first build.  (Not a field of mgta_build_stats: the struct keeps its layout.) */
int mgta_sdbg_last_emit_fused(mgta_ctx *, int64_t *n_passes);
/* Records of the LAST build pass are still on the device: copy them (device -> device) into a caller-owned device
 * buffer (e.g. a torch tensor that is then all-gathered over RCCL).  d_dst = NULL only queries *n_records. */
int mgta_sdbg_export_records_device(mgta_ctx *, void *d_dst, uint64_t capacity_bytes, uint64_t *n_records);
/* convenience: upload + build + free */
int mgta_sdbg_build(mgta_ctx *, const uint32_t *packed_seq, uint64_t n_words, const uint64_t *start_idx,
                    uint64_t n_reads, uint64_t n_short_reads, int k, int min_count, int need_mercy,
                    mgta_edge_sink sink, void *user, mgta_build_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Succinct de Bruijn graph on the device (replaces SuccinctDBG::LoadFromMultiFile/init and the
 * rank/select indexes: succinct_dbg.cpp:595-723, succinct_dbg.h:62-86, rank_and_select.h)
 * ------------------------------------------------------------------------------------------------ */
/* From the logical edge stream (all buckets): recs[size], bucket_items[65536], tip labels. */
int mgta_sdbg_load(mgta_ctx *, int k, const uint16_t *recs, int64_t size, const int64_t *bucket_items,
                   const uint32_t *tips, int64_t n_tip_words, int words_per_tip, mgta_sdbg **out);
/* row f-4 (succinct_dbg.cpp:595-723 without the disk round trip): the graph of the edge stream the LAST
 * mgta_sdbg_build* call of this context left on the device (one pass over all 65536 buckets), read where it lies — the records
 * never visit the host.  MGTA_EINVAL when there is no such stream (no build yet, a bucket sub-range, several passes). */
int mgta_sdbg_load_resident(mgta_ctx *, mgta_sdbg **out);
/* mgta_sdbg_load with the stream's large multiplicities (the sink's `large`: one word per record of 255, in stream order), for a
 * context that keeps multiplicities (mgta_ctx_keep_multiplicity; without the switch the words are ignored).  MGTA_EINVAL when n_large
 * is not the number of records stored as 255. */
int mgta_sdbg_load_large(mgta_ctx *, int k, const uint16_t *recs, int64_t size, const int64_t *bucket_items, const uint32_t *tips,
                         int64_t n_tip_words, int words_per_tip, const uint16_t *large, int64_t n_large, mgta_sdbg **out);
/* The same load from the files `buildgraph` wrote: PREFIX.sdbg_info + PREFIX.sdbg.0 .. N-1 (SdbgReader + LoadFromMultiFile,
 * sdbg_multi_io.h:201-417, succinct_dbg.cpp:595-723).  The host maps the files and copies them to the device; the variable-length records
 * are parsed there, one bucket per lane.  What every rank of a multi-GPU search and every one-shot `megagta denovo|search` calls.
 * The records are never on the device all at once: they are decoded range by range (at most MGTA_LOAD_RANGE_RECORDS of them, default 2^32 =
 * 8 GB) and the 64-edge lines each range completes are packed at once, so the peak is the graph (2 B per edge) + its rank prefix sums
 * (1.2 B per edge) + one range -- the 63 G-edge graph of a 1 G-read set loads into 288 GB (round 4 held all records beside the lines). */
int mgta_sdbg_load_files(mgta_ctx *, const char *prefix, mgta_sdbg **out);
void mgta_sdbg_free(mgta_sdbg *);
int64_t mgta_sdbg_size(const mgta_sdbg *);
int mgta_sdbg_k(const mgta_sdbg *);                 /* the graph's k (node length), -1 for NULL */
/* batched navigation (test hook + building block of the search): for each edge id the valid
 * outgoing edges in the reference's order (descending id) [succinct_dbg.cpp:78-97];
 * outdeg[i] = -1 for an invalid edge.  out4 = n x 4 int64 (unused slots -1). Host pointers. */
int mgta_sdbg_outgoing(mgta_sdbg *, const int64_t *edges, int64_t n, int64_t *out4, int8_t *outdeg);
/* Navigation probe (test hook): operation `op` on n argument tuples, one device lane per tuple, each answered by the very device
 * function the kernels of this library walk the graph with (csrc/graph.hpp, csrc/graph_nav.hpp).  Host pointers.
 *
 *   op                          arg0      arg1     arg2    out (int64 per tuple)             defined for
 *   MGTA_NAV_RANK_LAST          pos       -        -       1: `last` bits in [0..pos]        pos in [-1, size)
 *   MGTA_NAV_RANK_TIP           pos       -        -       1: tip bits in [0..pos]           pos in [0, size)  (no early-out for -1)
 *   MGTA_NAV_RANK_W             pos       c        -       1: edges with W == c in [0..pos]  c in 1..4 (plain symbols), pos in [-1, size)
 *   MGTA_NAV_SELECT_LAST        r         -        -       1: position of the r-th one,      r in [-1, total]: -1 -> -1, total -> size
 *   MGTA_NAV_SELECT_W           r         c        -       1:   0-based                      c in 1..4, r in [-1, total of c]
 *   MGTA_NAV_FORWARD            edge      -        -       1: Forward (size / -1 past the    any edge with W != 0 (tips included);
 *                                                             ends of `last`)                   W == 0: MGTA_NAV_UNDEFINED
 *   MGTA_NAV_BACKWARD           edge      -        -       1: Backward                       any edge of a node that is no tip (a tip has no edge
 *                                                                                               into it); a tip: MGTA_NAV_UNDEFINED
 *   MGTA_NAV_LAST_INDEX         edge      -        -       1: the node's last edge           any edge (size when no `last` bit follows)
 *   MGTA_NAV_OUTGOING           edge      -        -       5: degree, 4 x (id << 4 |         any edge; degree -1 for one that is not valid
 *                                                             multi1 << 3 | label), -1 unused
 *   MGTA_NAV_INCOMING           edge      -        -       5: degree, 4 ids, -1 unused       any edge; degree -1 for one that is not valid
 *   MGTA_NAV_PREV_SIMPLE        edge      -        -       1: PrevSimplePathEdge or -1       any edge (-1 for one that is not valid)
 *   MGTA_NAV_NEXT_SIMPLE        edge      -        -       1: NextSimplePathEdge or -1       any edge (-1 for one that is not valid)
 *   MGTA_NAV_REVERSE_COMPLEMENT edge      -        -       1: its edge or -1                 any edge (-1 for one that is not valid), k <= 255
 *   MGTA_NAV_LABEL              edge      -        -       1: k; out_sym: k symbols 1..4     any edge, k <= 255
 *   MGTA_NAV_OUT_FD             edge      r        hint    29, see below                     any edge; hint -1 ("none": the descriptor is read
 *                                                                                               from the edge's own line) or a line < ceil(size / 64)
 *
 * MGTA_NAV_OUT_FD walks one step of the forward-descriptor chain of the search kernel (g_out_all_fd, g_out_nth_fd): a descriptor (r, hint) of
 * an edge is the Select argument of its Forward and a line at or before the line of that `last` bit.  out[0] = out-degree (min(4, .), -1 for
 * an edge that is not valid and has no descriptor), out[1..4] = the packed out-edges, out[5..8] / out[9..12] = r / hint of their own
 * descriptors (hint -1 = none: the edge lies in the line before the target line, r is then 0), then g_out_nth_fd for n = 0..3:
 * out[13..16] = its degree, out[17..20] = its edge, out[21..24] / out[25..28] = r / hint.  Slots the device function leaves alone (n >= degree)
 * hold MGTA_NAV_UNTOUCHED.  A descriptor whose hint line lies behind the bit it looks for: out[0] = MGTA_NAV_UNDEFINED.
 *
 * Ids, positions, ranks and symbols outside the ranges above: MGTA_EINVAL before anything is launched, `out` untouched.  What only the graph
 * knows is checked on the device before the function is called and answered with MGTA_NAV_UNDEFINED in out[0]; besides the two cases in the
 * table that is an edge whose Forward / Backward leaves [0, size) under OUTGOING / NEXT_SIMPLE / INCOMING / PREV_SIMPLE, which no stream of a
 * build contains.  The rank and select operations hold for ANY records; the others need a stream a build produced (as every kernel of the
 * library does).  An empty graph answers the few tuples in range (rank of -1, select of -1 and 0) without a launch. */
enum {
    MGTA_NAV_RANK_LAST = 0, MGTA_NAV_RANK_TIP = 1, MGTA_NAV_RANK_W = 2, MGTA_NAV_SELECT_LAST = 3, MGTA_NAV_SELECT_W = 4, MGTA_NAV_FORWARD = 5,
    MGTA_NAV_BACKWARD = 6, MGTA_NAV_LAST_INDEX = 7, MGTA_NAV_OUTGOING = 8, MGTA_NAV_INCOMING = 9, MGTA_NAV_PREV_SIMPLE = 10,
    MGTA_NAV_NEXT_SIMPLE = 11, MGTA_NAV_REVERSE_COMPLEMENT = 12, MGTA_NAV_LABEL = 13, MGTA_NAV_OUT_FD = 14
};
#define MGTA_NAV_UNTOUCHED (-2)
#define MGTA_NAV_UNDEFINED (-3)
int mgta_sdbg_navigate(mgta_sdbg *, int op, const int64_t *arg0, const int64_t *arg1, const int64_t *arg2, int64_t n, int64_t *out,
                       uint8_t *out_sym /* n x k, MGTA_NAV_LABEL only */);
/* batched IndexBinarySearchEdge over (k+1)-symbol strings (symbols 1..4) [succinct_dbg.cpp:427-549]. */
/* the validity bits as they are now (SuccinctDBG::invalid_, succinct_dbg.h:117-131): bit e of words[e / 64]; ceil(size / 64) words.
 * Set for tips and $ edges after a load, and for everything `mgta_denovo` removed. */
int mgta_sdbg_invalid_bits(mgta_sdbg *, uint64_t *words);
int mgta_sdbg_index_edges(mgta_sdbg *, const uint8_t *seqs /* n x (k+1) */, int64_t n, int64_t *edge_ids);

/* batched EdgeMultiplicity (succinct_dbg.h:133-147): the full count of the (k+1)-mer of each edge, as the stream gave it (tips and $
 * edges have one too).  MGTA_EINVAL for a graph loaded without mgta_ctx_keep_multiplicity and for an id outside [0, size). */
int mgta_sdbg_edge_multiplicity(mgta_sdbg *, const int64_t *edge_ids, int64_t n, uint16_t *mult);

/* ------------------------------------------------------------------------------------------------
 * Per-contig k-mer coverage and abundance (the `kmer_coverage` step at the end of the reference's bin/post_proc.sh:113-118, which
 * recounts from the reads what the graph already holds).  Contig i = seqs[offsets[i] .. offsets[i + 1]), letters in any case.  A
 * WINDOW is a (k+1)-mer of the contig at offset p = 0 .. len - k - 1; its coverage is the multiplicity of the edge
 * IndexBinarySearchEdge (succinct_dbg.cpp:530-549) finds for it, and 0 when there is none or when the window holds a letter other
 * than A, C, G, T (no N -> G folding: an N was never counted).  Only the string as given is looked up (the graph holds both strands
 * with equal counts).  per_contig[i]: see the struct; median = the LOWER median over all windows, zeros included (element
 * (n_windows - 1) / 2 of the ascending order); the mean is sum / n_windows, formed by the caller.  per_window (may be NULL): the
 * coverages back to back, contig by contig (prefix sums of n_windows index it).  abundance (may be NULL) [65536]: abundance[m] =
 * number of DISTINCT edges of multiplicity m that the windows of THIS CALL found (an edge reached from three contigs counts once;
 * index 65535 = that or more).  One call = one set of contigs: the marks live for one call, so a gene's contigs go in one call (the
 * library cuts its own work into batches that fit the per-window scratch and keeps the marks across them;
 * mgta_ctx_set_coverage_batch sets the windows per batch, 0 = the library's 2^29: small values exercise that on small inputs).
 * Every output is a function of (graph, contigs) only.  MGTA_EINVAL for a graph loaded without mgta_ctx_keep_multiplicity.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_contig_cov {
    uint64_t sum;                    /* sum of the window coverages */
    uint32_t len, n_windows;         /* n_windows = max(0, len - k); 0 -> every other field but len is 0 */
    uint32_t n_covered;              /* windows with coverage > 0 */
    uint32_t min, max, median;
} mgta_contig_cov;
typedef struct mgta_coverage_stats {
    int64_t n_contigs, n_windows;
    int64_t n_walked;                /* windows whose edge was found by one forward step from the window before */
    int64_t n_index_searches;        /* windows that needed IndexBinarySearchEdge: the first of a contig, and the first after the contig left the graph */
    int64_t n_batches;
    int64_t groups_per_cu;           /* lane groups of 8 (one contig, one dependent line in flight each) a CU holds at once in the walk
                                      * kernel: 32 per workgroup x the workgroups its registers allow (asked of the runtime) */
    double ms_kernel;                /* walk + statistics kernels (HIP events) */
    double ms_walk;                  /* the walk kernel alone */
} mgta_coverage_stats;
int mgta_ctx_set_coverage_batch(mgta_ctx *, uint64_t windows);
int mgta_contig_coverage(mgta_sdbg *, const char *seqs, const uint64_t *offsets /* [n + 1] */, int64_t n, mgta_contig_cov *per_contig,
                         uint16_t *per_window /* optional */, int64_t *abundance /* optional, [65536] */, mgta_coverage_stats *stats /* optional */);

/* ------------------------------------------------------------------------------------------------
 * Window-shared coverage: a coverage that ADDS UP over sets of contigs (what per-cluster and per-taxon abundance are summed from;
 * mgta_contig_coverage credits an edge's full multiplicity to every contig that walks over it, so its numbers cannot be summed over
 * redundant contigs).  Contigs, windows and the edge of a window are exactly those of mgta_contig_coverage: only the string as given
 * is looked up, a window with a letter other than A, C, G, T has no edge, there is no N -> G folding.  With
 *   edge(i, p)  the edge of window p of contig i, or none,
 *   mult(e)     its multiplicity, capped at 65535,
 *   share(e)    the number of windows OF THIS CALL whose edge is e (occurrences, not distinct contigs: a contig that holds the same
 *               (k+1)-mer twice contributes 2, and both of its windows carry that share),
 *   mass(i, p)  floor(mult(e) * 65536 / share(e)), an unsigned Q16 number; 0 for a window without an edge,
 * per_contig[i].mass = the sum of mass(i, p) over its windows.  per_window_share (may be NULL): the shares back to back, contig by
 * contig, as per_window of the coverage call, 0 = no edge; per_window (may be NULL): the multiplicities, laid out the same way.
 * Each edge loses less than share(e) units to the floor, so with total_mult = the sum of mult over the DISTINCT edges of the call
 *   65536 * total_mult - (covered windows of the call)  <=  sum of per_contig[i].mass  <=  65536 * total_mult.
 * Every output and every stats field but ms_* and n_batches is a function of (graph, contigs) only; the order of the contigs in the
 * call changes nothing but the order of the records.  One call = one set of contigs: shares are counted over the whole call,
 * whatever the batches the library cuts its walk into (mgta_ctx_set_coverage_batch moves no output).  The counts live in a table
 * keyed by the edge id and sized by the windows of the call, never by the graph; mgta_ctx_set_share_hash_bits keeps only the low
 * `bits` bits of its hash (1 .. 64, default 64): with a few bits nearly every key collides and the outputs must not move -- a switch
 * for tests, like mgta_ctx_set_derep_hash_bits.  Limits: n < 2^31 contigs and fewer than 2^32 windows in the call (a share fits 32
 * bits); beyond either the call returns MGTA_EINVAL, says which, and writes nothing.  Device memory: 8 bytes per window of a batch,
 * 4 bytes per window of the call and 16 bytes per table slot (2 to 4 slots per min(windows, edges of the graph)), accounted like
 * every other buffer of the context; what does not fit is MGTA_ENOMEM, nothing is truncated.  MGTA_EINVAL for a graph loaded
 * without mgta_ctx_keep_multiplicity.  n = 0: MGTA_OK, stats all zero.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_contig_share {
    uint64_t mass;                   /* sum of the window masses, Q16 */
    uint32_t len, n_windows;         /* as in mgta_contig_cov */
    uint32_t n_covered;              /* windows with an edge of multiplicity > 0 */
    uint32_t n_unique;               /* covered windows whose edge no other window of the call has (share 1) */
    uint32_t max_share;              /* largest share over the covered windows; 0 when nothing is covered */
    uint32_t reserved_;              /* 0 */
} mgta_contig_share;
typedef struct mgta_share_stats {
    int64_t n_contigs, n_windows;
    int64_t n_walked, n_index_searches;   /* as in mgta_coverage_stats, and equal to them on the same input: the walk is done once */
    int64_t n_batches;
    int64_t n_covered;               /* covered windows of the call */
    int64_t n_distinct_edges;        /* distinct edges the windows of the call found */
    uint64_t total_mult;             /* sum of mult over those distinct edges */
    uint64_t total_mass;             /* sum of per_contig[i].mass */
    uint64_t table_slots;            /* slots of the count table */
    uint64_t table_bytes;            /* its bytes (key + count and multiplicity per slot) */
    uint64_t window_bytes;           /* bytes kept per call beside it: the slot number of every window */
    double ms_walk;                  /* the walk kernel (HIP events) */
    double ms_count;                 /* edge ids -> table, batch by batch */
    double ms_share;                 /* table -> masses and per-contig records */
    double ms_total;                 /* the three together */
} mgta_share_stats;
int mgta_ctx_set_share_hash_bits(mgta_ctx *, int bits);   /* 1..64, default 64 */
int mgta_contig_share_coverage(mgta_sdbg *, const char *seqs, const uint64_t *offsets /* [n + 1] */, int64_t n, mgta_contig_share *per_contig,
                               uint32_t *per_window_share /* optional */, uint16_t *per_window /* optional */, mgta_share_stats *stats /* optional */);

/* ------------------------------------------------------------------------------------------------
 * Read recruitment (the `-m proc_match_reads.fa` output of the same `kmer_coverage` command line, bin/post_proc.sh:113-118): which reads
 * of the library share a (k+1)-mer with a set of contigs.  Contigs as in mgta_contig_coverage; reads as uploaded for the build
 * (reads_reversed as in mgta_findstart: one upload serves buildgraph, findstart and this).  Every WINDOW of a contig, as given AND
 * reverse-complemented, marks the edge IndexBinarySearchEdge finds for it: nothing when there is none, nothing when it holds a letter
 * other than A, C, G, T (no N -> G folding).  Window p of read r HITS iff the edge found for its k + 1 bases is marked (the validity
 * bit is not looked at, as for the coverage windows).  hit_windows[r] (may be NULL) = the number of hitting windows; bit r of
 * match_bits[r / 64] = at least one window of read r hits.  A read shorter than k + 1 has no windows.  Only the reads
 * [0, n_short_reads) are scanned and have a bit (the rest are the assist sequences of a multi-k library).  On a `-m 1` graph of these
 * very reads a hit is plain equality of (k+1)-mers on either strand.  With hit_windows = NULL the walk of a read ends at its first
 * hit.  Works on any loaded graph (no multiplicities needed, none allocated); uses the graph's mark bits, cleared at the start of the
 * call like mgta_contig_coverage's, so the two never see each other's marks.  One call = one set of contigs.  n = 0 or
 * n_short_reads = 0: match_bits all zero, stats all zero.  Every output and every stats field but ms_* is a function of (graph,
 * contigs, reads) only.  MGTA_EINVAL: NULL graph / reads / match_bits, n_short_reads > the reads uploaded, graph and reads of
 * different contexts.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_match_stats {
    int64_t n_contigs, n_contig_windows;   /* windows of the contigs as given (the reverse complements double the work, not this number) */
    int64_t n_marked_edges;                /* distinct edges the contigs turned on, both strands together */
    int64_t n_reads, n_read_windows;       /* sum max(0, len - k) over the reads scanned */
    int64_t n_walked, n_index_searches;    /* read windows found by one forward step / by IndexBinarySearchEdge */
    int64_t n_matched_reads;
    int64_t groups_per_cu;                 /* as in mgta_coverage_stats, for the read walk */
    double ms_mark, ms_walk;               /* HIP events */
} mgta_match_stats;
int mgta_reads_match_contigs(mgta_sdbg *, const mgta_reads *reads, int reads_reversed, uint64_t n_short_reads,
                             const char *seqs, const uint64_t *offsets /* [n + 1] */, int64_t n,
                             uint64_t *match_bits /* [ceil(n_short_reads / 64)], bit r of word r / 64 */,
                             uint32_t *hit_windows /* optional [n_short_reads] */, mgta_match_stats *stats /* optional */);

/* ------------------------------------------------------------------------------------------------
 * Per-library coverage: how many read windows of every library (sample) lie on the windows of a set of contigs, counted from the
 * READS.  (The graph's multiplicities are pooled over the read set and, in a multi-k run, include the contigs of the earlier k: they
 * cannot tell libraries apart.)  Any loaded graph serves: no multiplicities are needed and none are allocated.
 * Libraries: library s holds the reads [lib_end[s - 1], lib_end[s]) of `reads`, lib_end[-1] = 0; lib_end must not descend (an empty
 * library is legal) and lib_end[n_libs - 1] <= the reads uploaded; the reads at and behind lib_end[n_libs - 1] (the assist sequences
 * of a multi-k library) are not scanned.  reads_reversed as in mgta_reads_match_contigs.
 * Contigs, windows and edge(w) are exactly those of mgta_contig_coverage: only the string as given is looked up, a window with a letter
 * other than A, C, G, T in either case has no edge, there is no N -> G folding.  With
 *   share(e)     the number of windows OF THIS CALL whose edge is e, as in mgta_contig_share_coverage (occurrences are counted),
 *   count(w, s)  the number of windows v of the reads of library s, each read taken as sequenced, with v = w or v = revcomp(w) as
 *                strings; ONE read window counts once, also when w is its own reverse complement; 0 when w has no edge.  (A read
 *                window is found by its edge, so the graph has to hold it: every graph built from these reads holds both strands of
 *                all their windows.  The validity bit of an edge is not looked at.)
 *   mass[i * n_libs + s] = the sum over the windows p of contig i of floor(count(w_ip, s) * 65536 / share(edge(w_ip))), Q16.
 * Counts are 64-bit; there is no cap.  per_contig (may be NULL): len, n_windows as in mgta_contig_cov; n_covered = windows with
 * count > 0 in at least one library; n_unique, max_share over those as in mgta_contig_share; mass = the sum of the contig's masses
 * over the libraries.  per_window_count (may be NULL): count(w, s) window-major in the window order of mgta_contig_coverage's
 * per_window, the library index minor.  per_window_share (may be NULL): share(edge(w)), 0 = no edge.  lib_hit_windows (may be NULL):
 * per library, the read windows that were credited to at least one key.
 * Consequences.  On a `-m 1` graph of exactly these reads the sum of count(w, s) over the libraries is the uncapped multiplicity of
 * edge(w) (twice that where w is its own reverse complement: the graph counts such a read window on both strands), and wherever the
 * multiplicity is below 65535 one library over all reads gives mass[i] = mgta_contig_share_coverage's mass bit for bit.  In general
 * the sum of mass[i][s] over s differs from the pooled mass by less than n_libs units per covered window.
 * Every output and every stats field but ms_* and n_batches is a function of (graph, reads, lib_end, contigs): neither
 * mgta_ctx_set_coverage_batch nor mgta_ctx_set_share_hash_bits nor the order of the reads inside a library moves any of them.  Uses
 * the graph's mark bits, cleared at the start of the call.  Limits: 1 <= n_libs <= 256, n < 2^31 contigs, fewer than 2^32 windows in
 * the call, k + 1 <= 128; beyond any the call returns MGTA_EINVAL, names the limit and writes nothing.  MGTA_EINVAL too for a NULL
 * graph, reads, lib_end or mass and for a graph and reads of different contexts.  Device memory: 16 bytes per window of a batch (the
 * edge ids of both strands), 8 bytes per window of the call (two slot numbers), 16 bytes per table slot (2 to 4 slots per key; the
 * keys are the distinct edges of both strands) and 8 * n_libs bytes per key, accounted like every other buffer of the context; what
 * does not fit is MGTA_ENOMEM, nothing is truncated.  n = 0: MGTA_OK, stats all zero.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_sample_cov_stats {
    int64_t n_contigs, n_windows;
    int64_t n_walked, n_index_searches;   /* contig windows of BOTH strands found by one forward step / by IndexBinarySearchEdge */
    int64_t n_batches;
    int64_t n_covered;               /* covered windows of the call */
    int64_t n_keys;                  /* distinct edges of the contig windows, both strands */
    int64_t n_libs;
    int64_t n_reads, n_read_windows; /* reads scanned = lib_end[n_libs - 1]; sum max(0, len - k) over them */
    int64_t n_read_walked, n_read_index_searches;
    int64_t n_hit_windows;           /* read windows credited to a key = the sum of lib_hit_windows */
    int64_t groups_per_cu;           /* as in mgta_coverage_stats, for the read scan */
    uint64_t total_mass;             /* sum of per_contig[i].mass */
    uint64_t table_slots;            /* slots of the key table */
    uint64_t table_bytes;            /* its bytes (key, share and key number per slot) */
    uint64_t window_bytes;           /* the two slot numbers of every window */
    uint64_t count_bytes;            /* the rows of counts: (n_keys + 1) * n_libs * 8 */
    double ms_mark;                  /* contig walks, table and key numbers (HIP events) */
    double ms_scan;                  /* the read scan */
    double ms_mass;                  /* counts -> masses and per-contig records */
    double ms_total;                 /* the three together */
} mgta_sample_cov_stats;
int mgta_contig_sample_coverage(mgta_sdbg *, const mgta_reads *reads, int reads_reversed, const uint64_t *lib_end /* [n_libs] */, int n_libs,
                                const char *seqs, const uint64_t *offsets /* [n + 1] */, int64_t n, uint64_t *mass /* [n * n_libs], Q16 */,
                                mgta_contig_share *per_contig /* optional [n] */, uint64_t *per_window_count /* optional [windows * n_libs] */,
                                uint32_t *per_window_share /* optional [windows] */, uint64_t *lib_hit_windows /* optional [n_libs] */,
                                mgta_sample_cov_stats *stats /* optional */);

/* ------------------------------------------------------------------------------------------------
 * Pileup: the reads placed on the contigs of ONE set (a gene's FASTA), per-base depth in the contig's strand, the reads that fit a
 * contig end to end, the positions where the reads disagree with it.  The rule is this project's own; no mapper is consulted.  Any
 * loaded graph serves (no multiplicities needed); the reads [0, n_short_reads) are scanned; reads_reversed as in
 * mgta_reads_match_contigs.
 *   Read     s = the packed bases as sequenced (an N of the input is a G); s^0 = s, s^1 = revcomp(s), L its length.
 *   Contig   c_i = its letters folded to upper case; a letter other than A, C, G, T equals no base, a window that holds one is no key.
 *   Anchor   (o, p, i, q): window p of s^o and window q of c_i are the same k + 1 letters and that (k+1)-mer has an edge in the graph
 *            (found by the read's walk: a graph built from these reads holds both strands of all their windows; the validity bit of
 *            an edge is not looked at).  On any other graph a window without an edge anchors nothing.
 *   Candidate  a distinct (i, o, d) with at least one anchor on the diagonal d = q - p (d may be negative, d + L may exceed len_i).
 *            votes = its anchors (distinct p); overlap = the positions x in [max(0, d), min(len_i, d + L)), n_ov their number; n_mm =
 *            the number of x with c_i[x] != s^o[x - d]; score = n_ov - 2 * n_mm.
 *   Pass     votes >= min_anchors (default 1), n_ov >= min_overlap (default k + 1), n_mm * 1000 <= max_mismatch_permille * n_ov
 *            (default 50).  A parameter given as 0 takes its default.
 *   Placements of a read = ALL passing candidates with the read's highest score; ties are all placed.  Two equal contigs give two
 *            placements, two diagonals of one contig (an internal repeat) are two candidates, and a read equal to its own reverse
 *            complement has the candidates o = 0 and o = 1 and may be placed on both: nothing is special-cased.
 *   Pile     every placement adds 1 to counts[(offsets[i] + x) * 4 + b] for every x of its overlap, b = s^o[x - d] (A C G T = 0 1 2 3);
 *            a read with exactly one placement also adds 1 to uniq[offsets[i] + x].  depth = A + C + G + T.
 * per_contig (may be NULL): len; n_covered = positions with depth > 0; min_depth, max_depth over all positions (0 for len 0);
 * n_placed = placements on the contig, n_unique = those of reads placed once; depth_sum; mismatch_sum = the sum of n_mm over the
 * placements.  per_read (may be NULL): the lowest placement by (contig, orient, diag) with its score and n_mismatch (which all ties
 * share the score of), n_placed = the number of placements; {0, -1, 0, 0, 0, 0} for a read without one.  No output and no stats field
 * but ms_* depends on the order of anything: all sums are integers, the choice is a maximum over a total order; neither
 * mgta_ctx_set_pileup_chunk nor mgta_ctx_set_share_hash_bits moves any.  Uses the graph's mark bits, cleared at the start of the call.
 * Limits, each MGTA_EINVAL naming it with nothing written: k + 1 <= 128, n < 2^31, offsets[0] = 0 and offsets[n] < 2^32, reads of at
 * most 65535 bases, no negative parameter, permille <= 1000.  MGTA_EINVAL too for a NULL graph, reads or counts and for a graph and
 * reads of different contexts.  All contigs of the call are resident at once (the best-hit rule needs them): 2 bytes per letter, 8 per
 * window for the two slot numbers, 16 per table slot, 8 per occurrence (at most 2 per window), 20 per letter for counts and uniq, one
 * 32-bit word per window of the longest read for every group of lanes in flight; what does not fit is MGTA_ENOMEM, nothing is
 * truncated and there is no cap on candidates.  n = 0 or n_short_reads = 0: MGTA_OK, counts and stats zero.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_pileup_params { int32_t min_anchors, min_overlap, max_mismatch_permille; } mgta_pileup_params;  /* 0 = the default of each */
typedef struct mgta_contig_pileup { uint32_t len, n_covered, min_depth, max_depth; uint64_t n_placed, n_unique, depth_sum, mismatch_sum; } mgta_contig_pileup;
typedef struct mgta_read_place { int32_t score, contig, diag, orient; uint32_t n_placed, n_mismatch; } mgta_read_place;
typedef struct mgta_pileup_stats {
    int64_t n_contigs, n_contig_letters, n_contig_windows;
    int64_t n_keys;                  /* distinct edges of the contig windows, both strands */
    int64_t n_occurrences;           /* entries of the occurrence index: (contig, window, strand) per key */
    int64_t n_reads, n_read_windows; /* reads scanned; sum max(0, len - k) over them */
    int64_t n_hit_windows;           /* read windows whose edge is a key */
    int64_t n_read_walked, n_read_index_searches;
    int64_t n_reads_with_candidate, n_candidates;
    int64_t n_verified;              /* anchors that start a run on their diagonal: each is compared along its whole overlap */
    int64_t n_reads_placed, n_reads_multi, n_placements;
    int64_t n_bases_piled;           /* the sum of all counts */
    int64_t groups_per_cu;           /* as in mgta_coverage_stats, for the read scan */
    uint64_t peak_bytes;             /* most device bytes of the call's own buffers */
    double ms_keys, ms_index, ms_scan, ms_records, ms_total;   /* HIP events */
} mgta_pileup_stats;
int mgta_reads_pileup(mgta_sdbg *, const mgta_reads *reads, int reads_reversed, uint64_t n_short_reads, const char *seqs,
                      const uint64_t *offsets /* [n + 1] */, int64_t n, const mgta_pileup_params *params /* NULL = defaults */,
                      uint32_t *counts /* [offsets[n] * 4], A C G T */, uint32_t *uniq /* [offsets[n]] or NULL */,
                      mgta_contig_pileup *per_contig /* [n] or NULL */, mgta_read_place *per_read /* [n_short_reads] or NULL */,
                      mgta_pileup_stats *stats /* or NULL */);
int mgta_ctx_set_pileup_chunk(mgta_ctx *, uint32_t reads);   /* reads per queue grab, 0 = the library's; a switch for tests, moves no output */

/* ------------------------------------------------------------------------------------------------
 * Gapped pileup: mgta_reads_pileup with reads placed across ONE insertion or deletion.  An entry of its own; mgta_reads_pileup is
 * what it was.  Read, contig, anchor, candidate (i, o, d), votes, n_ov, n_mm, the pass test and the pile are those of
 * mgta_reads_pileup, word for word.  The rule is this project's own.
 *   Parameters  the three of mgta_reads_pileup, and max_gap G (default 32, at most 255), gap_open (default 4), gap_extend (default 1),
 *            0 <= gap_extend <= gap_open <= 255.  A parameter given as 0 takes its default.  Parameters of the rule, not measurements.
 *   One-gap candidate  a distinct (i, o, d1, d2), d1 != d2, g = |d2 - d1| <= G.  P1 = the anchor windows p of s^o on (i, o, d1), P2 those
 *            on (i, o, d2).  ins = max(0, d1 - d2) read letters have no partner, del = max(0, d2 - d1) contig letters are skipped.
 *            A breakpoint b is legal iff min(P1) + k + 1 <= b and b + ins <= max(P2); the candidate exists iff a legal b exists.
 *            Under b the read letters p in [0, b) lie at x = p + d1, the letters p in [b + ins, L) at x = p + d2; a pair with x
 *            outside [0, len_i) does not count.  n_ov = the pairs, n_mm = those that differ (n_ov is the same for every legal b).
 *            votes = |{p in P1 : p + k + 1 <= b}| + |{p in P2 : p >= b + ins}|.
 *            score = n_ov - 2 * n_mm - (gap_open + gap_extend * g).
 *            The candidate's b = the legal b of the highest score, the lowest such b on a tie: a gap inside a repeat is left-aligned.
 *            pos = b + d1 = the first contig position right of the gap's left side: the first deleted letter, or the letter in front
 *            of which the insertion lies.  (d1, d2) and (d2, d1) are two candidates.
 *   Pass     the three tests of mgta_reads_pileup on the candidate's votes, n_ov and n_mm (both sides have an anchor by construction).
 *   Placements of a read = ALL passing candidates, gapped and ungapped (d2 = d1, score = n_ov - 2 * n_mm) alike, with the read's
 *            highest score; ties are all placed.  "The lowest" is by (contig, orient, d1, d2).
 *   Pile     every placement piles its pairs into counts / uniq as mgta_reads_pileup does; the deleted contig positions get nothing
 *            from it, the inserted read letters go nowhere.
 * per_contig as in mgta_reads_pileup over all placements.  per_read (may be NULL): mgta_gap_place = mgta_read_place of the lowest
 * placement (diag = d1) with diag2 = d2 and brk = b; an ungapped placement has diag2 = diag and brk = 0; {0, -1, 0, 0, 0, 0, 0, 0}
 * for a read without one.  gaps[gap_cap]: one mgta_gap_rec per gapped placement -- read, contig, pos, len = d2 - d1 (> 0 letters
 * deleted, < 0 inserted), brk, orient, unique = 1 iff it is the read's only placement -- sorted by (contig, pos, len, read, orient,
 * d1 = pos - brk) before the call returns: no device order shows.  More records than gap_cap: MGTA_EINVAL, the message names the
 * count needed, stats->n_gap_placements holds it and nothing else is written (gaps may be NULL with gap_cap = 0).
 * Stats: the fields of mgta_pileup_stats -- n_candidates and n_verified count the ungapped candidates; n_reads_placed, n_reads_multi,
 * n_placements and n_bases_piled all placements -- then n_gap_candidates = one-gap candidates, n_gap_passing = those that pass,
 * n_reads_gapped = reads whose per_read record is gapped, n_gap_placements, n_inserted / n_deleted = the letters of the gapped
 * placements' gaps.  All but ms_*, peak_bytes, groups_per_cu, n_read_walked and n_read_index_searches are functions of the inputs
 * alone; neither mgta_ctx_set_pileup_chunk nor mgta_ctx_set_share_hash_bits moves any.
 * Limits: those of mgta_reads_pileup, and max_gap in [0, 255], 0 <= gap_extend <= gap_open <= 255 (after the defaults); each
 * MGTA_EINVAL naming the limit with nothing written.  Memory: that of mgta_reads_pileup, and per group of lanes in flight a list of the
 * read's diagonals of 24 bytes each, sized for the most a read of the call can have: (windows of the longest read) * (the most
 * occurrences of one key); fewer groups run where the rows would pass 1 GiB and what does not fit is MGTA_ENOMEM: no cap on
 * candidates.  n = 0 or n_short_reads = 0: MGTA_OK, everything zero.
 * What it is not: one gap per read; a gap nearer than k + 1 letters to an end of the read has no anchor on its short side and the read
 * stays with the ungapped rule; no quality values; mgta_reads_phase takes no allele from a gapped placement.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_gapped_params { int32_t min_anchors, min_overlap, max_mismatch_permille, max_gap, gap_open, gap_extend; } mgta_gapped_params;
typedef struct mgta_gap_place { int32_t score, contig, diag, orient; uint32_t n_placed, n_mismatch; int32_t diag2; uint32_t brk; } mgta_gap_place;
typedef struct mgta_gap_rec { uint64_t read; int32_t contig; uint32_t pos; int32_t len; uint32_t brk; int32_t orient, unique; } mgta_gap_rec;
typedef struct mgta_gapped_stats {
    int64_t n_contigs, n_contig_letters, n_contig_windows, n_keys, n_occurrences, n_reads, n_read_windows, n_hit_windows;
    int64_t n_read_walked, n_read_index_searches, n_reads_with_candidate, n_candidates, n_verified;
    int64_t n_reads_placed, n_reads_multi, n_placements, n_bases_piled, groups_per_cu;
    uint64_t peak_bytes;
    double ms_keys, ms_index, ms_scan, ms_records, ms_total;   /* up to here mgta_pileup_stats */
    int64_t n_gap_candidates;        /* one-gap candidates: (i, o, d1, d2) with a legal breakpoint */
    int64_t n_gap_passing;           /* those that pass the three tests */
    int64_t n_reads_gapped;          /* reads whose per_read record (the lowest placement) is gapped */
    int64_t n_gap_placements;        /* = the gap records */
    int64_t n_inserted, n_deleted;   /* letters, summed over the gapped placements */
    int64_t diag_list_entries;       /* entries of one group's diagonal list (a function of the inputs too) */
} mgta_gapped_stats;
int mgta_reads_pileup_gapped(mgta_sdbg *, const mgta_reads *reads, int reads_reversed, uint64_t n_short_reads, const char *seqs,
                             const uint64_t *offsets /* [n + 1] */, int64_t n, const mgta_gapped_params *params /* NULL = defaults */,
                             uint32_t *counts /* [offsets[n] * 4] */, uint32_t *uniq /* [offsets[n]] or NULL */,
                             mgta_contig_pileup *per_contig /* [n] or NULL */, mgta_gap_place *per_read /* [n_short_reads] or NULL */,
                             mgta_gap_rec *gaps /* [gap_cap] */, uint64_t gap_cap, mgta_gapped_stats *stats /* or NULL */);

/* ------------------------------------------------------------------------------------------------
 * Phase: which alleles of the variant positions (sites) of a contig travel together on one fragment -- a read, or two mates of a
 * paired library.  The rule is this project's own; it counts, it reconstructs no haplotype.  Needs no graph: the inputs are the reads,
 * the placements mgta_reads_pileup returned for them (per_read) and the sites.
 *   Contigs  0 .. n - 1, len_i = offsets[i + 1] - offsets[i].  Their letters are not an input: an allele is the read's base.
 *   Sites    contig i has the sites site_pos[site_off[i] .. site_off[i + 1]): 0-based positions, strictly ascending, each below len_i;
 *            site_off[0] = 0, S = site_off[n].  A site is named by its index u in site_pos, counted over all contigs of the call.
 *   Libraries  lib_end as in mgta_contig_sample_coverage: library s holds the reads [lib_end[s - 1], lib_end[s]), lib_end[-1] = 0;
 *            lib_paired[s] != 0 says its reads are interleaved mates.  The reads scanned are [0, lib_end[n_libs - 1]).
 *   Usable   read r is usable iff place[r].n_placed == 1.  With (i, o, d) = its contig, orient and diag it covers the positions
 *            x in [max(0, d), min(len_i, d + L)) of contig i (none where that range is empty) and shows there the letter s^o[x - d],
 *            s^o and L as in mgta_reads_pileup.  A record with another n_placed is not looked at beyond that field.
 *   Mates    in a paired library that starts at read f, the reads f + 2j and f + 2j + 1 are mates (the interleaving `buildlib` writes);
 *            an odd last read has no mate.  No read of an unpaired library has one.
 *   Fragment two mates are ONE fragment iff both are usable, both lie on the same contig and their orients differ.  Every other usable
 *            read is a fragment of its own.  The fragment's allele at a site is the letter of the read that covers the site; where
 *            both mates cover it, that letter if they agree, and where they disagree there is no allele: one conflict.
 *   Pairs    the sites u < v of one contig are tabled iff pos_v - pos_u < max_span (default 1000; 0 takes the default).  pair_off[u] =
 *            the number of tabled pairs (u', v') with u' < u, pair_off[S] = n_pairs; the pair (u, v) has the index pair_off[u] + (v - u - 1).
 * Outputs.  site_counts[u * 4 + b] = the fragments with the allele b (A C G T = 0 1 2 3) at site u.  joint[p * 16 + b_u * 4 + b_v] = the
 * fragments that have the allele b_u at u AND the allele b_v at v, p the index of the tabled pair (u, v).  Stats: n_reads = the reads
 * scanned; n_usable; n_fragments; n_mate_fragments = those of two mates; n_fragments_allele / n_fragments_linked = the fragments with at
 * least one / at least two alleles; n_alleles = the sum of site_counts; n_conflicts = (fragment, site) with two letters that differ;
 * n_pair_adds = the sum of joint; n_sites = S; n_pairs.  Everything but ms_* and peak_bytes is a function of the inputs alone: all sums
 * are integers, no output depends on the order of the reads inside a library (mates moved together), of the contigs or of any device
 * work, and mgta_ctx_set_phase_chunk moves none.
 * mgta_phase_pairs is host-only (no device, no context): it validates the site lists (site_off[0] = 0, site_off ascending, the
 * positions of a contig strictly ascending) and fills pair_off[S + 1], so that a caller can size joint.
 * Limits, each MGTA_EINVAL naming it with nothing written: sites ascending and below the contig's length; place[r].contig < n (and not
 * negative) for every usable read; lib_end not descending and lib_end[n_libs - 1] <= the reads uploaded; 1 <= n_libs <= 256;
 * joint_cap (in pairs) >= pair_off[S], the message names the count needed; reads of at most 65535 bases; n < 2^31, S < 2^32,
 * max_span >= 0; offsets ascending.  MGTA_EINVAL too for NULL reads, place, lib_end, lib_paired, offsets, site_off or pair_off, and for
 * NULL site_pos, site_counts or joint where S or n_pairs is not 0.  Device memory: 24 bytes per read scanned, 20 per site, 64 per
 * tabled pair; what does not fit is MGTA_ENOMEM.  n = 0 or S = 0: MGTA_OK and all outputs zero.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_phase_params { int32_t max_span; } mgta_phase_params;   /* 0 = the default, 1000 */
typedef struct mgta_phase_stats {
    int64_t n_reads, n_usable;
    int64_t n_fragments, n_mate_fragments;
    int64_t n_fragments_allele, n_fragments_linked;
    int64_t n_alleles, n_conflicts, n_pair_adds;
    int64_t n_sites, n_pairs;
    uint64_t peak_bytes;             /* most device bytes of the call's own buffers */
    double ms_upload, ms_scan, ms_total;   /* HIP events: place and tables host -> device; the scan; the two together */
} mgta_phase_stats;
int mgta_phase_pairs(const uint64_t *site_off /* [n + 1] */, const uint32_t *site_pos /* [S] */, int64_t n, int32_t max_span,
                     uint64_t *pair_off /* [S + 1] */);
int mgta_reads_phase(const mgta_reads *reads, int reads_reversed, const mgta_read_place *place /* [lib_end[n_libs - 1]] */,
                     const uint64_t *lib_end /* [n_libs] */, const uint8_t *lib_paired /* [n_libs] */, int n_libs,
                     const uint64_t *offsets /* [n + 1] */, int64_t n, const uint64_t *site_off /* [n + 1] */,
                     const uint32_t *site_pos /* [S] */, const mgta_phase_params *params /* NULL = defaults */,
                     uint32_t *site_counts /* [S * 4] */, uint64_t *pair_off /* [S + 1] */, uint32_t *joint /* [joint_cap * 16] */,
                     uint64_t joint_cap /* pairs */, mgta_phase_stats *stats /* or NULL */);
int mgta_ctx_set_phase_chunk(mgta_ctx *, uint32_t slots);   /* fragment slots per queue grab, 0 = the library's; a switch for tests, moves no output */

/* ------------------------------------------------------------------------------------------------
 * Read recruitment by the gene's model: which reads of the library the profile HMM places in one of six frames.  The rule is this
 * library's own; it is not HMMER's and nothing here is checked against it.  Needs no graph.  Two modes (mgta_recruit_params.mode):
 * the blocks Stretch .. Best below state mode 0, global in the stretch; mode 1, local, follows them.
 *   Input.     The reads [0, n_short_reads) of an uploaded library (reads_reversed as in mgta_reads_match_contigs) and a model of
 *              mgta_hmm_load, both of this context.
 *   Frames.    For a read of n bases: frame f in {0, 1, 2} is the read as sequenced from base f, frame f in {3, 4, 5} its reverse
 *              complement from base f - 3.  Frame f has floor((n - f mod 3) / 3) codons (none when n < f mod 3), translated by the
 *              standard code into the upper-case letters KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF (codon =
 *              16 b0 + 4 b1 + b2, A C G T = 0 .. 3).  The library holds A, C, G, T only: there is no X.
 *   Stretch.   A frame's stretch is its longest run of residues without a stop; among equally long runs the first (lowest aa_from,
 *              0-based in the frame's translation).  A stretch shorter than min_aa (>= 1) is not scored, nor is an empty one.
 *   Score.     Exactly what mgta_seqs_align returns for the stretch as a protein sequence (the block of mgta_seqs_align below: global
 *              in the stretch, local in the model, fp64, every + one IEEE add, the maximum first and then + e, the first candidate
 *              wins a tie): score bit for bit, model_to the lowest end column that reaches it, model_from the column of the first
 *              match state of the path its traceback walks.  No traceback is made here: every candidate of the recurrence carries
 *              the column it entered the model at, and the candidate that wins a maximum hands its column on, under the same tie
 *              order.  A stretch whose score is -inf is scored and unaligned.
 *   Best.      The scored frame with the highest score, the lowest frame number on equality.  status 0: aa_from, aa_len, frame,
 *              score, model_from, model_to of that frame.  status 1 (every scored frame is -inf): score -inf, frame, aa_from and
 *              aa_len of the lowest scored frame, model_from = model_to = 0.  status 2 (no scored frame): score -inf, zeros.
 *   Recruited. status == 0 and score >= min_score.  min_score is in nats; -inf, +inf and an exact score are legal thresholds.  The
 *              default, 20 bits = 20 * 0.6931471805599453 nats, is a knob, not a calibrated value: no E-values are computed.
 * Outputs: bit r of hit_bits[r / 64] = read r is recruited (reads at and behind n_short_reads have no bit and no record);
 * recs[r] when given; col_depth[j - 1], j = 1 .. M, when given = the number of recruited reads with model_from <= j <= model_to.
 * stats: n_reads scanned, n_frames_scored, n_cells = the sum of aa_len * M over the scored frames, n_unaligned (status 1),
 * n_unscored (status 2), n_recruited and n_recruited_frame[f] by best frame.  Everything but ms_*, blocks_per_cu, waves_per_block,
 * grid_blocks, lds_bytes, msc_in_lds, rows_per_wave and chunk is a function of (tables, reads, params) alone, the same to the last
 * bit for every chunk and across runs: integer atomics only, one writer per record.
 * The rule above is mode 0 = MGTA_RECRUIT_GLOBAL, the default (params NULL, or mode 0: the same bytes).  It is global in the stretch:
 * a read that runs over an end of the gene has to place its flank as inserts and scores low, and where the gene's own stop cuts a
 * frame in two only the longer run is looked at.
 *
 * mode 1 = MGTA_RECRUIT_LOCAL places reads locally.  Frames, translation, letters, tables and e(j, x) are as above.
 *   Stretches. Every maximal run of residues without a stop that has at least min_aa residues is scored, in every frame, in ascending
 *              position.
 *   Score.     The maximum, over all non-empty substrings x_a .. x_b of the stretch, of what mgta_seqs_align returns for that substring
 *              as a protein: the same recurrence and the same adds, bit for bit.  As one sweep over the stretch it is the recurrence
 *              of mgta_seqs_align with three changes.  (1) The match state of every row takes B = 0 as its first candidate, entering
 *              at column j and row i; on equality B wins over M, I, D.  (2) The delete state VD[i][j + 1] is fed by the value
 *              VM[i][j] would have WITHOUT its B candidate: a path does not delete straight after its first match, exactly as row 1
 *              of mgta_seqs_align has no delete state.  (3) The alignment may end in the match state of any row: score = max over
 *              i, j of VM[i][j].
 *   Ties.      In every maximum the candidate written first wins: B, M, I, D.  The end cell is the cell of the lowest column that
 *              reaches the score, and in that column the lowest row.
 *   Record.    model_to = the end column; model_from = the column of the match state the winning path entered at, carried through
 *              the recurrence with the winner of each maximum; aa_from, aa_len = the ALIGNED SPAN, first to last residue the path
 *              emits, 0-based in the frame's translation -- not the whole stretch as in mode 0.
 *   Best.      The stretch with the highest score; on equality the lower frame, then the lower aa_from.  status 0: as above.
 *              status 1 (every scored stretch is -inf): score -inf, the frame and the whole first scored stretch, model_from =
 *              model_to = 0.  status 2: no stretch of min_aa residues exists.  Recruited as above.
 *   Outputs.   col_depth as above; n_frames_scored counts the scored stretches, n_cells = the sum of stretch length * M over them.
 * Per read the local score is >= the global score, so at one threshold the local set contains the global set.  Local scores of
 * unrelated sequence are always positive: on a synthetic model of 120 columns, 300 stop-free 50-mers at random had a median of 12.0
 * bits and a maximum of 17.6 bits, so in local mode the default of 20 bits sits close to noise.  It remains a knob.
 * In both modes: no flanking states with a cost, no Forward score, no E-values, no prefilter, one device; the reverse model is not used.
 * Limits: a read of more than 3 * 4096 + 2 bases among the scanned ones is MGTA_EINVAL naming the first such read, with nothing
 * written.  MGTA_EINVAL also, before anything is written: NULL context / model / reads / hit_bits (n_short_reads > 0), n_short_reads
 * above the upload, a model or reads of another context, min_aa < 1, a NaN min_score, a mode other than 0 and 1, mode 1 with a model
 * of more than 1 048 575 columns (entry column and row share a register).  n_short_reads = 0: col_depth and stats all zero.
 * ------------------------------------------------------------------------------------------------ */
#define MGTA_RECRUIT_GLOBAL 0
#define MGTA_RECRUIT_LOCAL 1
typedef struct mgta_recruit_params { int32_t min_aa; int32_t mode /* MGTA_RECRUIT_GLOBAL (0, the default) or MGTA_RECRUIT_LOCAL */; double min_score; } mgta_recruit_params;
typedef struct mgta_recruit_rec { double score; int32_t model_from, model_to; uint16_t aa_from, aa_len; uint8_t frame, status; uint8_t pad[2]; } mgta_recruit_rec;
typedef struct mgta_recruit_stats {
    int64_t n_reads, n_frames_scored, n_cells;
    int64_t n_unaligned, n_unscored, n_recruited;
    int64_t n_recruited_frame[6];
    int64_t blocks_per_cu, waves_per_block, grid_blocks, lds_bytes, msc_in_lds;   /* as in mgta_align_stats */
    int64_t rows_per_wave;                 /* residues a wave sweeps back to back: 256, or what the longest read needs */
    int64_t chunk;                         /* reads per queue grab of this call */
    double ms_scan, ms_fill;               /* HIP events: the length scan; translation, fill and records */
} mgta_recruit_stats;
int mgta_reads_recruit(mgta_ctx *, const mgta_hmm *, const mgta_reads *, int reads_reversed, uint64_t n_short_reads,
                       const mgta_recruit_params * /* NULL = defaults: min_aa 20, min_score 20 bits in nats */,
                       uint64_t *hit_bits /* [ceil(n_short_reads / 64)] */, mgta_recruit_rec *recs /* [n_short_reads] or NULL */,
                       uint64_t *col_depth /* [M] or NULL */, mgta_recruit_stats *stats /* or NULL */);
int mgta_ctx_set_recruit_chunk(mgta_ctx *, uint32_t reads);   /* reads per queue grab (at most 64 are taken), 0 = the library's; a switch for tests, moves no output */

/* ------------------------------------------------------------------------------------------------
 * De-replication ("get the unique merged contigs", the first step of the reference's bin/post_proc.sh:50-55: `Clustering.jar derep`,
 * then `ReadSeq.jar rm-dupseq -d`, both from a submodule the reference does not ship).  Needs no graph.  Sequence i =
 * seqs[offsets[i] .. offsets[i + 1]), a byte string compared byte for byte: no case folding, no reverse complement (a gene's contigs
 * all have the gene's orientation).  Every sequence gets
 *   status 1 (duplicate): some j < i has s[j] == s[i]; rep[i] = the lowest such j, copies[i] = 0;
 *   status 2 (contained): a first occurrence that is a substring of some LONGER sequence; rep[i] = -1, copies[i] = the number of
 *                         inputs equal to s[i], itself included;
 *   status 0 (kept):      every other first occurrence; rep[i] = i, copies as for contained.
 * The empty sequence is contained as soon as a non-empty one exists.  The result is exactly this for any input: hashes only choose
 * what is compared, every equality and containment that decides a status is confirmed on the letters.  status, rep, copies and every
 * stats field but ms_* and n_compares are functions of the input only; n_compares depends on the order in which the device linked
 * the window lists and may differ from call to call.  mgta_ctx_set_derep_hash_bits keeps only the low `bits` bits of both hashes
 * (1 .. 64, default 64): with a few bits nearly every key collides and the outputs must not move -- a switch for tests, like
 * mgta_ctx_set_coverage_batch.  Limits: n < 2^31 sequences and fewer than 2^32 letters in the first occurrences; beyond either the
 * call returns MGTA_EINVAL and says which (nothing is truncated).  Device memory: about 9 bytes per letter of the first occurrences
 * plus 16 bytes per slot of the window table (2 to 4 slots per window), accounted like every other buffer of the context; what does
 * not fit is MGTA_ENOMEM.  MGTA_EINVAL: NULL context, n < 0, NULL outputs or offsets with n > 0, descending offsets (nothing is
 * written).  n = 0: MGTA_OK, stats all zero.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_derep_stats {
    int64_t n_seqs, n_letters;             /* the input */
    int64_t n_first;                       /* first occurrences = n_contained + n_kept */
    int64_t n_duplicates, n_contained, n_kept;
    int64_t n_windows;                     /* anchor windows of the first occurrences in the table (0 when there is one first occurrence) */
    int64_t anchor_len;                    /* min(16, shortest non-empty first occurrence); 0 when every sequence is empty */
    int64_t n_compares;                    /* letter comparisons of a sequence against a candidate, both passes; depends on list order */
    double ms_dups, ms_table, ms_verify;   /* HIP events: duplicate pass; packing + window table; anchor choice + list walks */
} mgta_derep_stats;
int mgta_seqs_derep(mgta_ctx *, const char *seqs, const uint64_t *offsets /* [n + 1] */, int64_t n,
                    uint8_t *status, int64_t *rep, uint32_t *copies, mgta_derep_stats *stats /* may be NULL */);
int mgta_ctx_set_derep_hash_bits(mgta_ctx *, int bits);   /* 1..64, default 64 */

/* ------------------------------------------------------------------------------------------------
 * Alignment of protein sequences to a profile HMM (the place of `hmmalign` in the reference's bin/post_proc.sh:65; HMMER is not
 * part of the reference and the rule below is this library's own, not hmmalign's).  Needs no graph.  Sequence i =
 * seqs[offsets[i] .. offsets[i + 1]), L residues x_1 .. x_L; the model is the one mgta_hmm_load was given, M nodes.
 *   Tables.    msc[j][a], j = 1 .. M: log-odds match score; tsc[X][j]: the transition OUT OF node j, X in MM, MI, MD, IM, II, DM, DD;
 *              insert emissions are 0; node M has no insert state; node 0's transitions are not used.
 *   Residues.  a = alpha[x_i]; a letter without a column (x, *, anything else; every byte >= 127) emits 0 in a match state:
 *              e(j, x) = msc[j][alpha[x]] or 0.
 *   Mode.      Global in the sequence, local in the model: every residue is emitted, the first one by some match state at no entry
 *              cost, the last one by some match state, where the alignment ends.  No flanking states.
 *   Recurrence (i = 1 .. L, j = 1 .. M; fp64, every + one IEEE add, no contraction; whatever is not defined is -inf):
 *              VM[i][j] = max( 0 if i == 1 (B);  and for i > 1, j > 1:  VM[i-1][j-1] + tsc[MM][j-1] (M),  VI[i-1][j-1] + tsc[IM][j-1] (I),
 *                              VD[i-1][j-1] + tsc[DM][j-1] (D) ) + e(j, x_i)             (the maximum first, then + e)
 *              VI[i][j] = max( VM[i-1][j] + tsc[MI][j],   VI[i-1][j] + tsc[II][j] )       i > 1, j < M
 *              VD[i][j] = max( VM[i][j-1] + tsc[MD][j-1], VD[i][j-1] + tsc[DD][j-1] )     i > 1, j > 1
 *   Score.     score = max_j VM[L][j].  Ties matter for the traceback only: in every max the candidate written first wins on equality
 *              (B, M, I, D), and the end column is the LOWEST j that reaches the score.
 *   Unaligned. L == 0 or score == -inf: status 1, score -inf, every count 0, model_from = model_to = 0, a row of '-', an empty path.
 *   No table entry may be +inf (-inf is legal), so no NaN arises.
 * Outputs: recs[i]; cols[i*M .. (i+1)*M) when cols is given: one byte per model column, the residue UPPER-CASED where a match state
 * emitted it, '-' for a delete state and for every column outside [model_from, model_to]; when path is given, the state path over
 * 'M', 'I', 'D' in path order at path + offsets[i] + i*M (the caller's offsets as they are), L + n_delete <= L + M - 2 characters,
 * not terminated, its length in path_len[i] (required with path).  Everything but stats.ms_* and the residency fields is a function
 * of (tables, sequences); mgta_ctx_set_align_batch (cells = L * M of one batch; 0 = by the context's free memory; a batch always holds
 * at least one sequence) is a switch for tests and moves no output.  Limits: L <= 4096 residues per sequence and n < 2^31; beyond,
 * MGTA_EINVAL names the limit.  Device memory: the letters, one traceback byte per cell of a batch and the batch's outputs, accounted
 * like every other buffer; what does not fit is MGTA_ENOMEM.  MGTA_EINVAL: NULL context / model / recs / offsets (n > 0) / path_len
 * with path, n < 0, descending offsets, a model of another context (nothing is written).  n = 0: MGTA_OK, stats all zero.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_align_rec {
    double score;                          /* -inf when unaligned */
    int32_t status;                        /* 0 aligned, 1 unaligned */
    int32_t model_from, model_to;          /* first and last match column, 1-based (0 when unaligned) */
    int32_t n_match, n_insert, n_delete;
} mgta_align_rec;
typedef struct mgta_align_stats {
    int64_t n_seqs, n_aligned, n_unaligned;
    int64_t n_cells;                       /* sum of L * M */
    int64_t n_batches;
    int64_t blocks_per_cu;                 /* what the runtime answered for the fill kernel with its LDS (largest over the batches) */
    int64_t waves_per_block;               /* sequences in flight per workgroup: 4, 2 or 1 by the longest sequence of the batch (smallest over the batches) */
    int64_t grid_blocks;                   /* workgroups of the largest launch */
    int64_t lds_bytes;                     /* LDS of a workgroup (largest over the batches) */
    int64_t msc_in_lds;                    /* 1: every batch read the match scores from LDS; 0: some batch read them from device memory */
    double ms_fill, ms_trace;              /* HIP events, summed over the batches */
} mgta_align_stats;
int mgta_seqs_align(mgta_ctx *, const mgta_hmm *, const char *seqs, const uint64_t *offsets /* [n + 1] */, int64_t n,
                    mgta_align_rec *recs /* [n] */, uint8_t *cols /* [n * M] or NULL */, char *path /* [offsets[n] + n * M] or NULL */,
                    int32_t *path_len /* [n] or NULL */, mgta_align_stats *stats /* may be NULL */);
int mgta_ctx_set_align_batch(mgta_ctx *, int64_t cells);   /* 0 = by memory (default) */

/* ------------------------------------------------------------------------------------------------
 * Forward score and per-residue posteriors of protein sequences on a profile HMM: how far a placement of mgta_seqs_align can be
 * trusted (what a user of `hmmalign` read from its PP lines and a user of Xander from a bit score).  The rule below is this
 * library's own, as mgta_seqs_align's is: HMMER is on none of the project's machines and nothing here is checked against it.  No
 * optimal-accuracy re-alignment is made from the posteriors.  Needs no graph.
 *   Tables, residues, mode and WHICH CELLS EXIST are exactly mgta_seqs_align's: global in the sequence, local in the model; the
 *              first residue is emitted by some match state at no entry cost, the last one by some match state; insert emissions
 *              are 0; the insert state exists for i > 1 and j < M, the delete state for i > 1 and j > 1, and FM[i][j] for i > 1
 *              needs j > 1.  e(j, i) = msc[j][alpha[x_i]], or 0 for a letter without a column; t.. is the transition OUT OF the
 *              node named.  Whatever is not defined is -inf.
 *   lse.       Every max of that rule becomes lse(a, b, c) = m + log(exp(a - m) + exp(b - m) + exp(c - m)), m = max(a, b, c); with
 *              m = -inf the result is -inf.  -inf - -inf is never evaluated, so `*` entries of a model stay legal and no NaN
 *              arises.  Everything is fp64.
 *   Forward (i = 1 .. L, j = 1 .. M):
 *              FM[1][j] = e(j, 1)
 *              FM[i][j] = lse(FM[i-1][j-1] + tMM[j-1], FI[i-1][j-1] + tIM[j-1], FD[i-1][j-1] + tDM[j-1]) + e(j, i)     i > 1, j > 1
 *              FI[i][j] = lse(FM[i-1][j] + tMI[j], FI[i-1][j] + tII[j])                                                i > 1, j < M
 *              FD[i][j] = lse(FM[i][j-1] + tMD[j-1], FD[i][j-1] + tDD[j-1])                                            i > 1, j > 1
 *              F = lse over j of FM[L][j]
 *   Backward (i = L .. 1, j = M .. 1), with N(i, j) = e(j+1, i+1) + BM[i+1][j+1] for j < M, else -inf:
 *              BM[L][j] = 0;  BI[L][j] = BD[L][j] = -inf
 *              BM[i][j] = lse(tMM[j] + N(i, j), tMI[j] + BI[i+1][j] (j < M), tMD[j] + BD[i][j+1] (j < M and i > 1))    i < L
 *              BI[i][j] = lse(tIM[j] + N(i, j), tII[j] + BI[i+1][j])                                                   1 < i < L, j < M
 *              BD[i][j] = lse(tDM[j] + N(i, j), tDD[j] + BD[i][j+1])                                                   1 < i < L, 1 < j < M
 *              Bt = lse over j of e(j, 1) + BM[1][j]       (equals F up to rounding; reported as a check value)
 *   Posteriors. PM[i][j] = exp(FM[i][j] + BM[i][j] - F), PI[i][j] = exp(FI[i][j] + BI[i][j] - F); 0 where either factor is -inf.
 *              For every residue i the sum over j of PM[i][j] + PI[i][j] is 1.
 *   Unaligned. L == 0 or F == -inf (exactly when mgta_seqs_align calls the sequence unaligned): status 1, fwd = bwd = -inf, zeros
 *              everywhere else.
 * Labels: labels[r] (r as in seqs: offsets[i] + the residue's place) names the state whose posterior pp[r] is: +j the match state
 * of node j, -j the insert state of node j (1 <= j < M), 0 none (pp[r] = 0).  Any labelling is evaluated, not only Viterbi's; the
 * callers above pass the one the path of mgta_seqs_align gives.  Outputs: recs[i]; pp[offsets[0] .. offsets[n]) when given (needs
 * labels); col_match[i*M + j-1] = sum over the rows of PM[.][j] and col_insert[i*M + j-1] = that of PI[.][j] when given.  Everything
 * but stats.ms_*, n_batches and the residency fields (workgroups, waves_per_block, blocks_per_cu, lds_bytes, msc_in_lds,
 * peak_bytes) is a function of (tables, sequences, labels), the same to the last bit whatever the batch and across runs: every
 * output has one writer and one fixed order of additions.  mgta_ctx_set_posterior_batch (cells = L * M of one batch; 0 = by the
 * context's free memory; a batch always holds at least one sequence) is a switch for tests and moves no output.  Limits: L <= 4096
 * residues per sequence and n < 2^31; beyond, MGTA_EINVAL names the limit.  Device memory: the letters, the labels and pp, 16 bytes
 * per cell of a batch (FM and FI) and the batch's outputs, accounted like every other buffer; what does not fit is MGTA_ENOMEM.
 * MGTA_EINVAL: NULL context / model / recs / offsets (n > 0), pp without labels, n < 0, descending offsets, a model of another
 * context, a label above M or below -(M - 1) (the first one is named); nothing is written.  n = 0: MGTA_OK, stats all zero.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_post_rec {
    double fwd, bwd;                       /* F and Bt in nats; -inf when unaligned */
    int32_t status, pad;                   /* 0 scored, 1 unaligned */
} mgta_post_rec;
typedef struct mgta_post_stats {
    int64_t n_seqs, n_scored, n_unaligned;
    int64_t n_cells;                       /* sum of L * M */
    int64_t n_batches;
    int64_t workgroups;                    /* of the largest launch */
    int64_t waves_per_block;               /* sequences in flight per workgroup: 4, 2 or 1 by the longest sequence of the batch (smallest over the batches) */
    int64_t blocks_per_cu;                 /* what the runtime answered, the smaller of the two kernels (largest over the batches) */
    int64_t lds_bytes;                     /* LDS of a workgroup of the backward kernel (largest over the batches) */
    int64_t msc_in_lds;                    /* 1: every batch read the match scores from LDS; 0: some batch read them from device memory */
    int64_t peak_bytes;                    /* most device memory the context held during the call */
    double ms_forward, ms_backward;        /* HIP events, summed over the batches */
} mgta_post_stats;
int mgta_seqs_posterior(mgta_ctx *, const mgta_hmm *, const char *seqs, const uint64_t *offsets /* [n + 1] */, int64_t n,
                        const int32_t *labels /* [offsets[n]] or NULL */, mgta_post_rec *recs /* [n] */,
                        double *pp /* [offsets[n]] or NULL; needs labels */, double *col_match /* [n * M] or NULL */,
                        double *col_insert /* [n * M] or NULL */, mgta_post_stats *stats /* may be NULL */);
int mgta_ctx_set_posterior_batch(mgta_ctx *, int64_t cells);   /* 0 = by memory (default); a switch for tests, moves no output */

/* ------------------------------------------------------------------------------------------------
 * Complete-linkage clusters of aligned rows ("cluster at 99% aa identity", the reference's bin/post_proc.sh:57-85: `Clustering.jar
 * dmatrix -l 25`, `cluster`, `rep-seqs -l <cutoff>`, from a submodule the reference does not ship; the rule below is this library's
 * own and is not checked against the jars).  Needs no graph.  Input: n rows of M bytes, row r = rows[r*M .. (r+1)*M), the `cols` rows
 * of mgta_seqs_align: a byte is '-' or a residue; lens[n], the unaligned length of each record; min_overlap >= 1; cutoff, an fp64 in
 * [0, 1].
 *   Pair counts.  For i < j: n_overlap(i,j) = the number of columns where both rows hold a byte other than '-'; n_diff(i,j) = the
 *                 number of those columns where the two bytes differ.  Bytes are compared byte for byte, no case folding; every value
 *                 0 .. 255 other than '-' is a residue.  Inserted residues are not in the rows and do not count; a column where only
 *                 one row has a residue does not count either way.
 *   Kept pair.    n_overlap >= min_overlap and (double)n_diff <= cutoff * (double)n_overlap: one IEEE multiply and one compare, no
 *                 contraction.  Every other pair is APART.
 *   Clusters.     A row with no residue at all is UNALIGNED: in no cluster (cluster -1, rep -1).  Every other row starts as a cluster
 *                 of its own.  Then, repeatedly: of every pair of clusters (A, B), min(A) < min(B), whose cross pairs are ALL kept,
 *                 take the one with the smallest complete-linkage distance = the largest n_diff / n_overlap over its cross pairs
 *                 (fractions compared exactly, by cross-multiplication in 64-bit integers, never in floating point; ties: the lower
 *                 min(A), then the lower min(B)) and merge it; stop when no such pair exists.  This is complete linkage cut at
 *                 `cutoff`.  Only kept pairs can ever decide a merge, so the sparse list of kept pairs is all the linkage needs.
 *   Numbering.    Clusters are numbered 0, 1, .. by their lowest member.  A cluster's representative is the member with the largest
 *                 lens, the lowest index on a tie (`rep-seqs -l`).
 * mgta_rows_pairs gives the kept pairs sorted by (i, j).  At most `cap` pairs are stored: *n_pairs is the number found; when it
 * exceeds cap NOTHING is stored (call again with a buffer that holds them; pairs = NULL with cap = 0 only counts).
 * Both calls hold every kept pair on the host while they run, also when the count then exceeds cap: a caller that expects many pairs
 * saves the second device pass by passing a generous buffer at once.
 * mgta_rows_cluster runs the pairs on the device and the linkage on the host inside the library (connected components of the
 * kept-pair graph first, then each component with a priority queue).  mgta_pairs_link is that linkage alone, host only, no context
 * and no device: the kept pairs of n rows ascending by (i, j) as mgta_rows_pairs gives them, n_residues[i] = the residue columns of
 * row i (0 = unaligned), lens; the same four outputs and the linkage's fields of stats.  MGTA_EINVAL: a pair outside 0 <= i < j < n,
 * n_overlap = 0, n_diff > n_overlap, a row of a pair without residues, pairs not ascending, n_residues outside 0 .. 65535, NULLs.  cluster[i], rep[i]: the cluster's number and the representative's
 * row; rep_diff[i], rep_overlap[i]: the counts of row i against its representative (every member of a cluster is a kept pair with
 * every other): for the representative itself 0 and its own number of residue columns, for an unaligned row 0 and 0.
 * Every output is a function of the inputs only, except stats.ms_*, the counters of work done (n_tiles, n_link_pops) and the
 * residency fields.  mgta_ctx_set_cluster_tile sets the rows of one row block (0 = the default, 4096): the device works on one row
 * block x row block tile at a time, so its memory is bounded whatever n is (4 bytes per pair of a tile, the tile's kept pairs, the
 * rows once); a switch for tests, the outputs do not move.  Limits: n < 2^31 and 1 <= M < 65536 (both counts fit 16 bits); beyond
 * either the call returns MGTA_EINVAL, names the limit and writes nothing.  The rows (1.125 bytes per input byte, laid out once) must fit
 * the device memory the call may use, else MGTA_ENOMEM; the linkage holds fewer than 2^32 kept pairs, else MGTA_ENOMEM before it starts.  Kept pairs that do not fit the memory the call may use:
 * MGTA_ENOMEM with the count in the message; nothing is truncated.  MGTA_EINVAL: NULL context, n < 0, NULL rows / lens / outputs /
 * n_pairs with n > 0, NULL pairs with cap > 0, cap < 0, min_overlap < 1, cutoff outside [0, 1] or NaN (nothing is written).
 * n = 0: MGTA_OK, stats all zero.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_row_pair { int32_t i, j; uint16_t n_diff, n_overlap; } mgta_row_pair;   /* i < j, kept pairs only */
typedef struct mgta_cluster_stats {
    int64_t n_rows, n_unaligned;
    int64_t n_pairs_kept;
    int64_t n_clusters, n_singletons, largest_cluster;   /* mgta_rows_cluster only */
    int64_t n_components;                  /* connected components of the kept-pair graph over the aligned rows (mgta_rows_cluster only) */
    int64_t n_tiles;                       /* row block x row block tiles the device worked on */
    int64_t n_link_pops;                   /* entries the linkage took from its queues, stale ones included */
    int64_t blocks_per_cu;                 /* what the runtime answered for the pairs kernel */
    int64_t grid_blocks;                   /* workgroups of the largest pairs launch */
    int64_t lds_bytes;                     /* LDS of a workgroup of the pairs kernel */
    int64_t peak_bytes;                    /* most device memory the call held at once */
    double ms_pairs, ms_link;              /* HIP events summed over the tiles (layout, pairs, count, scan, write); host clock of the linkage */
} mgta_cluster_stats;
int mgta_rows_pairs(mgta_ctx *, const uint8_t *rows /* [n * M] */, int64_t n, int64_t M, int64_t min_overlap, double cutoff,
                    mgta_row_pair *pairs /* [cap] or NULL */, int64_t cap, int64_t *n_pairs, mgta_cluster_stats *stats /* may be NULL */);
int mgta_rows_cluster(mgta_ctx *, const uint8_t *rows /* [n * M] */, const int64_t *lens /* [n] */, int64_t n, int64_t M, int64_t min_overlap,
                      double cutoff, int32_t *cluster /* [n] */, int64_t *rep /* [n] */, uint16_t *rep_diff /* [n] */,
                      uint16_t *rep_overlap /* [n] */, mgta_cluster_stats *stats /* may be NULL */);
int mgta_pairs_link(const mgta_row_pair *pairs /* [n_pairs], ascending by (i, j) */, int64_t n_pairs, const int32_t *n_residues /* [n] */,
                    const int64_t *lens /* [n] */, int64_t n, int32_t *cluster, int64_t *rep, uint16_t *rep_diff, uint16_t *rep_overlap,
                    mgta_cluster_stats *stats /* may be NULL */);
int mgta_ctx_set_cluster_tile(mgta_ctx *, int64_t rows_per_tile);   /* 0 = default */

/* ------------------------------------------------------------------------------------------------
 * The merge tree of aligned rows: clusters at several cut-offs from one pass over the pairs.  Definitions as in the block above.
 *   Tree.   Input: the kept pairs of n rows ascending by (i, j), as mgta_rows_pairs gives them for (min_overlap, D), and
 *           n_residues[n].  The tree is the SET of merges the rule of mgta_rows_cluster makes on these pairs.  One merge is an
 *           mgta_tree_merge: a < b are the lowest members of the two clusters when they merge (the merged cluster keeps name a),
 *           n_diff / n_overlap their complete-linkage distance, the largest fraction over their cross pairs, IN LOWEST TERMS, 0 as
 *           0 / 1: which cross pair attains it never shows.  The list is sorted ascending by (fraction compared exactly, a, b); this
 *           is not the order in which the sequential rule makes the merges, it is a function of the input.  n_merges = aligned rows -
 *           clusters at D.
 *   Cut.    The clusters at cut-off c, an fp64 with 0 <= c <= D, are BY DEFINITION what mgta_pairs_link returns for the sub-list of the
 *           pairs kept at c ((double)n_diff <= c * (double)n_overlap): the same four outputs, numbering and representative.  Merge
 *           distances of complete linkage never decrease, so a cut is a prefix of the tree WHERE THE KEPT RULE IS MONOTONE in the
 *           fraction.  One rounded product is not: for a cut-off an ulp below a small rational it may keep 3 / 22 and not 15 / 110.
 *           So mgta_tree_cut takes, in one pass over the pairs, hi = the largest fraction among the pairs kept at c and lo = the
 *           smallest among those not kept; when no pair is "not kept" or hi < lo exactly, the clusters are the union of the merges
 *           whose fraction is <= hi (none when no pair is kept), numbered and given representatives as by mgta_pairs_link; otherwise
 *           it runs mgta_pairs_link's linkage on the kept sub-list and counts that in stats.n_cut_fallbacks.  Both routes give the
 *           same answer where both apply.  mgta_tree_cut is host only, no context and no device; `merges` must be the tree of
 *           `pairs`.  It cannot know D: a caller that cuts above D gets the clusters at D's pairs; mgta_rows_clusters checks c <= D.
 * mgta_pairs_tree is the device part: symmetric neighbour lists per cluster built once from the pairs, then rounds launched by the
 * host in which every pair of clusters that are each other's smallest key merges at once (under the strict order of the keys the
 * sequential rule merges exactly those, whatever else it merges before; complete linkage is reducible), with one small read-back a
 * round and at most n - 1 rounds.  A clique of m clusters at one distance merges one pair a round: m - 1 rounds over m lists
 * (stats.n_rounds and n_entries_visited show it).  At most `cap` merges are stored: *n_merges is the number found; when it exceeds cap
 * NOTHING is stored.  Device memory: 32 bytes per kept pair for the lists (two buffers), 12 more while they are built, about 80 per
 * row; MGTA_ENOMEM names the need.  The limits of the linkage apply: n < 2^31 and fewer than 2^32 kept pairs (MGTA_ENOMEM).
 * MGTA_EINVAL: the cases of mgta_pairs_link, NULL context, cap < 0, NULL merges with cap > 0, NULL n_merges (nothing is written).
 * mgta_rows_clusters runs mgta_rows_pairs' pass once at D = the largest of cutoffs[n_cutoffs] (n_cutoffs >= 1, each in [0, 1]), the
 * tree on the device and one cut per cut-off on the host: cluster, rep, rep_diff, rep_overlap hold n_cutoffs * n values, cut-off k at
 * [k * n, (k + 1) * n); merges [n] may be NULL (then n_merges may be NULL too).  n = 0: MGTA_OK, stats all zero.  Every output is a
 * function of the inputs only, except stats.ms_*, peak_bytes and the counters of work done.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_tree_merge { int32_t a, b; uint16_t n_diff, n_overlap; } mgta_tree_merge;   /* a < b; the fraction in lowest terms */
typedef struct mgta_tree_stats {
    int64_t n_rows, n_pairs, n_merges;
    int64_t n_rounds;                      /* rounds that merged something */
    int64_t n_entries_visited;             /* list entries read: every list once for its first nearest, then the old lists of every rewrite */
    int64_t n_lists_rewritten;             /* summed over the rounds */
    int64_t n_cut_fallbacks;               /* cuts that ran the host linkage on the kept sub-list */
    int64_t n_unaligned, n_clusters, n_singletons, largest_cluster;   /* of the last cut */
    int64_t peak_bytes;                    /* most device memory the call held at once */
    double ms_pairs;                       /* mgta_rows_clusters: the pairs pass */
    double ms_build, ms_rounds;            /* HIP events: the lists; the rounds (read-backs included) */
    double ms_cut;                         /* host clock, summed over the cuts */
} mgta_tree_stats;
int mgta_pairs_tree(mgta_ctx *, const mgta_row_pair *pairs /* [n_pairs], ascending by (i, j) */, int64_t n_pairs, const int32_t *n_residues /* [n] */,
                    int64_t n, mgta_tree_merge *merges /* [cap] or NULL */, int64_t cap, int64_t *n_merges, mgta_tree_stats *stats /* may be NULL */);
int mgta_tree_cut(const mgta_row_pair *pairs, int64_t n_pairs, const mgta_tree_merge *merges, int64_t n_merges, const int32_t *n_residues /* [n] */,
                  const int64_t *lens /* [n] */, int64_t n, double cutoff, int32_t *cluster, int64_t *rep, uint16_t *rep_diff, uint16_t *rep_overlap,
                  mgta_tree_stats *stats /* may be NULL */);
int mgta_rows_clusters(mgta_ctx *, const uint8_t *rows /* [n * M] */, const int64_t *lens /* [n] */, int64_t n, int64_t M, int64_t min_overlap,
                       const double *cutoffs /* [n_cutoffs] */, int64_t n_cutoffs, int32_t *cluster /* [n_cutoffs * n] */, int64_t *rep,
                       uint16_t *rep_diff, uint16_t *rep_overlap, mgta_tree_merge *merges /* [n] or NULL */, int64_t *n_merges,
                       mgta_tree_stats *stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------------
 * The nearest reference protein of every contig (the place of FrameBot in the reference's bin/post_proc.sh:106-111, which names
 * `AlignmentTool pairwise-knn` on the protein representatives as the alternative; neither tool nor a BLOSUM file is part of the
 * reference, and the rule below is this library's own, not theirs).  Needs no graph.  Contig i = seqs[offsets[i] .. offsets[i + 1]),
 * L residues x_1 .. x_L; reference r = refs[ref_offsets[r] .. ref_offsets[r + 1]), R residues y_1 .. y_R.
 *   Residue class.  c(b) = 1 .. 26 for an ASCII letter (A / a = 1 .. Z / z = 26), c(b) = 0 for every other byte.
 *   Scoring.    sub, int8[27][27], the caller's: s(i, j) = sub[c(x_i)][c(y_j)].  gap_open and gap_extend, integers with
 *               0 <= gap_extend <= gap_open <= 1024; gap_open is the cost of a gap's FIRST residue, gap_extend of every further one.
 *   Mode.       Global in the contig, local in the reference (the choice of mgta_seqs_align, for the same reason: a contig is a
 *               piece of the gene): every contig residue is consumed, the first one is matched at no entry cost, the last one is
 *               matched and the alignment ends there.
 *   Recurrence  (i = 1 .. L, j = 1 .. R; int32 throughout; whatever is not defined below is undefined and is never a candidate):
 *               M[i][j] = s(i,j) + max( 0 if i == 1 (B);  for i > 1, j > 1:  M[i-1][j-1] (M), X[i-1][j-1] (X), Y[i-1][j-1] (Y) )
 *               X[i][j] = max( M[i-1][j] - gap_open, X[i-1][j] - gap_extend )      i > 1     (x_i against a gap: insert)
 *               Y[i][j] = max( M[i][j-1] - gap_open, Y[i][j-1] - gap_extend )      j > 1     (y_j skipped: delete)
 *   Score.      score(contig, ref) = max_j M[L][j]; no score when L = 0, R = 0 or no M[L][j] is defined (R = 1 < L is the smallest
 *               such case).  Ties decide the traceback only: the candidate written first wins (B, M, X, Y; for X: M, X; for Y: M, Y),
 *               and the end column is the LOWEST j that reaches the score.
 *   Nearest.    The reference with the highest score; on a tie the lowest reference index.  A contig with no scored pair is
 *               UNALIGNED: status 1, ref -1, every other field 0, an empty path.
 *   Record.     From the traceback against the nearest reference only: ref, score; ref_from, ref_to: the first and the last matched
 *               reference position, 1-based; n_match: match states; n_ident: match states with c(x_i) == c(y_j) != 0; n_insert,
 *               n_delete; when path is given, the state path over 'M', 'I', 'D' in path order at path + offsets[i] + i*4096 (the
 *               caller's offsets as they are), L + n_delete characters, not terminated, its length in path_len[i] (required with path).
 *   Range.      Under the limits a defined value is at most 127 * 4096 + 1024 * 8192 < 2^24 in magnitude and never leaves int32.  The
 *               kernels hold "undefined" as the sentinel -2^30; whatever derives from it stays within 9.6e6 of it (a monotone path of
 *               at most 8191 + 128 steps, each worth between -1152 and +127), so it is below every defined value, below the floor
 *               -2^29 under which nothing is reported, and above INT32_MIN: nothing wraps.
 * scores, when given, takes score(i, r) of EVERY pair at scores[i * n_ref + r], INT32_MIN where the pair has no score (the tests'
 * view; it costs 4 bytes of device memory per pair).  Two passes on the device: the score pass over all pairs, int32 without any
 * traceback store, one wave per contig along the concatenation of the references; then the n (contig, nearest reference) pairs are
 * filled again with one direction byte per cell, in batches, and one thread per pair walks the bytes back.  Every output is a
 * function of the inputs only, except stats.ms_*, the counters of work done (n_batches, n_segments) and the residency fields;
 * mgta_ctx_set_nearest_batch (cells = L * R of one trace batch; 0 = by the context's free memory; a batch always holds at least one
 * pair) is a switch for tests and moves no output.  Limits: L <= 4096, R <= 4096, n < 2^31, n_ref < 2^31, and the references together
 * hold fewer than 2^31 residues (a column of their concatenation is a 32-bit number); beyond any of them MGTA_EINVAL names the limit
 * and nothing is written.  Device memory: the letters of both sides, 8 bytes per (contig, segment of references) of the score pass,
 * one traceback byte per cell of a trace batch and the batch's outputs, accounted like every other buffer; what does not fit is
 * MGTA_ENOMEM.  MGTA_EINVAL (nothing is written): NULL context; with n > 0 NULL offsets / recs / sub / ref_offsets (n_ref > 0) /
 * seqs or refs with residues / path_len with path; n < 0, n_ref < 0, descending offsets on either side, gap parameters out of range.
 * n = 0: MGTA_OK, stats all zero.  n_ref = 0: every contig unaligned.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_nearest_rec { int32_t status, ref, score, ref_from, ref_to, n_match, n_ident, n_insert, n_delete; } mgta_nearest_rec;
typedef struct mgta_nearest_stats {
    int64_t n_seqs, n_refs, n_pairs, n_unaligned;
    int64_t n_cells;                       /* sum of L * R over all pairs (INT64_MAX when it does not fit) */
    int64_t n_trace_cells;                 /* sum of L * R over the (contig, nearest reference) pairs */
    int64_t n_batches;                     /* batches of the trace pass */
    int64_t n_segments;                    /* runs of whole references the score pass cut the concatenation into (1 when the contigs fill the device) */
    int64_t blocks_per_cu;                 /* what the runtime answered for the score kernel with its LDS */
    int64_t waves_per_block;               /* contigs in flight per workgroup: 4, 2 or 1 by the longest contig */
    int64_t grid_blocks;                   /* workgroups of the score pass */
    int64_t lds_bytes;                     /* LDS of a workgroup */
    int64_t peak_bytes;                    /* most device memory the call held at once */
    double ms_score, ms_trace;             /* HIP events: the score pass; fill and walk of the trace pass, summed over the batches */
} mgta_nearest_stats;
int mgta_seqs_nearest(mgta_ctx *, const char *seqs, const uint64_t *offsets /* [n + 1] */, int64_t n,
                      const char *refs, const uint64_t *ref_offsets /* [n_ref + 1] */, int64_t n_ref,
                      const int8_t *sub /* [27 * 27] */, int32_t gap_open, int32_t gap_extend,
                      mgta_nearest_rec *recs /* [n] */, int32_t *scores /* [n * n_ref] or NULL; INT32_MIN = no score */,
                      char *path /* [offsets[n] + n * 4096] or NULL */, int32_t *path_len /* [n] or NULL */, mgta_nearest_stats *stats /* may be NULL */);
int mgta_ctx_set_nearest_batch(mgta_ctx *, int64_t cells);   /* 0 = by memory (default); a switch for tests, the outputs do not move */

/* ------------------------------------------------------------------------------------------------
 * The nearest reference protein of every NUCLEOTIDE contig, with shifts of the reading frame (the place of FrameBot on the nucleotide
 * representatives in the reference's bin/post_proc.sh:106-109; FrameBot is not part of the reference, and the rule below is this
 * library's own, not FrameBot's).  Needs no graph.  Contig i = nucl[offsets[i] .. offsets[i + 1]), L nucleotides x_1 .. x_L;
 * reference r = refs[ref_offsets[r] .. ref_offsets[r + 1]), R residues y_1 .. y_R.  Residue classes c(), sub, gap_open and gap_extend
 * are those of mgta_seqs_nearest; frameshift is one more cost, 0 <= frameshift <= 1024.
 *   Nucleotide. A, C, G, T of either case are 0 .. 3; every other byte is unknown.
 *   Codon.      For i >= 3, a(i) is the residue of (x_{i-2}, x_{i-1}, x_i) by the standard code (codon = 16 * b0 + 4 * b1 + b2 into
 *               KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF); a codon with an unknown letter gives X; a stop gives
 *               `*`, which is class 0.  e(i, j) = sub[c(a(i))][c(y_j)], u(j) = sub[c('X')][c(y_j)].
 *   Mode.       Global in the contig, local in the reference: every nucleotide is consumed, the alignment begins before x_1 at no
 *               cost against any reference position, and it ends in a match state at row L.
 *   Recurrence  (rows i = 1 .. L are nucleotide positions, j = 1 .. R; int32; whatever is not defined is never a candidate):
 *               P[i][j]  = the maximum of the defined M[i][j], X[i][j], Y[i][j], preference M, X, Y.
 *               prev(i', j') = 0 when i' = 0 (B, any j'); P[i'][j'] for i' >= 1 and j' >= 1; undefined otherwise.
 *               M[i][j]  = the maximum, the first candidate winning a tie, of
 *                            1. i >= 3:  e(i, j) + prev(i-3, j-1)                  (a codon)
 *                            2. i >= 2:  u(j) - frameshift + prev(i-2, j-1)        (one nucleotide missing: two letters stand for a
 *                                                                                  residue nobody knows)
 *                            3. i >= 4:  e(i, j) - frameshift + prev(i-4, j-1)     (one nucleotide too many: x_{i-3} is dropped, the
 *                                                                                  codon is the last three)
 *               X[i][j]  = max( M[i-3][j] - gap_open, X[i-3][j] - gap_extend )    i >= 4    (a whole codon against a gap: insert)
 *               Y[i][j]  = max( M[i][j-1] - gap_open, Y[i][j-1] - gap_extend )    j >= 2    (y_j skipped: delete)
 *   Score.      score(contig, ref) = max_j M[L][j], the end column the LOWEST such j; no score where no M[L][j] is defined (L = 0,
 *               L = 1, R = 0, and R = 1 with L >= 5 are such cases).  For X and Y the candidate written first wins a tie (M).
 *   Nearest.    The reference with the highest score; on a tie the lowest reference index.  A contig with no scored pair is
 *               UNALIGNED: status 1, ref -1, every other field 0, an empty path.
 *   Record.     From the traceback against the nearest reference only: ref, score; ref_from, ref_to: the reference position of the
 *               first and of the last match state, 1-based; n_match, n_short, n_long: match states of candidate 1, 2, 3; n_ident:
 *               candidate 1 and 3 states with c(a(i)) == c(y_j) != 0; n_insert: inserted codons; n_delete.  When path is given,
 *               the state path in path order over 'M' (candidate 1), '<' (2, short), '>' (3, long), 'I', 'D' at
 *               path + offsets[i] + i*4096 (the caller's offsets as they are), at most L/2 + R characters, not terminated, its length
 *               in path_len[i] (required with path).
 *   Range.      A path has at most 4096 residue-consuming states, 4096 inserted codons, 4096 deleted residues and 4096 shifts (a
 *               shift is a residue-consuming state), so a defined value is at most 127 * 4096 + 1024 * 3 * 4096 = 13 103 104 < 2^24
 *               in magnitude.  The kernels hold "undefined" as the sentinel -2^30; whatever derives from it has moved by at most
 *               12288 + 4096 + 128 steps of between -(128 + 1024 + 1024) and +127 each, so it lies within [-3.6e7, +2.1e6] of the
 *               sentinel: below every defined value, below the floor -2^29 under which nothing is reported, above INT32_MIN.
 * scores, when given, takes score(i, r) of EVERY pair at scores[i * n_ref + r], INT32_MIN where the pair has no score.  The passes,
 * the batches (mgta_ctx_set_nearest_batch sets this call's trace batch too, in cells = L * R), the device memory, MGTA_ENOMEM and
 * the MGTA_EINVAL cases are those of mgta_seqs_nearest, with `nucl` for `seqs` and frameshift out of range as one more; the workgroup
 * holds 4, 2 or 1 waves within 80 KB of LDS while the longest contig allows it, and one wave with up to 864 + 9 * 12288 bytes above
 * that.  Every output is a function of the inputs only, except stats.ms_*, the counters of work done and the residency fields.
 * Limits: L <= 12288, R <= 4096, n < 2^31, n_ref < 2^31, fewer than 2^31 reference residues in all; beyond any of them MGTA_EINVAL
 * names the limit and nothing is written.  n = 0: MGTA_OK, stats all zero.  n_ref = 0: every contig unaligned.
 * It is not FrameBot's rule: shifts of one nucleotide only, a long codon always drops its first letter, and no metric pre-filter.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_frameshift_rec { int32_t status, ref, score, ref_from, ref_to, n_match, n_ident, n_insert, n_delete, n_short, n_long; } mgta_frameshift_rec;
typedef struct mgta_frameshift_stats {
    int64_t n_seqs, n_refs, n_pairs, n_unaligned;
    int64_t n_cells;                       /* sum of L * R over all pairs, L in nucleotide rows (INT64_MAX when it does not fit) */
    int64_t n_trace_cells;                 /* sum of L * R over the (contig, nearest reference) pairs */
    int64_t n_batches;                     /* batches of the trace pass */
    int64_t n_segments;                    /* runs of whole references the score pass cut the concatenation into */
    int64_t blocks_per_cu;                 /* what the runtime answered for the score kernel with its LDS */
    int64_t waves_per_block;               /* contigs in flight per workgroup: 4, 2 or 1 by the longest contig */
    int64_t grid_blocks;                   /* workgroups of the score pass */
    int64_t lds_bytes;                     /* LDS of a workgroup */
    int64_t peak_bytes;                    /* most device memory the call held at once */
    double ms_score, ms_trace;             /* HIP events: the score pass; fill and walk of the trace pass, summed over the batches */
    int64_t n_shifted;                     /* aligned contigs with at least one short or long codon */
} mgta_frameshift_stats;
int mgta_seqs_frameshift(mgta_ctx *, const char *nucl, const uint64_t *offsets /* [n + 1] */, int64_t n,
                         const char *refs, const uint64_t *ref_offsets /* [n_ref + 1] */, int64_t n_ref,
                         const int8_t *sub /* [27 * 27] */, int32_t gap_open, int32_t gap_extend, int32_t frameshift,
                         mgta_frameshift_rec *recs /* [n] */, int32_t *scores /* [n * n_ref] or NULL; INT32_MIN = no score */,
                         char *path /* [offsets[n] + n * 4096] or NULL */, int32_t *path_len /* [n] or NULL */,
                         mgta_frameshift_stats *stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------------
 * Contigs that two references explain better than one (the place of the chimera removal in the reference's bin/post_proc.sh:89-95,
 * which runs `uchime` on the representatives; that tool is not part of the reference, and the rule below is this library's own: it is
 * not uchime's and is not checked against it).  Needs no graph.  Contigs, references, residue classes, sub, gap_open and gap_extend
 * are those of mgta_seqs_nearest, and score(x, y) is exactly its score: global in x, local in y, int32, or undefined.  Two more
 * parameters: min_seg, 1 <= min_seg <= 4096, the fewest residues on either side of a break, and min_gain, 1 <= min_gain <= 2^20.
 * For a contig x of L residues and a reference r:   P_r(b) = score(x[1..b], y_r),   S_r(b) = score(x[b..L], y_r).
 * A breakpoint b means left = x[1..b], right = x[b+1..L]; b is in range when min_seg <= b <= L - min_seg.
 *   1. Top two.  P1(b): the reference with the highest defined P_r(b), the lowest index on a tie; P2(b): the same choice among the
 *                other references; S1(b), S2(b) likewise from S_r(b).  Any of the four may be absent.
 *   2. The pair. If P1(b) and S1(b+1) name different references, the pair at b is (P1(b), S1(b+1)).  Otherwise the candidates are
 *                (P1(b), S2(b+1)) and (P2(b), S1(b+1)), each only when both members exist; of two the larger sum wins, the first
 *                on a tie; with no candidate there is no pair at b.  two(b) is the pair's sum.
 *   3. The break. b* = the lowest b in range whose two(b) is the maximum; A and B are its left and right reference (A != B).
 *   4. One parent. N = P1(L), the nearest reference.  one = max( P_N(L), max over r in {N, A, B} and over b in range with both terms
 *                defined of P_r(b) + S_r(b+1) ): a single parent gets the free jump at the break that two parents get, so a contig
 *                with a plain insertion or deletion against every reference does not gain its own gap cost.
 *   5. Verdict.  gain = two(b*) - one.  status 1 (chimeric) when gain >= min_gain, else 0 (clean).  status 2 (unchecked) when no b in
 *                range has a pair: L < 2 * min_seg, fewer than two references that score, an empty contig or reference set.  An
 *                unchecked record keeps ref and score when N exists, else they are -1 and 0; its other fields are 0 and left_ref =
 *                right_ref = -1.
 *   Record.      status; ref, score: N and P_N(L) (-1, 0 without N); brk: b*; left_ref, left_score, right_ref, right_score: the
 *                pair at b*; two, one, gain.
 *   Range.       As for mgta_seqs_nearest a defined score is below 2^24 in size (127 * 4096 + 1024 * 8192); two and one are sums of
 *                two such values and gain is their difference: all below 2^26, nothing leaves int32.  The kernels hold
 *                "undefined" as that function's sentinel -2^30 with its floor -2^29; what derives from it stays within 9.7e6 of it.
 * tops, when given, takes the top two of every row (the tests' view): for row b of contig c, at (offsets[c] + b - 1) * 8, P1.score,
 * P1.ref, P2.score, P2.ref, S1.score, S1.ref, S2.score, S2.ref, the S entries for the suffix that STARTS at b; an absent entry is
 * INT32_MIN, -1.  Two passes on the device, one kernel: the top-two pass, a lane per contig row, a wave along the concatenation of
 * the references in both directions (the suffix pass runs over the reversed contig and the reversed references), the row's maximum
 * over the current reference and its top two in registers; then the parents pass over N, A, B of every contig that has a pair, which
 * writes the rows' maxima out.  Steps 2 to 5 are O(L) per contig and run on the host.  Every output is a function of the inputs only,
 * except stats.ms_*, the counters of work done and the residency fields; mgta_ctx_set_chimera_segment (reference columns of one
 * segment of the run, cut at reference boundaries; 0 = the library's choice) and mgta_ctx_set_chimera_groups (work items a (contig,
 * direction) is cut into, each a run of consecutive segments, at most one per segment; 0 = by the number of contigs) are switches
 * for tests and move no output.  Limits and
 * errors are those of mgta_seqs_nearest: L <= 4096, R <= 4096, n < 2^31, n_ref < 2^31, fewer than 2^31 reference residues in all;
 * beyond any of them, or with min_seg / min_gain / gap parameters out of range, MGTA_EINVAL names the limit and nothing is written.
 * MGTA_EINVAL also: NULL context; with n > 0 NULL offsets / recs / sub / ref_offsets (n_ref > 0) / seqs or refs with residues; n < 0,
 * n_ref < 0, descending offsets on either side.  n = 0: MGTA_OK, stats all zero.  Device memory: the letters of both sides twice, 16
 * bytes per (row, direction, group of segments), 8 bytes per column of the longest segment for every resident wave (at most 4096 of them)
 * when a contig has more than 64 residues, 24 bytes per row and 56 bytes per contig of the parents pass, which reads the references
 * where they lie, accounted like every other buffer; what does not fit is MGTA_ENOMEM.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_chimera_rec { int32_t status, ref, score, brk, left_ref, left_score, right_ref, right_score, two, one, gain; } mgta_chimera_rec;
typedef struct mgta_chimera_stats {
    int64_t n_seqs, n_refs, n_clean, n_chimeric, n_unchecked;
    int64_t n_cells;                       /* cells of the top-two pass: 2 * sum of L * R over all pairs (INT64_MAX when it does not fit) */
    int64_t n_parent_cells;                /* cells of the parents pass */
    int64_t n_items, n_parent_items;       /* work items (contig, direction, group of segments) of the two passes */
    int64_t n_segments;                    /* runs of whole references the concatenation is cut into */
    int64_t n_groups;                      /* groups of consecutive segments: 1 when the contigs fill the device */
    int64_t grid_blocks;                   /* workgroups of the top-two pass */
    int64_t waves_per_block;               /* items in flight per workgroup */
    int64_t blocks_per_cu;                 /* what the runtime answered for the kernel, at most 4 */
    int64_t lds_bytes;                     /* LDS of a workgroup: sub */
    int64_t bound_bytes;                   /* the boundary buffers of all resident waves: 8 B per column of the longest segment each (0 when no contig has more than 64 residues) */
    int64_t peak_bytes;                    /* most device memory the call held at once */
    double ms_top, ms_parents;             /* HIP events: the top-two pass with its fold; the parents pass */
} mgta_chimera_stats;
int mgta_seqs_chimera(mgta_ctx *, const char *seqs, const uint64_t *offsets /* [n + 1] */, int64_t n,
                      const char *refs, const uint64_t *ref_offsets /* [n_ref + 1] */, int64_t n_ref,
                      const int8_t *sub /* [27 * 27] */, int32_t gap_open, int32_t gap_extend, int32_t min_seg, int32_t min_gain,
                      mgta_chimera_rec *recs /* [n] */, int32_t *tops /* [offsets[n] * 8] or NULL */, mgta_chimera_stats *stats /* may be NULL */);
int mgta_ctx_set_chimera_segment(mgta_ctx *, int64_t columns);   /* 0 = chosen by the library; a switch for tests, the outputs do not move */
int mgta_ctx_set_chimera_groups(mgta_ctx *, int64_t groups);     /* 0 = by the number of contigs; a switch for tests, the outputs do not move */

/* ------------------------------------------------------------------------------------------------
 * Seed finder (replaces the read scan of `megagta findstart`, fast_kmer_filter.cpp:108-176,193-215):
 * every window of k nucleotides (k a multiple of 3, k/3 <= 24) of every read, on both strands, whose translation is one of
 * the n_ref reference words.  A word = its residues in the code of prot_kmer.h:31-43 (ARNDCQEGHILKMFPSTWYV = 0..19, '*' = 20),
 * 5 bits each, first residue highest: ref_words[2i] = the first min(12, k/3) residues, ref_words[2i+1] = the rest
 * (kmer.h:66-84); of equal words the first one wins (insert_unique, fast_kmer_filter.cpp:88).
 * reads_reversed: the reads were uploaded reversed, as mgta_sdbg_build wants them (cx1_read2sdbg_s1.cpp:97) — one upload serves
 * both.  A hit names the read, the strand (0 = as sequenced, 1 = reverse complement), the window start inside that strand's
 * string (ProcessSequenceMulti's nucl_pos) and the reference word.  At most `cap` hits are stored; *n_hits is the number found
 * (call again with a larger buffer when it exceeds cap).  Order of the hits is unspecified (the reference shuffles its output).
 * ---------------------------------------------------------------------------------------------- */
typedef struct mgta_seed_hit {
    uint64_t read;
    uint32_t pos_strand;             /* window start << 1 | strand */
    int32_t ref;                     /* index into ref_words */
} mgta_seed_hit;
int mgta_findstart(mgta_ctx *, const mgta_reads *reads, int reads_reversed, int k, const uint64_t *ref_words, int64_t n_ref,
                   mgta_seed_hit *hits, int64_t cap, int64_t *n_hits, double *ms_kernel /* optional */);

/* ------------------------------------------------------------------------------------------------
 * `megagta denovo` on a loaded graph (multi-k runs: the contigs of k feed `buildgraph --assist_seq` of the next k and `findstart`):
 * RemoveTips (assembly_algorithms.cpp:76-183), PopBubbles (:245-301, branch_group.cpp:22-141), then the maximal simple paths
 * written as contigs (main_assemble, assembler.cpp:98-167; UnitigGraph::InitFromSdBG with a file, unitig_graph.cpp:80-150,208-303).
 * The reference's loops race between threads; the result here is that of its ONE-thread run, byte for byte, computed in parallel
 * on the device (see denovo.hip).  CONSUMES the validity bits of the graph (as the reference does): do not search it afterwards.
 * max_tip_len: -1 = 2k, 0 = keep tips; min_contig: shortest contig written (the driver passes the next k + 1).
 * *fasta receives the malloc'd text of PREFIX.contigs.fa (">k{K}_{id} flag={f} multi={%.4lf} len={L}\n{seq}\n" per contig, ids in
 * ascending end-edge order = the one-thread order); free it with mgta_host_free.  PREFIX.contigs.fa.info is "n_contigs total_len\n".
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_denovo_stats {
    int64_t n_tips, n_bubbles;               /* what the reference logs: tips removed, bubbles popped */
    int64_t n_bubble_candidates, n_bubble_rounds;
    int64_t n_paths, n_unitig_sweeps;
    int64_t n_contigs, total_len;
    float ms_tips, ms_bubbles, ms_unitigs;
} mgta_denovo_stats;
int mgta_denovo(mgta_sdbg *, int max_tip_len, int no_bubble, int min_contig, char **fasta, uint64_t *fasta_len,
                mgta_denovo_stats *stats /* optional */);
void mgta_host_free(void *);

/* ------------------------------------------------------------------------------------------------
 * Profile HMM tables (parsed on the host exactly like Parser::readHMM, hmmer3b_parser.h:19-177;
 * heuristic like MostProbablePath, most_probable_path.h:48-118)
 * ------------------------------------------------------------------------------------------------ */
int mgta_hmm_load(mgta_ctx *, int M, int A, const double *msc /* [(M+1)*A] */, const double *tsc /* [7*(M+1)] */,
                  const double *max_match /* [M+1] */, const double *h /* [3*(M+1)] */,
                  const int32_t *alpha /* [127] residue letter -> column */, mgta_hmm **out);
void mgta_hmm_free(mgta_hmm *);

/* ------------------------------------------------------------------------------------------------
 * Batched HMM-guided A* (replaces the OMP seed loop of search(): search.cpp:184-189,
 * HMMGraphSearch::search/astarSearch: hmm_graph_search.h:60-343, NodeEnumerator::enumerateNodes:
 * node_enumerator.h:65-246)
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgta_astar_side {
    int32_t ok, fval, length, state_no, state, partial;
    int64_t node_id, n_closed, n_expanded, n_opened;
    double real_score, score;
} mgta_astar_side;

typedef struct mgta_astar_stats {
    int64_t n_seeds, n_expansions, n_opened, n_retries;   /* n_retries: searches run again because the pool was exhausted (normally 0): by
                                                           * the host after the pass (independent searches) or in place (ordered window) */
    double ms_total, ms_kernel;
    int64_t n_grown, n_rehash, n_recycled;                /* searches that outgrew their base arena, hash tables re-built, chunks re-used */
    uint64_t pool_bytes, pool_used;                       /* device memory set aside for the searches / most of it in use at once */
    int64_t n_resumes;                                    /* ordered window only: passes that gave up (the lowest running search outgrew its
                                                           * reserve) and were resumed behind the commit frontier (normally 0) */
    uint64_t reserve_bytes, reserve_used;                 /* the lowest running search's reserve (last pass) / most of it ever in use */
    int64_t max_search_nodes, max_search_expansions;      /* the largest single search of the batch: nodes opened, nodes expanded */
    int64_t order_abandoned;                              /* ordered window only, and only with MEGAGTA_SEARCH_ALLOW_UNORDERED=1 in the environment: 1 = the
                                                           * searches in flight outgrew the pool and the batch went on sharing its paths WITHOUT an order
                                                           * (the reference's multi-thread behaviour); by default the order is held whatever it costs */
    int64_t n_cache_drops;                                /* shared-cache inserts that found no room within the probe limit (0 in every measured run;
                                                           * > 0: later seeds may have searched where they could have followed a cached path) */
    int64_t hmm_in_lds;                                   /* 1: the HMM tables were staged in LDS; 0: (M + 1)(A + 11) * 8 B beside the heap tops
                                                           * exceed the CU's 160 KB (models longer than ~400 columns): read from device memory */
    int64_t n_over_limit;                                 /* search sides that outgrew the page limit (2 GB per array, ~33 M nodes, unless
                                                           * mgta_ctx_set_search_page_limit set another) and are reported as failed searches
                                                           * (ok = 0, no extension); each is named on stderr, and the count is on the per-gene "Done"
                                                           * line of `megagta search` and of search_dist.py (rank 0's).  0 in every measured run */
    double ms_queue_drained;                              /* first pass: milliseconds from the kernel's start to the moment the last seed of the batch was
                                                           * TAKEN by a search slot; ms_kernel - ms_queue_drained = the tail in which the launch only finishes
                                                           * the searches in flight (a batch cannot end before its longest search does) */
} mgta_astar_stats;

/* sink gets one call per seed, in seed order: left (already reverse-complemented) + right halves. */
typedef int (*mgta_contig_sink)(void *user, int64_t seed_index, const char *left, int64_t left_len,
                                const char *right, int64_t right_len, const mgta_astar_side *right_side,
                                const mgta_astar_side *left_side);

/* kmers: n x (k+1) characters ACGT (any case), start_state[i] = model position - 1 (search.cpp:157).
 * cache_mode 0 = cold: every seed independent (empty term_nodes caches), embarrassingly parallel;
 * cache_mode B >= 1 = shared term_nodes caches (search.cpp:182) with an ordered-commit window: the search of seed j
 *   sees exactly the paths found by seeds <= j - B, whatever the scheduling.  B = 1 is the reference's sequential
 *   run (`search ... 1`, bit-identical FASTA); larger B trades that equivalence for up to B searches in flight per
 *   direction while staying deterministic. */
int mgta_astar_batch(mgta_sdbg *, const mgta_hmm *fwd, const mgta_hmm *rev, const char *kmers,
                     const int32_t *start_state, int64_t n, int prune_len, double low_cov_penalty,
                     int cache_mode, mgta_contig_sink sink, void *user, mgta_astar_stats *stats);
/* cache_mode -1 = shared caches WITHOUT any ordering: every search sees whatever paths have been inserted when it looks (what the
 * reference's `search` with more than one thread does, search.cpp:182-189).  Least work and no waiting, but which of several equally
 * good paths a seed takes depends on timing: not the default anywhere; MEGAGTA_CACHE_WINDOW=-1 selects it in `megagta search`. */
/* The same batch run with the stream and the work memory of `run` (another context of the graph's device) instead of the graph's own:
 * two host threads can search two genes of one gene_list side by side on one graph (search.cpp:124 loops over the genes one after the
 * other).  mgta_ctx_set_search_share(run, 1, 2) on both contexts gives each batch half of the CUs.  Results do not depend on it.
 * (Measured on two genes of 76 k / 103 k seeds: no faster than one after the other -- `megagta search` keeps the genes sequential
 * unless MEGAGTA_SEARCH_LANES=2.) */
int mgta_astar_batch_on(mgta_ctx *run, mgta_sdbg *, const mgta_hmm *fwd, const mgta_hmm *rev, const char *kmers,
                        const int32_t *start_state, int64_t n, int prune_len, double low_cov_penalty,
                        int cache_mode, mgta_contig_sink sink, void *user, mgta_astar_stats *stats);
/* The same batch with its results in flat arrays instead of one call-back per seed: contig i = (*contigs)[offsets[i] .. offsets[i + 1]) =
 * left + lower-cased seed k-mer (k + 1 characters) + right, the sequence line `search` writes (hmm_graph_search.h:60-81).  *contigs is
 * malloc'd (mgta_host_free); offsets [n + 1] and sides [2 n] (right, left per seed; may be NULL) are the caller's. */
int mgta_astar_batch_packed(mgta_sdbg *, const mgta_hmm *fwd, const mgta_hmm *rev, const char *kmers, const int32_t *start_state, int64_t n,
                            int prune_len, double low_cov_penalty, int cache_mode, char **contigs, uint64_t *offsets, mgta_astar_side *sides,
                            mgta_astar_stats *stats);
int mgta_ctx_set_search_share(mgta_ctx *, int num, int den);     /* this context's search batches use num/den of the CUs (default 1/1) */

/* ---- measurement: the device's random 128-byte line ceiling -------------------------------------------------------------------------
 * Not part of the reference's interface: the yardstick the search's roofline is priced against (bench.py `search.roofline`).  The A*
 * expansion (hmm_graph_search.h:191-343) and the succinct-graph walks under it (succinct_dbg.cpp:78-97, rank_and_select.h:153-280)
 * are chains of random 128-byte line reads.  Every configuration is run once over a table of `table_bytes` (>= 8 GB to leave every
 * cache behind) with the kernels' own access shape: groups of 8 lanes read one aligned line each (16 B per lane); a wavefront carries
 * `groups` groups, each with `unroll` independent lines in flight, `waves_per_cu` wavefronts per CU.  dependent = 1 chases pointers
 * (the next line's index is read from the line just fetched): ns_per_step is then the loaded latency of one dependent line;
 * dependent = 2: the same chase with a store to another random line in every step (a store in front of a dependent fetch): 16 bytes
 * per lane = the whole line; dependent = 3: one lane's 16 bytes = a partial line.
 * In: waves_per_cu 1..32, groups 1..8, unroll 1|2|4|8, dependent 0..3, steps >= 1.  Out: the rest. */
typedef struct mgta_line_probe {
    int32_t waves_per_cu, groups, unroll, dependent;
    uint64_t steps;                  /* line reads per group and chain */
    int32_t lines_in_flight_per_cu, pad_;
    uint64_t lines;                  /* lines read by the launch */
    double ms, gb_per_s, ns_per_step;
} mgta_line_probe;
int mgta_probe_random_lines(mgta_ctx *, uint64_t table_bytes, mgta_line_probe *cfg, int n_cfg);

#ifdef __cplusplus
}
#endif
#endif /* MEGAGTA_HIP_H_ */
