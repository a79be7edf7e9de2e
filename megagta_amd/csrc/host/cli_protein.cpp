// cli_protein.cpp — the protein post-processing of a gene's contigs (the steps of bin/post_proc.sh on the device): derep, align,
// posterior, cluster, clustertree, nearest, chimera.  None needs a graph; every argument is checked before a device is opened.  The file
// formats are this project's own (INTEGRATION.md 2i .. 2m); the Python formatters of megagta_amd/ print the same bytes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "cli.hpp"
#include "../frameshift_seq.hpp"

namespace mgta_cli {
// a device call has refused its input: the [ERROR] line of the command, and its exit code
static int nothing_written(const char *who, mgta_ctx *ctx) {
    fprintf(stderr, "    [ERROR] %s: %s: nothing written\n", who, mgta_last_error());
    ctx_put(ctx);
    return 1;
}

// ---- derep: the unique, non-contained records of a gene's protein contigs, and the nucleotide records they select ("get the unique
// merged contigs", bin/post_proc.sh:50-55,84-85).  Formats: INTEGRATION.md 2i.
int main_derep(int argc, char **argv) {
    if (argc != 3 && argc != 5) { fprintf(stderr, "Usage: megagta derep <prot.fasta> <out_prefix> [<nucl.fasta> <nucl_out_prefix>]\n"); return 1; }
    RssLine rss;
    const std::string fasta = argv[1], out_prefix = argv[2];
    const FastaRecords in = read_fasta(fasta, true);
    const int64_t n = in.n();
    FastaRecords nucl;
    if (argc == 5 && !read_paired("derep", in, fasta, argv[3], nucl)) return 1;
    const double t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    std::vector<uint8_t> status((size_t)n + 1);
    std::vector<int64_t> rep((size_t)n + 1);
    std::vector<uint32_t> copies((size_t)n + 1);
    mgta_derep_stats st;
    if (mgta_seqs_derep(ctx, in.seqs.data(), in.offsets.data(), n, status.data(), rep.data(), copies.data(), &st) != MGTA_OK) die("mgta_seqs_derep: %s", mgta_last_error());
    logf("derep of %lld records, %lld letters: %lld kept, %lld duplicate, %lld contained; anchor %lld, %lld windows, %lld comparisons; duplicates %.1f ms, table %.1f ms, "
         "walks %.1f ms; wall %.3f s", (long long)st.n_seqs, (long long)st.n_letters, (long long)st.n_kept, (long long)st.n_duplicates, (long long)st.n_contained,
         (long long)st.anchor_len, (long long)st.n_windows, (long long)st.n_compares, st.ms_dups, st.ms_table, st.ms_verify, now_s() - t0);
    static const char *kStatus[3] = {"kept", "duplicate", "contained"};
    std::string kept, map, nkept;
    for (size_t u = 0; u < (size_t)n; ++u) {
        map += in.names[u] + "\t" + kStatus[status[u]] + "\t" + (status[u] == 2 ? std::string("-") : in.names[(size_t)rep[u]]) + "\t" + std::to_string(copies[u]) + "\n";
        if (status[u] != 0) continue;
        in.append_record(kept, u);
        if (argc == 5) nucl.append_record(nkept, u);
    }
    write_or_die(out_prefix + "_rmdup.fasta", kept);
    write_or_die(out_prefix + "_rmdup_map.txt", map);
    if (argc == 5) write_or_die(std::string(argv[4]) + "_rmdup.fasta", nkept);
    ctx_put(ctx);
    return 0;
}

// ---- align: the records of a gene's protein contigs placed on the columns of the gene's profile HMM (the place of `hmmalign` in
// bin/post_proc.sh:65; the rule is mgta_seqs_align's own).  Needs no graph and leaves a worker's resident graphs alone.  Formats: INTEGRATION.md 2j.
int main_align(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "Usage: megagta align <model.hmm> <prot.fasta> <out_prefix>\n"); return 1; }
    RssLine rss;
    const std::string fasta = argv[2], out_prefix = argv[3];
    const FastaRecords in = read_fasta(fasta, true);
    const int64_t n = in.n();
    const double t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    int columns = 0;
    mgta_hmm *hm = upload_hmm(ctx, argv[1], &columns);
    const size_t M = (size_t)columns;
    std::vector<mgta_align_rec> recs((size_t)n + 1);
    std::vector<uint8_t> cols((size_t)n * M + 1);
    std::vector<char> path(in.seqs.size() + (size_t)n * M + 1);
    std::vector<int32_t> plen((size_t)n + 1);
    mgta_align_stats st;
    if (mgta_seqs_align(ctx, hm, in.seqs.data(), in.offsets.data(), n, recs.data(), cols.data(), path.data(), plen.data(), &st) != MGTA_OK)
        die("mgta_seqs_align: %s", mgta_last_error());
    logf("align of %lld records to %zu columns: %lld aligned, %lld unaligned; %lld cells in %lld batches, %lld workgroups of %lld waves, %lld per CU, %lld B of LDS, match "
         "scores in %s; fill %.1f ms, trace %.1f ms; wall %.3f s", (long long)st.n_seqs, M, (long long)st.n_aligned, (long long)st.n_unaligned, (long long)st.n_cells,
         (long long)st.n_batches, (long long)st.grid_blocks, (long long)st.waves_per_block, (long long)st.blocks_per_cu, (long long)st.lds_bytes,
         st.msc_in_lds ? "LDS" : "device memory", st.ms_fill, st.ms_trace, now_s() - t0);
    std::string fa, table = "#contig\tlen\tstatus\tscore\tmodel_from\tmodel_to\tmatch\tinsert\tdelete\n";
    char num[64];
    for (size_t u = 0; u < (size_t)n; ++u) {
        const mgta_align_rec &r = recs[u];
        const char *x = in.seqs.data() + in.offsets[u];
        const uint8_t *row = cols.data() + u * M;
        fa += ">" + in.headers[u] + "\n";
        if (r.status != 0) fa.append(M, '-');
        else {
            const char *p = path.data() + in.offsets[u] + u * M;
            size_t xi = 0, j = (size_t)r.model_from - 1;
            fa.append((const char *)row, j);
            for (int32_t s = 0; s < plen[u]; ++s) {
                if (p[s] == 'I') { const char c = x[xi++]; fa += (c >= 'A' && c <= 'Z') ? (char)(c + 32) : c; }
                else { fa += (char)row[j++]; xi += p[s] == 'M'; }
            }
            fa.append((const char *)row + j, M - j);
        }
        fa += "\n";
        if (r.status != 0) snprintf(num, sizeof num, "-inf");
        else snprintf(num, sizeof num, "%.4f", r.score);
        table += in.names[u] + "\t" + std::to_string(in.offsets[u + 1] - in.offsets[u]) + "\t" + (r.status ? "unaligned" : "aligned") + "\t" + num + "\t" +
                 std::to_string(r.model_from) + "\t" + std::to_string(r.model_to) + "\t" + std::to_string(r.n_match) + "\t" + std::to_string(r.n_insert) + "\t" +
                 std::to_string(r.n_delete) + "\n";
    }
    mgta_hmm_free(hm);
    write_or_die(out_prefix + "_aligned.fasta", fa);
    write_or_die(out_prefix + "_aligned.txt", table);
    ctx_put(ctx);
    return 0;
}

// ---- posterior: the Forward score of a gene's protein contigs on the gene's profile HMM and the posterior of every residue on the path
// `align` gives it (mgta_seqs_align for the path, then mgta_seqs_posterior; the rule and the PP code are this project's own).  Needs no
// graph and leaves a worker's resident graphs alone.  Formats: INTEGRATION.md 2j'.
static char pp_char(double p) {
    const double q = p + 0.05;
    return q >= 1.0 ? '*' : (char)('0' + (int)std::floor(q * 10.0));
}

int main_posterior(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "Usage: megagta posterior <model.hmm> <prot.fasta> <out_prefix>\n"); return 1; }
    RssLine rss;
    const std::string fasta = argv[2], out_prefix = argv[3];
    const FastaRecords in = read_fasta(fasta, true);
    const int64_t n = in.n();
    const double t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    int columns = 0;
    mgta_hmm *hm = upload_hmm(ctx, argv[1], &columns);
    const size_t M = (size_t)columns;
    std::vector<mgta_align_rec> recs((size_t)n + 1);
    std::vector<uint8_t> cols((size_t)n * M + 1);
    std::vector<char> path(in.seqs.size() + (size_t)n * M + 1);
    std::vector<int32_t> plen((size_t)n + 1);
    mgta_align_stats ast;
    if (mgta_seqs_align(ctx, hm, in.seqs.data(), in.offsets.data(), n, recs.data(), cols.data(), path.data(), plen.data(), &ast) != MGTA_OK)
        die("mgta_seqs_align: %s", mgta_last_error());
    // the label of every residue: the state of the path that emitted it (0 for the residues of an unaligned record)
    std::vector<int32_t> labels(in.seqs.size() + 1, 0);
    for (size_t u = 0; u < (size_t)n; ++u) {
        if (recs[u].status != 0) continue;
        const char *p = path.data() + in.offsets[u] + u * M;
        int32_t j = recs[u].model_from - 1;
        uint64_t r = in.offsets[u];
        for (int32_t s = 0; s < plen[u]; ++s) {
            if (p[s] == 'M') labels[r++] = ++j;
            else if (p[s] == 'I') labels[r++] = -j;
            else ++j;
        }
    }
    std::vector<mgta_post_rec> post((size_t)n + 1);
    std::vector<double> pp(in.seqs.size() + 1, 0.0);
    mgta_post_stats st;
    if (mgta_seqs_posterior(ctx, hm, in.seqs.data(), in.offsets.data(), n, labels.data(), post.data(), pp.data(), nullptr, nullptr, &st) != MGTA_OK)
        die("mgta_seqs_posterior: %s", mgta_last_error());
    logf("posterior of %lld records on %zu columns: %lld scored, %lld unaligned; %lld cells in %lld batches, %lld workgroups of %lld waves, %lld per CU, %lld B of LDS, "
         "match scores in %s; peak %lld B; forward %.1f ms, backward %.1f ms; wall %.3f s", (long long)st.n_seqs, M, (long long)st.n_scored, (long long)st.n_unaligned,
         (long long)st.n_cells, (long long)st.n_batches, (long long)st.workgroups, (long long)st.waves_per_block, (long long)st.blocks_per_cu, (long long)st.lds_bytes,
         st.msc_in_lds ? "LDS" : "device memory", (long long)st.peak_bytes, st.ms_forward, st.ms_backward, now_s() - t0);
    std::string fa, table = "#contig\tlen\tstatus\tfwd_nats\tfwd_bits\tviterbi\tmean_pp\tmin_pp\tn_below_half\n";
    char num[256];
    for (size_t u = 0; u < (size_t)n; ++u) {
        const bool un = post[u].status != 0 || recs[u].status != 0;
        const uint64_t L = in.offsets[u + 1] - in.offsets[u];
        const double *q = pp.data() + in.offsets[u];
        fa += ">" + in.headers[u] + "\n";
        if (un) fa.append(M, '.');
        else {
            const char *p = path.data() + in.offsets[u] + u * M;
            size_t xi = 0, j = (size_t)recs[u].model_from - 1;
            fa.append(j, '.');
            for (int32_t s = 0; s < plen[u]; ++s) {
                if (p[s] == 'D') { fa += '.'; ++j; }
                else { fa += pp_char(q[xi++]); j += p[s] == 'M'; }
            }
            fa.append(M - j, '.');
        }
        fa += "\n";
        table += in.names[u] + "\t" + std::to_string(L) + "\t";
        if (un) table += "unaligned\t-inf\t-inf\t-inf\t0.0000\t0.0000\t0\n";
        else {
            double total = 0.0, low = q[0];
            long long below = 0;
            for (uint64_t r = 0; r < L; ++r) {
                total += q[r];
                if (q[r] < low) low = q[r];
                below += q[r] < 0.5;
            }
            snprintf(num, sizeof num, "scored\t%.4f\t%.4f\t%.4f\t%.4f\t%.4f\t%lld\n", post[u].fwd, post[u].fwd / 0.6931471805599453, recs[u].score, total / (double)L, low,
                     below);
            table += num;
        }
    }
    mgta_hmm_free(hm);
    write_or_die(out_prefix + "_posterior.txt", table);
    write_or_die(out_prefix + "_aligned_pp.fasta", fa);
    ctx_put(ctx);
    return 0;
}

// ---- cluster: complete-linkage clusters of a gene's aligned protein contigs, their representatives and the nucleotide records those select
// ("cluster at 99% aa identity", bin/post_proc.sh:57-85; the rule is mgta_rows_cluster's own).  Needs no graph and leaves a worker's resident
// graphs alone.  Formats: INTEGRATION.md 2k.
struct ClusterInput {
    std::string fasta;
    FastaRecords prot, nucl_recs;                                        // prot.seqs: the A2M lines
    std::string rows;
    std::vector<int64_t> lens;
    int64_t n = 0;
    size_t M = 1;
    bool nucl = false;
};
// the rows and lengths of <aligned.fasta> and, with a path, the nucleotide records that go with them; false after an [ERROR] line
static bool cluster_read(const char *who, const char *aligned, const char *nucl, ClusterInput &in) {
    in.fasta = aligned;
    in.prot = read_fasta(in.fasta, true);
    const int64_t n = in.n = in.prot.n();
    // the row of a record: its A2M line without the lower-case (inserted) residues; its length: the characters that are not '-'
    in.lens.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        const size_t before = in.rows.size();
        int64_t len = 0;
        for (uint64_t p = in.prot.offsets[(size_t)i]; p < in.prot.offsets[(size_t)i + 1]; ++p) {
            const char c = in.prot.seqs[p];
            len += c != '-';
            if (!(c >= 'a' && c <= 'z')) in.rows += c;
        }
        in.lens[(size_t)i] = len;
        if (i == 0) in.M = in.rows.size();
        if (in.rows.size() - before != in.M || in.M == 0) {
            fprintf(stderr, "    [ERROR] %s: record %lld (%s) of %s has %zu columns, the first record has %zu: nothing written\n", who, (long long)i,
                    in.prot.names[(size_t)i].c_str(), in.fasta.c_str(), in.rows.size() - before, in.M);
            return false;
        }
    }
    in.nucl = nucl != nullptr;
    return !nucl || read_paired(who, in.prot, in.fasta, nucl, in.nucl_recs);
}
// PREFIX_clust.txt, PREFIX_rep_seqs.fasta and, with the nucleotide records, NUCL_PREFIX_rep_seqs.fasta from the four outputs of a linkage
static void cluster_write(const ClusterInput &in, const int32_t *cluster, const int64_t *rep, const uint16_t *rep_diff, const uint16_t *rep_overlap,
                          const std::string &out_prefix, const std::string &nucl_prefix) {
    std::string table = "#contig\tstatus\tcluster\trep\tlen\tn_diff\tn_overlap\n", reps, nreps;
    for (size_t u = 0; u < (size_t)in.n; ++u) {
        const bool unaligned = cluster[u] < 0, is_rep = !unaligned && rep[u] == (int64_t)u;
        table += in.prot.names[u] + "\t" + (unaligned ? "unaligned" : is_rep ? "rep" : "member") + "\t" + (unaligned ? std::string("-") : std::to_string(cluster[u])) + "\t" +
                 (unaligned ? std::string("-") : in.prot.names[(size_t)rep[u]]) + "\t" + std::to_string(in.lens[u]) + "\t" + std::to_string(rep_diff[u]) + "\t" +
                 std::to_string(rep_overlap[u]) + "\n";
        if (!is_rep) continue;
        reps += ">" + in.prot.headers[u] + "\n";
        for (uint64_t p = in.prot.offsets[u]; p < in.prot.offsets[u + 1]; ++p) {
            const char c = in.prot.seqs[p];
            if (c != '-') reps += (c >= 'a' && c <= 'z') ? (char)(c - 32) : c;
        }
        reps += "\n";
        if (in.nucl) {
            in.nucl_recs.append_record(nreps, u);
        }
    }
    write_or_die(out_prefix + "_clust.txt", table);
    write_or_die(out_prefix + "_rep_seqs.fasta", reps);
    if (in.nucl) write_or_die(nucl_prefix + "_rep_seqs.fasta", nreps);
}

int main_cluster(int argc, char **argv) {
    if (argc != 5 && argc != 7) {
        fprintf(stderr, "Usage: megagta cluster <aligned.fasta> <out_prefix> <dist_cutoff> <min_overlap> [<nucl.fasta> <nucl_out_prefix>]\n");
        return 1;
    }
    RssLine rss;
    const std::string out_prefix = argv[2];
    char *end = nullptr;
    const double cutoff = strtod(argv[3], &end);
    if (end == argv[3] || *end) { fprintf(stderr, "    [ERROR] cluster: dist_cutoff '%s' is not a number\n", argv[3]); return 1; }
    long long min_overlap = 0;
    if (!int_arg("cluster", "min_overlap", argv[4], &min_overlap)) return 1;
    ClusterInput in;
    if (!cluster_read("cluster", argv[1], argc == 7 ? argv[5] : nullptr, in)) return 1;
    const int64_t n = in.n;
    const size_t M = in.M;
    const double t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    std::vector<int32_t> cluster((size_t)n + 1);
    std::vector<int64_t> rep((size_t)n + 1);
    std::vector<uint16_t> rep_diff((size_t)n + 1), rep_overlap((size_t)n + 1);
    mgta_cluster_stats st;
    if (mgta_rows_cluster(ctx, (const uint8_t *)in.rows.data(), in.lens.data(), n, (int64_t)M, min_overlap, cutoff, cluster.data(), rep.data(), rep_diff.data(),
                          rep_overlap.data(), &st) != MGTA_OK)
        return nothing_written("cluster", ctx);
    logf("cluster of %lld rows of %zu columns at %g, overlap >= %lld: %lld unaligned, %lld kept pairs, %lld components, %lld clusters (%lld singletons, largest %lld); "
         "%lld tiles, %lld workgroups at most, %lld per CU, %lld B of LDS, peak %lld B; pairs %.1f ms, linkage %.1f ms; wall %.3f s", (long long)st.n_rows, M, cutoff,
         min_overlap, (long long)st.n_unaligned, (long long)st.n_pairs_kept, (long long)st.n_components, (long long)st.n_clusters, (long long)st.n_singletons,
         (long long)st.largest_cluster, (long long)st.n_tiles, (long long)st.grid_blocks, (long long)st.blocks_per_cu, (long long)st.lds_bytes, (long long)st.peak_bytes,
         st.ms_pairs, st.ms_link, now_s() - t0);
    cluster_write(in, cluster.data(), rep.data(), rep_diff.data(), rep_overlap.data(), out_prefix, argc == 7 ? argv[6] : "");
    ctx_put(ctx);
    return 0;
}

// ---- clustertree: the clusters of `cluster` at several cut-offs from one pass over the pairs and one merge tree (mgta_rows_clusters), and the
// tree itself.  Per item of <c1,c2,...>, whose text is the tag: <out_prefix>_d<tag>_clust.txt, <out_prefix>_d<tag>_rep_seqs.fasta and
// <nucl_out_prefix>_d<tag>_rep_seqs.fasta, each what `cluster` writes at that cut-off; once: <out_prefix>_tree.txt.  Formats: INTEGRATION.md 2k'.
int main_clustertree(int argc, char **argv) {
    if (argc != 5 && argc != 7) {
        fprintf(stderr, "Usage: megagta clustertree <aligned.fasta> <out_prefix> <c1,c2,...> <min_overlap> [<nucl.fasta> <nucl_out_prefix>]\n");
        return 1;
    }
    RssLine rss;
    const std::string out_prefix = argv[2], list = argv[3];
    std::vector<std::string> tags;
    std::vector<double> cutoffs;
    for (size_t at = 0; at <= list.size();) {
        const size_t comma = std::min(list.find(',', at), list.size());
        const std::string item = list.substr(at, comma - at);
        at = comma + 1;
        const bool text_ok = !item.empty() && item.find_first_not_of("0123456789.") == std::string::npos && item.find_first_of("0123456789") != std::string::npos &&
                             std::count(item.begin(), item.end(), '.') <= 1;
        char *end = nullptr;
        const double c = text_ok ? strtod(item.c_str(), &end) : -1.0;
        if (!text_ok || *end || !(c >= 0.0 && c <= 1.0)) {
            fprintf(stderr, "    [ERROR] clustertree: cut-off '%s' is not a number in [0, 1] written with 0-9 and .\n", item.c_str());
            return 1;
        }
        for (size_t k = 0; k < cutoffs.size(); ++k)
            if (cutoffs[k] == c) { fprintf(stderr, "    [ERROR] clustertree: cut-offs '%s' and '%s' are the same number\n", tags[k].c_str(), item.c_str()); return 1; }
        tags.push_back(item);
        cutoffs.push_back(c);
    }
    long long min_overlap = 0;
    if (!int_arg("clustertree", "min_overlap", argv[4], &min_overlap)) return 1;
    ClusterInput in;
    if (!cluster_read("clustertree", argv[1], argc == 7 ? argv[5] : nullptr, in)) return 1;
    const int64_t n = in.n;
    const size_t K = cutoffs.size(), stride = (size_t)n;
    const double t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    std::vector<int32_t> cluster(K * stride + 1);
    std::vector<int64_t> rep(K * stride + 1);
    std::vector<uint16_t> rep_diff(K * stride + 1), rep_overlap(K * stride + 1);
    std::vector<mgta_tree_merge> merges((size_t)n + 1);
    int64_t n_merges = 0;
    mgta_tree_stats st;
    if (mgta_rows_clusters(ctx, (const uint8_t *)in.rows.data(), in.lens.data(), n, (int64_t)in.M, min_overlap, cutoffs.data(), (int64_t)K, cluster.data(), rep.data(),
                           rep_diff.data(), rep_overlap.data(), merges.data(), &n_merges, &st) != MGTA_OK)
        return nothing_written("clustertree", ctx);
    logf("clustertree of %lld rows of %zu columns at %zu cut-offs, overlap >= %lld: %lld kept pairs, %lld merges in %lld rounds, %lld lists rewritten, %lld entries "
         "visited, %lld cuts by the host linkage, peak %lld B; pairs %.1f ms, lists %.1f ms, rounds %.1f ms, cuts %.1f ms; wall %.3f s", (long long)st.n_rows, in.M, K,
         min_overlap, (long long)st.n_pairs, (long long)st.n_merges, (long long)st.n_rounds, (long long)st.n_lists_rewritten, (long long)st.n_entries_visited,
         (long long)st.n_cut_fallbacks, (long long)st.peak_bytes, st.ms_pairs, st.ms_build, st.ms_rounds, st.ms_cut, now_s() - t0);
    for (size_t k = 0; k < K; ++k)
        cluster_write(in, cluster.data() + k * stride, rep.data() + k * stride, rep_diff.data() + k * stride, rep_overlap.data() + k * stride, out_prefix + "_d" + tags[k],
                      argc == 7 ? std::string(argv[6]) + "_d" + tags[k] : "");
    std::string tree = "#a_row\tb_row\ta\tb\tn_diff\tn_overlap\n";
    for (int64_t m = 0; m < n_merges; ++m) {
        const mgta_tree_merge &t = merges[(size_t)m];
        tree += std::to_string(t.a) + "\t" + std::to_string(t.b) + "\t" + in.prot.names[(size_t)t.a] + "\t" + in.prot.names[(size_t)t.b] + "\t" + std::to_string(t.n_diff) + "\t" +
                std::to_string(t.n_overlap) + "\n";
    }
    write_or_die(out_prefix + "_tree.txt", tree);
    ctx_put(ctx);
    return 0;
}

// ---- nearest: for every record of a gene's protein contigs the closest sequence of the gene's reference set and the identity to it (the
// place of FrameBot / `AlignmentTool pairwise-knn`, bin/post_proc.sh:106-111; the rule is mgta_seqs_nearest's own).  Needs no graph and leaves
// a worker's resident graphs alone.  Formats: INTEGRATION.md 2l.
// `MATCH,MISMATCH`, or a matrix file in NCBI format (`#` comments, a header row of letters, rows `LETTER v v ...`; `*` is class 0; letters
// the file does not have take its lowest value) -> sub[27 * 27]; an empty string when it is good, else what is wrong with it
static std::string parse_scoring(const std::string &spec, int8_t *sub) {
    {
        long long a = 0, b = 0;
        char *e1 = nullptr, *e2 = nullptr;
        const size_t comma = spec.find(',');
        if (comma != std::string::npos && spec.find(',', comma + 1) == std::string::npos) {
            const std::string sa = spec.substr(0, comma), sb = spec.substr(comma + 1);
            a = strtoll(sa.c_str(), &e1, 10); b = strtoll(sb.c_str(), &e2, 10);
            if (!sa.empty() && !sb.empty() && !*e1 && !*e2) {
                if (a < -128 || a > 127 || b < -128 || b > 127) return "a value of '" + spec + "' is outside int8";
                for (int x = 0; x < 27; ++x)
                    for (int y = 0; y < 27; ++y) sub[x * 27 + y] = (int8_t)((x == y && x != 0) ? a : b);
                return "";
            }
        }
    }
    FILE *f = fopen(spec.c_str(), "r");
    if (!f) return "'" + spec + "' is neither MATCH,MISMATCH nor a matrix file that can be read";
    std::vector<int> cols;                                               // the class of every column, in file order
    std::vector<std::vector<long long>> rows;
    std::vector<int> row_cls;
    std::string err;
    char *line = nullptr;
    size_t cap = 0;
    ssize_t n;
    bool have_header = false;
    while (err.empty() && (n = getline(&line, &cap, f)) >= 0) {
        if (char *h = strchr(line, '#')) *h = 0;
        std::vector<std::string> fld;
        for (char *tok = strtok(line, " \t\r\n"); tok; tok = strtok(nullptr, " \t\r\n")) fld.emplace_back(tok);
        if (fld.empty()) continue;
        auto cls_of = [](const std::string &t) { return t.size() != 1 ? -1 : t[0] == '*' ? 0 : (residue_class((unsigned char)t[0]) ? residue_class((unsigned char)t[0]) : -1); };
        if (!have_header) {
            have_header = true;
            for (const std::string &t : fld) {
                const int c = cls_of(t);
                if (c < 0 || std::find(cols.begin(), cols.end(), c) != cols.end()) { err = "bad header row"; break; }
                cols.push_back(c);
            }
            continue;
        }
        const int c = cls_of(fld[0]);
        if (c < 0 || std::find(cols.begin(), cols.end(), c) == cols.end() || std::find(row_cls.begin(), row_cls.end(), c) != row_cls.end() ||
            fld.size() != cols.size() + 1) { err = "bad row " + fld[0]; break; }
        std::vector<long long> v;
        for (size_t k = 1; k < fld.size() && err.empty(); ++k) {
            char *e = nullptr;
            const long long x = strtoll(fld[k].c_str(), &e, 10);
            if (e == fld[k].c_str() || *e) err = "bad row " + fld[0];
            else if (x < -128 || x > 127) err = "a value of row " + fld[0] + " is outside int8";
            v.push_back(x);
        }
        row_cls.push_back(c); rows.push_back(v);
    }
    free(line);
    fclose(f);
    if (!err.empty()) return "matrix " + spec + ": " + err;
    if (cols.empty() || rows.size() != cols.size()) return "matrix " + spec + ": a header row of letters and one row per letter of it";
    long long lowest = 127;
    for (const auto &v : rows) for (long long x : v) lowest = std::min(lowest, x);
    for (int x = 0; x < 27 * 27; ++x) sub[x] = (int8_t)lowest;
    for (size_t r = 0; r < rows.size(); ++r)
        for (size_t k = 0; k < cols.size(); ++k) sub[row_cls[r] * 27 + cols[k]] = (int8_t)rows[r][k];
    return "";
}
// `nearest --frameshift`: the same place for the NUCLEOTIDE contigs, with shifts of the reading frame (the rule is mgta_seqs_frameshift's
// own).  Writes <out_prefix>_frameshift.txt, _corr_prot.fasta and _corr_nucl.fasta.  Formats: INTEGRATION.md 2l'.
static int nearest_frameshift(int argc, char **argv) {
    if (argc != 9) {
        fprintf(stderr, "Usage: megagta nearest --frameshift <cost> <ref.faa> <nucl.fasta> <out_prefix> <gap_open> <gap_extend> <scoring>\n");
        return 1;
    }
    RssLine rss;
    const std::string ref_fasta = argv[3], fasta = argv[4], out_prefix = argv[5];
    long long cost = 0, gap_open = 0, gap_extend = 0;
    if (!int_arg("nearest", "frameshift cost", argv[2], &cost)) return 1;
    if (cost < 0 || cost > 1024) { fprintf(stderr, "    [ERROR] nearest: frameshift cost = %lld: 0 <= cost <= 1024 is needed: nothing written\n", cost); return 1; }
    if (!int_arg("nearest", "gap_open", argv[6], &gap_open) || !int_arg("nearest", "gap_extend", argv[7], &gap_extend)) return 1;
    if (gap_extend < 0 || gap_extend > gap_open || gap_open > 1024) {
        fprintf(stderr, "    [ERROR] nearest: gap_open = %lld, gap_extend = %lld: 0 <= gap_extend <= gap_open <= 1024 is needed: nothing written\n", gap_open, gap_extend);
        return 1;
    }
    int8_t sub[27 * 27];
    const std::string bad = parse_scoring(argv[8], sub);
    if (!bad.empty()) { fprintf(stderr, "    [ERROR] nearest: scoring: %s: nothing written\n", bad.c_str()); return 1; }
    const FastaRecords in = read_fasta(fasta), ref = read_fasta(ref_fasta);
    const int64_t n = in.n(), n_ref = ref.n();
    const auto [refs, roffsets] = clean_references(ref);
    const double t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    std::vector<mgta_frameshift_rec> recs((size_t)n + 1);
    std::vector<char> path((size_t)in.seqs.size() + (size_t)n * 4096 + 1);
    std::vector<int32_t> path_len((size_t)n + 1);
    mgta_frameshift_stats st;
    if (mgta_seqs_frameshift(ctx, in.seqs.data(), in.offsets.data(), n, refs.data(), roffsets.data(), n_ref, sub, (int32_t)gap_open, (int32_t)gap_extend, (int32_t)cost,
                             recs.data(), nullptr, path.data(), path_len.data(), &st) != MGTA_OK)
        return nothing_written("nearest", ctx);
    logf("nearest with frameshifts of %lld records among %lld references: %lld unaligned, %lld shifted; %lld cells in %lld segments, %lld workgroups of %lld waves, "
         "%lld per CU, %lld B of LDS; %lld trace cells in %lld batches; peak %lld B; score %.1f ms, trace %.1f ms; wall %.3f s", (long long)st.n_seqs, (long long)st.n_refs,
         (long long)st.n_unaligned, (long long)st.n_shifted, (long long)st.n_cells, (long long)st.n_segments, (long long)st.grid_blocks, (long long)st.waves_per_block,
         (long long)st.blocks_per_cu, (long long)st.lds_bytes, (long long)st.n_trace_cells, (long long)st.n_batches, (long long)st.peak_bytes, st.ms_score, st.ms_trace,
         now_s() - t0);
    std::string table = "#contig\tstatus\tref\tscore\tidentity\tlen\tref_len\tref_from\tref_to\tmatch\tident\tinsert\tdelete\tshort\tlong\tshifts\n", prot, nucl;
    char num[64];
    mgta::Corrected corr;
    for (size_t u = 0; u < (size_t)n; ++u) {
        const mgta_frameshift_rec &r = recs[u];
        const bool un = r.status != 0;
        const int64_t cols = (int64_t)r.n_match + r.n_short + r.n_long + r.n_insert + r.n_delete;
        snprintf(num, sizeof num, "%.4f", cols ? (double)r.n_ident / (double)cols : 0.0);
        const size_t L = (size_t)(in.offsets[u + 1] - in.offsets[u]);
        std::string shifts = ".";
        if (!un) {
            if (!mgta::corrected_of(in.seqs.data() + in.offsets[u], L, path.data() + in.offsets[u] + u * 4096, (size_t)path_len[u], &corr)) {
                fprintf(stderr, "    [ERROR] nearest: record %s: its path does not consume its %zu nucleotides: nothing written\n", in.names[u].c_str(), L);
                ctx_put(ctx);
                return 1;
            }
            shifts = corr.shifts;
            prot += ">" + in.names[u] + "\n" + corr.prot + "\n";
            nucl += ">" + in.names[u] + "\n" + corr.nucl + "\n";
        }
        table += in.names[u] + "\t" + (un ? "unaligned" : "aligned") + "\t" + (un ? std::string("-") : ref.names[(size_t)r.ref]) + "\t" + std::to_string(r.score) + "\t" + num +
                 "\t" + std::to_string(L) + "\t" + std::to_string(un ? 0 : roffsets[(size_t)r.ref + 1] - roffsets[(size_t)r.ref]) + "\t" + std::to_string(r.ref_from) + "\t" +
                 std::to_string(r.ref_to) + "\t" + std::to_string(r.n_match) + "\t" + std::to_string(r.n_ident) + "\t" + std::to_string(r.n_insert) + "\t" +
                 std::to_string(r.n_delete) + "\t" + std::to_string(r.n_short) + "\t" + std::to_string(r.n_long) + "\t" + shifts + "\n";
    }
    write_or_die(out_prefix + "_frameshift.txt", table);
    write_or_die(out_prefix + "_corr_prot.fasta", prot);
    write_or_die(out_prefix + "_corr_nucl.fasta", nucl);
    ctx_put(ctx);
    return 0;
}
int main_nearest(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "--frameshift")) return nearest_frameshift(argc, argv);
    if (argc != 7) { fprintf(stderr, "Usage: megagta nearest <ref.faa> <prot.fasta> <out_prefix> <gap_open> <gap_extend> <scoring>\n"); return 1; }
    RssLine rss;
    const std::string ref_fasta = argv[1], fasta = argv[2], out_prefix = argv[3];
    long long gap_open = 0, gap_extend = 0;
    if (!int_arg("nearest", "gap_open", argv[4], &gap_open) || !int_arg("nearest", "gap_extend", argv[5], &gap_extend)) return 1;
    if (gap_extend < 0 || gap_extend > gap_open || gap_open > 1024) {
        fprintf(stderr, "    [ERROR] nearest: gap_open = %lld, gap_extend = %lld: 0 <= gap_extend <= gap_open <= 1024 is needed: nothing written\n", gap_open, gap_extend);
        return 1;
    }
    int8_t sub[27 * 27];
    const std::string bad = parse_scoring(argv[6], sub);
    if (!bad.empty()) { fprintf(stderr, "    [ERROR] nearest: scoring: %s: nothing written\n", bad.c_str()); return 1; }
    const FastaRecords in = read_fasta(fasta, true), ref = read_fasta(ref_fasta);
    const int64_t n = in.n(), n_ref = ref.n();
    const auto [refs, roffsets] = clean_references(ref);
    const double t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    std::vector<mgta_nearest_rec> recs((size_t)n + 1);
    mgta_nearest_stats st;
    if (mgta_seqs_nearest(ctx, in.seqs.data(), in.offsets.data(), n, refs.data(), roffsets.data(), n_ref, sub, (int32_t)gap_open, (int32_t)gap_extend, recs.data(), nullptr,
                          nullptr, nullptr, &st) != MGTA_OK)
        return nothing_written("nearest", ctx);
    logf("nearest of %lld records among %lld references: %lld unaligned; %lld cells in %lld segments, %lld workgroups of %lld waves, %lld per CU, %lld B of LDS; "
         "%lld trace cells in %lld batches; peak %lld B; score %.1f ms, trace %.1f ms; wall %.3f s", (long long)st.n_seqs, (long long)st.n_refs, (long long)st.n_unaligned,
         (long long)st.n_cells, (long long)st.n_segments, (long long)st.grid_blocks, (long long)st.waves_per_block, (long long)st.blocks_per_cu, (long long)st.lds_bytes,
         (long long)st.n_trace_cells, (long long)st.n_batches, (long long)st.peak_bytes, st.ms_score, st.ms_trace, now_s() - t0);
    std::string table = "#contig\tstatus\tref\tscore\tidentity\tlen\tref_len\tref_from\tref_to\tmatch\tident\tinsert\tdelete\n";
    std::string rtable = "#ref\tref_len\tcontigs\tmean_identity\n";
    std::vector<int64_t> count((size_t)n_ref + 1);
    std::vector<double> total((size_t)n_ref + 1);
    char num[64];
    for (size_t u = 0; u < (size_t)n; ++u) {
        const mgta_nearest_rec &r = recs[u];
        const bool un = r.status != 0;
        const int64_t cols = (int64_t)r.n_match + r.n_insert + r.n_delete;
        const double idy = cols ? (double)r.n_ident / (double)cols : 0.0;
        if (!un) { ++count[(size_t)r.ref]; total[(size_t)r.ref] += idy; }
        snprintf(num, sizeof num, "%.4f", idy);
        table += in.names[u] + "\t" + (un ? "unaligned" : "aligned") + "\t" + (un ? std::string("-") : ref.names[(size_t)r.ref]) + "\t" + std::to_string(r.score) + "\t" + num +
                 "\t" + std::to_string(in.offsets[u + 1] - in.offsets[u]) + "\t" + std::to_string(un ? 0 : roffsets[(size_t)r.ref + 1] - roffsets[(size_t)r.ref]) + "\t" +
                 std::to_string(r.ref_from) + "\t" + std::to_string(r.ref_to) + "\t" + std::to_string(r.n_match) + "\t" + std::to_string(r.n_ident) + "\t" +
                 std::to_string(r.n_insert) + "\t" + std::to_string(r.n_delete) + "\n";
    }
    for (int64_t r = 0; r < n_ref; ++r) {
        const size_t u = (size_t)r;
        snprintf(num, sizeof num, "%.4f", count[u] ? total[u] / (double)count[u] : 0.0);
        rtable += ref.names[u] + "\t" + std::to_string(roffsets[u + 1] - roffsets[u]) + "\t" + std::to_string(count[u]) + "\t" + num + "\n";
    }
    write_or_die(out_prefix + "_nearest.txt", table);
    write_or_die(out_prefix + "_nearest_refs.txt", rtable);
    ctx_put(ctx);
    return 0;
}

// ---- chimera: the records of a gene's protein contigs that two sequences of the gene's reference set explain better than one (the place
// of `uchime`, bin/post_proc.sh:89-95; the rule is mgta_seqs_chimera's own).  Needs no graph and leaves a worker's resident graphs alone.
// References and scoring are read as `nearest` reads them.  Formats: INTEGRATION.md 2m.
int main_chimera(int argc, char **argv) {
    if (argc != 9 && argc != 11) {
        fprintf(stderr, "Usage: megagta chimera <ref.faa> <prot.fasta> <out_prefix> <gap_open> <gap_extend> <scoring> <min_seg> <min_gain> [<nucl.fasta> <nucl_out_prefix>]\n");
        return 1;
    }
    RssLine rss;
    const std::string ref_fasta = argv[1], fasta = argv[2], out_prefix = argv[3];
    long long gap_open = 0, gap_extend = 0, min_seg = 0, min_gain = 0;
    if (!int_arg("chimera", "gap_open", argv[4], &gap_open) || !int_arg("chimera", "gap_extend", argv[5], &gap_extend) ||
        !int_arg("chimera", "min_seg", argv[7], &min_seg) || !int_arg("chimera", "min_gain", argv[8], &min_gain)) return 1;
    if (gap_extend < 0 || gap_extend > gap_open || gap_open > 1024) {
        fprintf(stderr, "    [ERROR] chimera: gap_open = %lld, gap_extend = %lld: 0 <= gap_extend <= gap_open <= 1024 is needed: nothing written\n", gap_open, gap_extend);
        return 1;
    }
    if (min_seg < 1 || min_seg > 4096) { fprintf(stderr, "    [ERROR] chimera: min_seg = %lld: 1 <= min_seg <= 4096 is needed: nothing written\n", min_seg); return 1; }
    if (min_gain < 1 || min_gain > (1 << 20)) { fprintf(stderr, "    [ERROR] chimera: min_gain = %lld: 1 <= min_gain <= 2^20 is needed: nothing written\n", min_gain); return 1; }
    int8_t sub[27 * 27];
    const std::string bad = parse_scoring(argv[6], sub);
    if (!bad.empty()) { fprintf(stderr, "    [ERROR] chimera: scoring: %s: nothing written\n", bad.c_str()); return 1; }
    const FastaRecords in = read_fasta(fasta, true), ref = read_fasta(ref_fasta);
    const int64_t n = in.n(), n_ref = ref.n();
    FastaRecords nucl;
    if (argc == 11 && !read_paired("chimera", in, fasta, argv[9], nucl)) return 1;
    const auto [refs, roffsets] = clean_references(ref);
    const double t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    std::vector<mgta_chimera_rec> recs((size_t)n + 1);
    mgta_chimera_stats st;
    if (mgta_seqs_chimera(ctx, in.seqs.data(), in.offsets.data(), n, refs.data(), roffsets.data(), n_ref, sub, (int32_t)gap_open, (int32_t)gap_extend, (int32_t)min_seg,
                          (int32_t)min_gain, recs.data(), nullptr, &st) != MGTA_OK)
        return nothing_written("chimera", ctx);
    logf("chimera check of %lld records among %lld references, min_seg %lld, min_gain %lld: %lld chimeric, %lld clean, %lld unchecked; %lld cells in %lld items, "
         "%lld segments in %lld groups, %lld workgroups of %lld waves, %lld per CU, %lld B of LDS, %lld B of boundary buffers; parents: %lld cells in %lld items; peak %lld B; "
         "top two %.1f ms, parents %.1f ms; wall %.3f s", (long long)st.n_seqs, (long long)st.n_refs, min_seg, min_gain, (long long)st.n_chimeric, (long long)st.n_clean,
         (long long)st.n_unchecked, (long long)st.n_cells, (long long)st.n_items, (long long)st.n_segments, (long long)st.n_groups, (long long)st.grid_blocks,
         (long long)st.waves_per_block, (long long)st.blocks_per_cu, (long long)st.lds_bytes, (long long)st.bound_bytes, (long long)st.n_parent_cells,
         (long long)st.n_parent_items, (long long)st.peak_bytes, st.ms_top, st.ms_parents, now_s() - t0);
    std::string table = "#contig\tstatus\tref\tscore\tlen\tbreak\tleft_ref\tleft_score\tright_ref\tright_score\ttwo\tone\tgain\n", kept, nkept;
    auto ref_name = [&](int32_t r) { return r < 0 ? std::string("-") : ref.names[(size_t)r]; };
    for (size_t u = 0; u < (size_t)n; ++u) {
        const mgta_chimera_rec &r = recs[u];
        table += in.names[u] + "\t" + (r.status == 0 ? "clean" : r.status == 1 ? "chimeric" : "unchecked") + "\t" + ref_name(r.ref) + "\t" + std::to_string(r.score) + "\t" +
                 std::to_string(in.offsets[u + 1] - in.offsets[u]) + "\t" + std::to_string(r.brk) + "\t" + ref_name(r.left_ref) + "\t" + std::to_string(r.left_score) + "\t" +
                 ref_name(r.right_ref) + "\t" + std::to_string(r.right_score) + "\t" + std::to_string(r.two) + "\t" + std::to_string(r.one) + "\t" +
                 std::to_string(r.gain) + "\n";
        if (r.status == 1) continue;
        in.append_record(kept, u);
        if (argc == 11) nucl.append_record(nkept, u);
    }
    write_or_die(out_prefix + "_chimera.txt", table);
    write_or_die(out_prefix + "_nochim.fasta", kept);
    if (argc == 11) write_or_die(std::string(argv[10]) + "_nochim.fasta", nkept);
    ctx_put(ctx);
    return 0;
}

}  // namespace mgta_cli
