// cli_reads.cpp — coverage, sharecov (graph_counted), matchreads, samplecov and pileup (graph_any + the read library): the contigs of a
// FASTA set against the graph and the reads it was built from; recruit: the read library against a gene's model, without a graph.
// File formats: INTEGRATION.md; megagta_amd/*.py print the same bytes.
#include <algorithm>
#include <cstring>
#include "cli.hpp"

namespace mgta_cli {
// ---- coverage: per-contig k-mer coverage and abundance from the graph's own multiplicities (the reference's last post-processing step,
// `kmer_coverage` in bin/post_proc.sh:113-118, recounts them from the reads).  The file formats are this project's own: INTEGRATION.md.
int main_coverage(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "Usage: megagta coverage <sdbg_prefix> <contigs.fasta> <out_prefix>\n"); return 1; }
    RssLine rss;
    const std::string prefix = argv[1], fasta = argv[2], out_prefix = argv[3];
    const FastaRecords in = read_fasta(fasta);
    const int64_t n = in.n();
    double t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    mgta_sdbg *g = graph_counted(ctx, prefix, t0);
    std::vector<mgta_contig_cov> cov((size_t)n);
    std::vector<int64_t> abund(65536);
    mgta_coverage_stats st;
    t0 = now_s();
    // all records in ONE call: the abundance counts an edge once for the file
    if (mgta_contig_coverage(g, in.seqs.data(), in.offsets.data(), n, cov.data(), nullptr, abund.data(), &st) != MGTA_OK) die("mgta_contig_coverage: %s", mgta_last_error());
    logf("coverage of %lld contigs: %lld windows, %lld by the walk, %lld index searches, %lld batch%s; kernels %.1f ms (walk %.1f ms), wall %.3f s", (long long)n,
         (long long)st.n_windows, (long long)st.n_walked, (long long)st.n_index_searches, (long long)st.n_batches, st.n_batches == 1 ? "" : "es", st.ms_kernel,
         st.ms_walk, now_s() - t0);
    std::string table = "#contig\tlen\twindows\tcovered\tmean\tmedian\tmin\tmax\n", abundance;
    for (int64_t i = 0; i < n; ++i) {
        const mgta_contig_cov &c = cov[(size_t)i];
        appendf(table, "%s\t%u\t%u\t%u\t%.4f\t%u\t%u\t%u\n", in.names[(size_t)i].c_str(), c.len, c.n_windows, c.n_covered,
                c.n_windows ? (double)c.sum / (double)c.n_windows : 0.0, c.median, c.min, c.max);
    }
    for (int m = 0; m < 65536; ++m)
        if (abund[(size_t)m]) appendf(abundance, "%d\t%lld\n", m, (long long)abund[(size_t)m]);
    write_or_die(out_prefix + "_coverage.txt", table);
    write_or_die(out_prefix + "_abundance.txt", abundance);
    graph_done(g);
    ctx_put(ctx);
    return 0;
}

// ---- sharecov: the window-shared coverage of every record of a FASTA (mgta_contig_share_coverage): masses that add up over any set of
// contigs, what `megagta.py --taxon-abund` sums per cluster and per reference.  The file format is this project's own: INTEGRATION.md 2n.
// mass (Q16) is printed with four decimals by integers only, so that megagta_amd/taxonabund.py prints the same bytes at any size.
static void append_q16(std::string &out, uint64_t mass) {
    const unsigned __int128 q = ((unsigned __int128)mass * 10000u) >> 16;
    appendf(out, "%llu.%04llu", (unsigned long long)(q / 10000u), (unsigned long long)(q % 10000u));
}

int main_sharecov(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "Usage: megagta sharecov <sdbg_prefix> <contigs.fasta> <out_prefix>\n"); return 1; }
    RssLine rss;
    const std::string prefix = argv[1], fasta = argv[2], out_prefix = argv[3];
    const FastaRecords in = read_fasta(fasta);
    const int64_t n = in.n();
    double t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    mgta_sdbg *g = graph_counted(ctx, prefix, t0);
    std::vector<mgta_contig_share> rec((size_t)n);
    mgta_share_stats st;
    t0 = now_s();
    // all records in ONE call: the shares are counted over the file
    if (mgta_contig_share_coverage(g, in.seqs.data(), in.offsets.data(), n, rec.data(), nullptr, nullptr, &st) != MGTA_OK)
        die("mgta_contig_share_coverage: %s", mgta_last_error());
    logf("shared coverage of %lld contigs: %lld windows, %lld covered, %lld distinct edges, %lld batch%s; walk %.1f ms, count %.1f ms, share %.1f ms, table %.1f MB, wall %.3f s",
         (long long)n, (long long)st.n_windows, (long long)st.n_covered, (long long)st.n_distinct_edges, (long long)st.n_batches, st.n_batches == 1 ? "" : "es", st.ms_walk,
         st.ms_count, st.ms_share, (double)st.table_bytes / 1e6, now_s() - t0);
    std::string table = "#contig\tlen\twindows\tcovered\tunique\tmax_share\tmass\n";
    for (int64_t i = 0; i < n; ++i) {
        const mgta_contig_share &c = rec[(size_t)i];
        appendf(table, "%s\t%u\t%u\t%u\t%u\t%u\t", in.names[(size_t)i].c_str(), c.len, c.n_windows, c.n_covered, c.n_unique, c.max_share);
        append_q16(table, c.mass);
        table += '\n';
    }
    write_or_die(out_prefix + "_sharecov.txt", table);
    graph_done(g);
    ctx_put(ctx);
    return 0;
}

// ---- matchreads: the reads of the library that share a (k+1)-mer with the contigs of a FASTA, on either strand (the `-m` output of the
// reference's `kmer_coverage` step, bin/post_proc.sh:113-118).  The file format is this project's own: INTEGRATION.md 2h.
int main_matchreads(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "Usage: megagta matchreads <sdbg_prefix> <read.lib> <contigs.fasta> <out_prefix>\n"); return 1; }
    RssLine rss;
    const std::string prefix = argv[1], lib = argv[2], fasta = argv[3], out_prefix = argv[4];
    const FastaRecords in = read_fasta(fasta);
    const int64_t n = in.n();
    double t0 = now_s();
    PackedReads local;
    uint64_t n_reads = 0;
    const PackedReads &pr = reads_open(lib, local, &n_reads);
    logf("%llu reads, %llu total bases (load %.3f s)", (unsigned long long)n_reads, (unsigned long long)pr.start.back(), now_s() - t0);
    t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    mgta_sdbg *g = graph_any(ctx, prefix, t0);
    t0 = now_s();
    mgta_reads *rd = reads_upload(ctx, pr);
    std::vector<uint64_t> bits((size_t)((n_reads + 63) / 64) + 1);
    mgta_match_stats st;
    // all records in ONE call (the marks live for one call); bits only: the walk of a read ends at its first hit
    if (mgta_reads_match_contigs(g, rd, 1, n_reads, in.seqs.data(), in.offsets.data(), n, bits.data(), nullptr, &st) != MGTA_OK) die("mgta_reads_match_contigs: %s", mgta_last_error());
    mgta_reads_free(rd);
    logf("matched reads of %lld contigs: %lld contig windows marked %lld edges (%.1f ms); %lld of %lld reads match, %lld read windows, %lld by the walk, %lld index "
         "searches, %lld groups per CU (%.1f ms); wall %.3f s", (long long)n, (long long)st.n_contig_windows, (long long)st.n_marked_edges, st.ms_mark,
         (long long)st.n_matched_reads, (long long)st.n_reads, (long long)st.n_read_windows, (long long)st.n_walked, (long long)st.n_index_searches,
         (long long)st.groups_per_cu, st.ms_walk, now_s() - t0);
    const std::string path = out_prefix + "_match_reads.fa";
    FILE *f = fopen(path.c_str(), "w");
    if (!f) die("cannot write %s", path.c_str());
    std::string rec;
    for (uint64_t r = 0; r < n_reads; ++r) {
        if (!((bits[(size_t)(r >> 6)] >> (r & 63)) & 1)) continue;
        const uint64_t s0 = pr.start[(size_t)r], len = pr.start[(size_t)r + 1] - s0;
        rec = ">r" + std::to_string((unsigned long long)r) + "\n";
        for (uint64_t j = 0; j < len; ++j) {                            // reversed storage -> the read as sequenced
            const uint64_t q = s0 + (len - 1 - j);
            rec.push_back("ACGT"[(pr.words[(size_t)(q >> 4)] >> (30 - 2 * (q & 15))) & 3]);
        }
        rec.push_back('\n');
        if (fwrite(rec.data(), 1, rec.size(), f) != rec.size()) die("short write to %s", path.c_str());
    }
    if (fclose(f) != 0) die("short write to %s", path.c_str());
    graph_done(g);
    ctx_put(ctx);
    return 0;
}

// ---- recruit: the reads of the library that a gene's profile HMM places in one of six frames (mgta_reads_recruit).  No graph is loaded
// and a worker's resident graphs and library stay as they are.  The rule and the file formats are this project's own: INTEGRATION.md
// 2h'; megagta_amd/recruit.py prints the same bytes.
int main_recruit(int argc, char **argv) {
    const char *usage = "Usage: megagta recruit <model.hmm> <read.lib> <out_prefix> [--min-bits B] [--min-aa N] [--local]\n";
    if (argc < 4) { fputs(usage, stderr); return 1; }
    double min_bits = 20.0;
    long long min_aa = 20;
    bool local_mode = false;
    for (int i = 4; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--local") { local_mode = true; continue; }
        if ((a != "--min-bits" && a != "--min-aa") || i + 1 >= argc) { fputs(usage, stderr); return 1; }
        const char *text = argv[++i];
        if (a == "--min-aa") {
            if (!parse_ll(text, &min_aa) || min_aa < 1 || min_aa > 4096) { fprintf(stderr, "megagta recruit: --min-aa %s is not a count of 1 .. 4096 residues\n%s", text, usage); return 1; }
        } else {
            char *end = nullptr;
            min_bits = strtod(text, &end);
            if (end == text || *end || min_bits != min_bits) { fprintf(stderr, "megagta recruit: --min-bits %s is not a number\n%s", text, usage); return 1; }
        }
    }
    RssLine rss;
    const std::string model = argv[1], lib = argv[2], out_prefix = argv[3];
    const std::vector<LibRow> libs = read_lib_table(lib);
    double t0 = now_s();
    PackedReads local;
    uint64_t n_reads = 0;
    const PackedReads &pr = reads_open(lib, local, &n_reads);
    if (!libs.empty() && (uint64_t)(libs.back().to + 1) != n_reads)
        die("recruit: %s.lib_info names %lld reads, %s.bin holds %llu", lib.c_str(), libs.back().to + 1, lib.c_str(), (unsigned long long)n_reads);
    logf("%llu reads, %llu total bases (load %.3f s)", (unsigned long long)n_reads, (unsigned long long)pr.start.back(), now_s() - t0);
    t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    int M = 0;
    mgta_hmm *hmm = upload_hmm(ctx, model, &M);
    mgta_reads *rd = reads_upload(ctx, pr);
    std::vector<uint64_t> bits((size_t)((n_reads + 63) / 64) + 1), depth((size_t)M + 1);
    std::vector<mgta_recruit_rec> recs((size_t)n_reads + 1);
    const mgta_recruit_params par{(int32_t)min_aa, local_mode ? MGTA_RECRUIT_LOCAL : MGTA_RECRUIT_GLOBAL, min_bits * 0.6931471805599453};
    mgta_recruit_stats st;
    if (mgta_reads_recruit(ctx, hmm, rd, 1, n_reads, &par, bits.data(), recs.data(), depth.data(), &st) != MGTA_OK) die("mgta_reads_recruit: %s", mgta_last_error());
    mgta_reads_free(rd);
    mgta_hmm_free(hmm);
    logf("recruited reads of %s (%d columns, %s, >= %g bits, stretches >= %lld residues): %lld of %lld reads, %lld frames scored, %lld cells, %lld reads unaligned, %lld "
         "unscored; %lld rows per wave, %lld reads per grab, %lld waves per workgroup, %lld per CU, LDS %lld (scan %.1f ms, fill %.1f ms); wall %.3f s", model.c_str(), M,
         local_mode ? "local" : "global", min_bits, min_aa, (long long)st.n_recruited, (long long)st.n_reads, (long long)st.n_frames_scored, (long long)st.n_cells, (long long)st.n_unaligned,
         (long long)st.n_unscored, (long long)st.rows_per_wave, (long long)st.chunk, (long long)st.waves_per_block, (long long)st.blocks_per_cu, (long long)st.lds_bytes,
         st.ms_scan, st.ms_fill, now_s() - t0);
    std::string fa, table = "#read\tframe\taa_from\taa_len\tbits\tmodel_from\tmodel_to\n", cols = "#column\tdepth\n", summary;
    std::vector<long long> per_lib(libs.size(), 0);
    size_t s = 0;
    for (uint64_t r = 0; r < n_reads; ++r) {
        if (!((bits[(size_t)(r >> 6)] >> (r & 63)) & 1)) continue;
        const uint64_t s0 = pr.start[(size_t)r], len = pr.start[(size_t)r + 1] - s0;
        fa += ">r" + std::to_string((unsigned long long)r) + "\n";
        for (uint64_t j = 0; j < len; ++j) {                            // reversed storage -> the read as sequenced
            const uint64_t q = s0 + (len - 1 - j);
            fa.push_back("ACGT"[(pr.words[(size_t)(q >> 4)] >> (30 - 2 * (q & 15))) & 3]);
        }
        fa.push_back('\n');
        const mgta_recruit_rec &c = recs[(size_t)r];
        appendf(table, "%llu\t%u\t%u\t%u\t%.4f\t%d\t%d\n", (unsigned long long)r, (unsigned)c.frame, (unsigned)c.aa_from, (unsigned)c.aa_len, c.score / 0.6931471805599453,
                c.model_from, c.model_to);
        while (s < libs.size() && (long long)r > libs[s].to) ++s;
        if (s < libs.size()) ++per_lib[s];
    }
    for (int j = 0; j < M; ++j) appendf(cols, "%d\t%llu\n", j + 1, (unsigned long long)depth[(size_t)j]);
    appendf(summary, "reads_scanned\t%lld\nreads_scored\t%lld\nreads_recruited\t%lld\n", (long long)st.n_reads, (long long)(st.n_reads - st.n_unscored), (long long)st.n_recruited);
    for (int f = 0; f < 6; ++f) appendf(summary, "recruited_frame%d\t%lld\n", f, (long long)st.n_recruited_frame[f]);
    for (size_t l = 0; l < libs.size(); ++l) appendf(summary, "recruited_lib%zu\t%lld\n", l, per_lib[l]);
    if (local_mode) summary += "recruit_mode\tlocal\n";
    write_or_die(out_prefix + "_reads.fa", fa);
    write_or_die(out_prefix + ".txt", table);
    write_or_die(out_prefix + "_cols.txt", cols);
    write_or_die(out_prefix + "_summary.txt", summary);
    ctx_put(ctx);
    return 0;
}

// ---- samplecov: the read windows of every library of the read set on the windows of every record of a FASTA
// (mgta_contig_sample_coverage), what `megagta.py --sample-abund` sums per cluster.  A paired library is one sample: both mates count.
// The file format is this project's own: INTEGRATION.md 2o; megagta_amd/samplecov.py prints the same bytes.
int main_samplecov(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "Usage: megagta samplecov <sdbg_prefix> <read.lib> <contigs.fasta> <out_prefix>\n"); return 1; }
    RssLine rss;
    const std::string prefix = argv[1], lib = argv[2], fasta = argv[3], out_prefix = argv[4];
    const FastaRecords in = read_fasta(fasta);
    const int64_t n = in.n();
    const std::vector<LibRow> libs = read_lib_table(lib);
    if (libs.empty() || libs.size() > 256) die("samplecov: %s.lib_info names %zu libraries (1 .. 256 are supported)", lib.c_str(), libs.size());
    const size_t n_libs = libs.size();
    double t0 = now_s();
    PackedReads local;
    uint64_t n_reads = 0;
    const PackedReads &pr = reads_open(lib, local, &n_reads);
    logf("%llu reads, %llu total bases in %zu librar%s (load %.3f s)", (unsigned long long)n_reads, (unsigned long long)pr.start.back(), n_libs, n_libs == 1 ? "y" : "ies",
         now_s() - t0);
    std::vector<uint64_t> lib_end(n_libs), read_windows(n_libs, 0), hits(n_libs, 0);
    for (size_t s = 0; s < n_libs; ++s) lib_end[s] = (uint64_t)(libs[s].to + 1);
    if (lib_end.back() != n_reads) die("samplecov: %s.lib_info names %llu reads, %s.bin holds %llu", lib.c_str(), (unsigned long long)lib_end.back(), lib.c_str(), (unsigned long long)n_reads);
    t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    mgta_sdbg *g = graph_any(ctx, prefix, t0);
    const uint64_t k = (uint64_t)mgta_sdbg_k(g);
    for (size_t s = 0; s < n_libs; ++s)
        for (uint64_t r = s ? lib_end[s - 1] : 0; r < lib_end[s]; ++r) {
            const uint64_t len = pr.start[(size_t)r + 1] - pr.start[(size_t)r];
            read_windows[s] += len > k ? len - k : 0;
        }
    t0 = now_s();
    mgta_reads *rd = reads_upload(ctx, pr);
    std::vector<uint64_t> mass((size_t)n * n_libs + 1);
    std::vector<mgta_contig_share> rec((size_t)n + 1);
    mgta_sample_cov_stats st;
    // all records in ONE call: the shares are counted over the file
    if (mgta_contig_sample_coverage(g, rd, 1, lib_end.data(), (int)n_libs, in.seqs.data(), in.offsets.data(), n, mass.data(), rec.data(), nullptr, nullptr, hits.data(), &st) != MGTA_OK)
        die("mgta_contig_sample_coverage: %s", mgta_last_error());
    mgta_reads_free(rd);
    logf("per-library coverage of %lld contigs: %lld windows, %lld covered, %lld keys (%.1f ms); %lld reads, %lld read windows, %lld on a key, %lld by the walk, %lld index "
         "searches, %lld groups per CU (%.1f ms); masses %.1f ms; table %.1f MB, counts %.1f MB; wall %.3f s", (long long)n, (long long)st.n_windows, (long long)st.n_covered,
         (long long)st.n_keys, st.ms_mark, (long long)st.n_reads, (long long)st.n_read_windows, (long long)st.n_hit_windows, (long long)st.n_read_walked,
         (long long)st.n_read_index_searches, (long long)st.groups_per_cu, st.ms_scan, st.ms_mass, (double)st.table_bytes / 1e6, (double)st.count_bytes / 1e6, now_s() - t0);
    std::string table;
    for (size_t s = 0; s < n_libs; ++s)
        appendf(table, "#lib\t%zu\t%lld\t%llu\t%llu\t%s\n", s + 1, libs[s].to - libs[s].from + 1, (unsigned long long)read_windows[s], (unsigned long long)hits[s],
                libs[s].text.c_str());
    table += "#contig\tlen\twindows\tcovered\tunique\tmax_share";
    for (size_t s = 0; s < n_libs; ++s) appendf(table, "\tmass_%zu", s + 1);
    table += '\n';
    for (int64_t i = 0; i < n; ++i) {
        const mgta_contig_share &c = rec[(size_t)i];
        appendf(table, "%s\t%u\t%u\t%u\t%u\t%u", in.names[(size_t)i].c_str(), c.len, c.n_windows, c.n_covered, c.n_unique, c.max_share);
        for (size_t s = 0; s < n_libs; ++s) {
            table += '\t';
            append_q16(table, mass[(size_t)i * n_libs + s]);
        }
        table += '\n';
    }
    write_or_die(out_prefix + "_samplecov.txt", table);
    graph_done(g);
    ctx_put(ctx);
    return 0;
}
// ---- pileup: the reads of the library placed on the records of a FASTA (mgta_reads_pileup): per-base depth, placements and the positions
// where the reads disagree with a contig.  The rule and the file formats are this project's own: INTEGRATION.md 2p; megagta_amd/pileup.py
// prints the same bytes.  With --phase the same call also returns the placement of every read, the positions listed as variants are
// the sites and mgta_reads_phase counts which of their alleles one fragment shows together (the library table of .lib_info says which
// reads are mates): INTEGRATION.md 2q; megagta_amd/phase.py prints the same bytes.
int main_pileup(int argc, char **argv) {
    const char *usage = "Usage: megagta pileup <sdbg_prefix> <read.lib> <contigs.fasta> <out_prefix> [--min-anchors N] [--min-overlap N] [--max-mismatch-permille N] "
                        "[--min-depth N] [--min-alt-permille N] [--per-base] [--phase [--max-span N] [--min-link N] [--min-hap-permille N]]\n"
                        "                      [--gapped [--max-gap N] [--gap-open N] [--gap-extend N]]\n";
    if (argc < 5) { fputs(usage, stderr); return 1; }
    mgta_pileup_params par{0, 0, 0};
    long long min_depth = 8, min_alt = 100, max_span = 0, min_link = 4, min_hap = 100, max_gap = 0, gap_open = 0, gap_extend = 0;
    bool per_base = false, phase = false, phase_opt = false, gapped = false, gap_opt = false;
    for (int i = 5; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--per-base") { per_base = true; continue; }
        if (a == "--phase") { phase = true; continue; }
        if (a == "--gapped") { gapped = true; continue; }
        long long *into64 = a == "--min-depth" ? &min_depth : a == "--min-alt-permille" ? &min_alt : a == "--max-span" ? &max_span : a == "--min-link" ? &min_link :
                            a == "--min-hap-permille" ? &min_hap : a == "--max-gap" ? &max_gap : a == "--gap-open" ? &gap_open : a == "--gap-extend" ? &gap_extend : nullptr;
        if (into64 == &max_span || into64 == &min_link || into64 == &min_hap) phase_opt = true;
        if (into64 == &max_gap || into64 == &gap_open || into64 == &gap_extend) gap_opt = true;
        int32_t *into = a == "--min-anchors" ? &par.min_anchors : a == "--min-overlap" ? &par.min_overlap : a == "--max-mismatch-permille" ? &par.max_mismatch_permille : nullptr;
        if ((!into && !into64) || i + 1 >= argc) { fputs(usage, stderr); return 1; }
        long long v = 0;
        if (!parse_ll(argv[++i], &v) || v < 0 || v > 0x7FFFFFFFll) { fprintf(stderr, "megagta pileup: %s %s is not a count\n%s", a.c_str(), argv[i], usage); return 1; }
        if (into) *into = (int32_t)v; else *into64 = v;
    }
    if (phase_opt && !phase) { fprintf(stderr, "megagta pileup: --max-span, --min-link and --min-hap-permille are options of --phase\n%s", usage); return 1; }
    if (gap_opt && !gapped) { fprintf(stderr, "megagta pileup: --max-gap, --gap-open and --gap-extend are options of --gapped\n%s", usage); return 1; }
    RssLine rss;
    const std::string prefix = argv[1], lib = argv[2], fasta = argv[3], out_prefix = argv[4];
    const FastaRecords in = read_fasta(fasta);
    const int64_t n = in.n();
    std::vector<LibRow> libs;
    if (phase) {
        libs = read_lib_table(lib);
        if (libs.empty() || libs.size() > 256) die("pileup --phase: %s.lib_info names %zu libraries (1 .. 256 are supported)", lib.c_str(), libs.size());
    }
    double t0 = now_s();
    PackedReads local;
    uint64_t n_reads = 0;
    const PackedReads &pr = reads_open(lib, local, &n_reads);
    if (phase && (uint64_t)(libs.back().to + 1) != n_reads)
        die("pileup --phase: %s.lib_info names %lld reads, %s.bin holds %llu", lib.c_str(), libs.back().to + 1, lib.c_str(), (unsigned long long)n_reads);
    logf("%llu reads, %llu total bases (load %.3f s)", (unsigned long long)n_reads, (unsigned long long)pr.start.back(), now_s() - t0);
    t0 = now_s();
    mgta_ctx *ctx = ctx_get();
    mgta_sdbg *g = graph_any(ctx, prefix, t0);
    t0 = now_s();
    mgta_reads *rd = reads_upload(ctx, pr);
    const size_t n_sym = (size_t)in.offsets.back();
    std::vector<uint32_t> counts(n_sym * 4 + 4), uniq(n_sym + 1);
    std::vector<mgta_contig_pileup> rec((size_t)n + 1);
    std::vector<mgta_read_place> place(phase ? (size_t)n_reads + 1 : 0);
    mgta_pileup_stats st;
    std::string indels;
    // all records in ONE call: the best-hit rule looks at every contig of the file
    if (gapped) {
        // INTEGRATION.md 2p': the same files from the gapped counts and PREFIX_pileup_indels.txt; megagta_amd/gapped.py prints the same bytes
        const mgta_gapped_params gpar{par.min_anchors, par.min_overlap, par.max_mismatch_permille, (int32_t)max_gap, (int32_t)gap_open, (int32_t)gap_extend};
        std::vector<mgta_gap_place> gplace(phase ? (size_t)n_reads + 1 : 0);
        std::vector<mgta_gap_rec> gaps(std::max<size_t>(16, (size_t)n_reads / 8));
        mgta_gapped_stats gs;
        memset(&gs, 0, sizeof(gs));
        int rcode = mgta_reads_pileup_gapped(g, rd, 1, n_reads, in.seqs.data(), in.offsets.data(), n, &gpar, counts.data(), uniq.data(), rec.data(), phase ? gplace.data() : nullptr,
                                             gaps.data(), gaps.size(), &gs);
        if (rcode == MGTA_EINVAL && (uint64_t)gs.n_gap_placements > gaps.size()) {   // the buffer was sized from the reads: once more with the count the library names
            gaps.resize((size_t)gs.n_gap_placements);
            rcode = mgta_reads_pileup_gapped(g, rd, 1, n_reads, in.seqs.data(), in.offsets.data(), n, &gpar, counts.data(), uniq.data(), rec.data(), phase ? gplace.data() : nullptr,
                                             gaps.data(), gaps.size(), &gs);
        }
        if (rcode != MGTA_OK) die("mgta_reads_pileup_gapped: %s", mgta_last_error());
        gaps.resize((size_t)gs.n_gap_placements);
        memcpy(&st, &gs, sizeof(st));                                         // (the first fields of mgta_gapped_stats are mgta_pileup_stats)
        logf("gapped: %lld one-gap candidates, %lld pass; %lld reads placed across a gap, %lld gapped placements, %lld letters inserted, %lld deleted",
             (long long)gs.n_gap_candidates, (long long)gs.n_gap_passing, (long long)gs.n_reads_gapped, (long long)gs.n_gap_placements, (long long)gs.n_inserted,
             (long long)gs.n_deleted);
        for (size_t r = 0; phase && r < (size_t)n_reads; ++r) {               // a gapped placement gives --phase no allele
            const mgta_gap_place &p = gplace[r];
            place[r] = mgta_read_place{p.score, p.contig, p.diag, p.orient, p.diag2 != p.diag ? 0u : p.n_placed, p.n_mismatch};
        }
        std::vector<GapEvent> evs;
        for (const mgta_gap_rec &x : gaps) {
            GapEvent e;
            e.contig = x.contig; e.pos = x.pos; e.is_del = x.len > 0; e.len = (uint32_t)(x.len > 0 ? x.len : -x.len); e.unique = x.unique != 0;
            if (e.is_del) e.letters = in.seqs.substr((size_t)in.offsets[(size_t)x.contig] + x.pos, e.len);
            else {
                const uint64_t s0 = pr.start[(size_t)x.read], len = pr.start[(size_t)x.read + 1] - s0;
                for (uint32_t j = 0; j < e.len; ++j) {                        // the stored order is the read reversed
                    const uint64_t p = x.brk + j, q = s0 + (x.orient ? p : len - 1 - p);
                    const uint32_t c = (pr.words[(size_t)(q >> 4)] >> (30 - 2 * (q & 15))) & 3u;
                    e.letters.push_back("ACGT"[x.orient ? 3 - c : c]);
                }
            }
            evs.push_back(std::move(e));
        }
        indels = format_indels(in.names, in.offsets, counts.data(), evs, (uint32_t)min_depth, (uint32_t)min_alt);
    } else if (mgta_reads_pileup(g, rd, 1, n_reads, in.seqs.data(), in.offsets.data(), n, &par, counts.data(), uniq.data(), rec.data(), phase ? place.data() : nullptr, &st) != MGTA_OK)
        die("mgta_reads_pileup: %s", mgta_last_error());
    logf("pileup of %lld contigs: %lld windows, %lld keys, %lld occurrences (%.1f + %.1f ms); %lld reads, %lld read windows, %lld on a key; %lld reads with a candidate, "
         "%lld candidates, %lld verified; %lld reads placed, %lld more than once, %lld placements, %lld bases (%.1f ms); records %.1f ms; %.1f MB on the device; wall %.3f s",
         (long long)n, (long long)st.n_contig_windows, (long long)st.n_keys, (long long)st.n_occurrences, st.ms_keys, st.ms_index, (long long)st.n_reads,
         (long long)st.n_read_windows, (long long)st.n_hit_windows, (long long)st.n_reads_with_candidate, (long long)st.n_candidates, (long long)st.n_verified,
         (long long)st.n_reads_placed, (long long)st.n_reads_multi, (long long)st.n_placements, (long long)st.n_bases_piled, st.ms_scan, st.ms_records,
         (double)st.peak_bytes / 1e6, now_s() - t0);
    PhaseTexts ptxt;
    if (phase) {
        const double t1 = now_s();
        std::vector<uint64_t> site_off, lib_end(libs.size());
        std::vector<uint32_t> site_pos;
        std::vector<uint8_t> lib_paired(libs.size());
        for (size_t s = 0; s < libs.size(); ++s) { lib_end[s] = (uint64_t)(libs[s].to + 1); lib_paired[s] = libs[s].pe ? 1 : 0; }
        pileup_variant_sites(in.seqs, in.offsets, counts.data(), (uint32_t)min_depth, (uint32_t)min_alt, site_off, site_pos);
        std::vector<uint64_t> pair_off(site_pos.size() + 1);
        if (mgta_phase_pairs(site_off.data(), site_pos.data(), n, (int32_t)max_span, pair_off.data()) != MGTA_OK) die("mgta_phase_pairs: %s", mgta_last_error());
        std::vector<uint32_t> site_counts(site_pos.size() * 4 + 4), joint((size_t)pair_off.back() * 16 + 16);
        const mgta_phase_params pp{(int32_t)max_span};
        mgta_phase_stats ps;
        if (mgta_reads_phase(rd, 1, place.data(), lib_end.data(), lib_paired.data(), (int)libs.size(), in.offsets.data(), n, site_off.data(), site_pos.data(), &pp,
                             site_counts.data(), pair_off.data(), joint.data(), pair_off.back(), &ps) != MGTA_OK)
            die("mgta_reads_phase: %s", mgta_last_error());
        logf("phase of %lld sites, %lld pairs: %lld reads, %lld usable, %lld fragments, %lld of two mates; %lld with an allele, %lld with two or more; %lld alleles, %lld "
             "conflicts, %lld pair adds (upload %.1f ms, scan %.1f ms); %.1f MB on the device; wall %.3f s", (long long)ps.n_sites, (long long)ps.n_pairs, (long long)ps.n_reads,
             (long long)ps.n_usable, (long long)ps.n_fragments, (long long)ps.n_mate_fragments, (long long)ps.n_fragments_allele, (long long)ps.n_fragments_linked,
             (long long)ps.n_alleles, (long long)ps.n_conflicts, (long long)ps.n_pair_adds, ps.ms_upload, ps.ms_scan, (double)ps.peak_bytes / 1e6, now_s() - t1);
        ptxt = format_phase(in.names, site_off, site_pos, pair_off, joint.data(), (uint64_t)min_link, (uint64_t)min_hap);
    }
    mgta_reads_free(rd);
    static_assert(sizeof(PileupRow) == sizeof(mgta_contig_pileup), "PileupRow is mgta_contig_pileup");
    const PileupTexts txt = format_pileup(in.names, in.seqs, in.offsets, counts.data(), uniq.data(), reinterpret_cast<const PileupRow *>(rec.data()), (uint32_t)min_depth,
                                          (uint32_t)min_alt, per_base);
    write_or_die(out_prefix + "_pileup.txt", txt.summary);
    write_or_die(out_prefix + "_pileup_variants.txt", txt.variants);
    if (per_base) write_or_die(out_prefix + "_pileup_depth.txt", txt.depth);
    if (gapped) write_or_die(out_prefix + "_pileup_indels.txt", indels);
    if (phase) write_or_die(out_prefix + "_phase_links.txt", ptxt.links);
    if (phase) write_or_die(out_prefix + "_phase_blocks.txt", ptxt.blocks);
    graph_done(g);
    ctx_put(ctx);
    return 0;
}

}  // namespace mgta_cli
