// cli.hpp — what the units of the `megagta` binary share (host only, above the C ABI): session.cpp holds main(), the dispatch table and
// the `megagta serve` session; cli_graph.cpp, cli_reads.cpp, cli_protein.cpp and cli_dev.cpp hold the sub-commands by stage family.  A
// sub-command is `int main_NAME(argc, argv)` with argv[0] = its name, for a one-shot process and the worker alike; it reaches the session
// only through the functions declared here.
#pragma once
#include <sys/resource.h>
#include <sys/time.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <utility>
#include <vector>
#include "../../../include/megagta_hip.h"
#include "formats.hpp"

namespace mgta_cli {
using namespace mgta_host;

inline double now_s() {
    struct timeval tv;
    gettimeofday(&tv, nullptr);
    return tv.tv_sec + 1e-6 * tv.tv_usec;
}
inline int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}
struct RssLine {   // AutoMaxRssRecorder, utils.h:99-128
    double t0 = now_s();
    ~RssLine() {
        struct rusage u;
        getrusage(RUSAGE_SELF, &u);
        logf("Real: %.4lf\tuser: %.4lf\tsys: %.4lf\tmaxrss: %ld", now_s() - t0, u.ru_utime.tv_sec + 1e-6 * u.ru_utime.tv_usec,
             u.ru_stime.tv_sec + 1e-6 * u.ru_stime.tv_usec, u.ru_maxrss);
    }
};

// ---- the session (session.cpp) -----------------------------------------------------------------------------------------------------
bool in_worker();                                    // this process is `megagta serve`: contexts, library and graphs outlive the step
mgta_ctx *ctx_get(int lane = 0);                     // lane 1: the second context of the device, the other lane of a two-gene search
void ctx_put(mgta_ctx *ctx);
int writer_join();                                   // the graph files of the last buildgraph are complete; 1 when their writer failed
int contigs_join(bool free_text);                    // the same for the contigs file of the last denovo
PackedReads &lib_get(const std::string &bin_path, const std::string &lib_prefix, const std::string &extra, bool extra_is_assist, PackedReads &local,
                     PackedReads::Mark &mk);
// the library alone, as matchreads, samplecov, pileup and recruit take it, and a library's copy on the device (freed with mgta_reads_free)
PackedReads &reads_open(const std::string &lib, PackedReads &local, uint64_t *n_reads);
mgta_reads *reads_upload(mgta_ctx *ctx, const PackedReads &pr);
// the three ways to a graph (the rule is written once, above them in session.cpp), and the end of a step's use of one
mgta_sdbg *graph_take(mgta_ctx *ctx, const std::string &prefix, int *k_out, size_t *n_edges);
mgta_sdbg *graph_counted(mgta_ctx *ctx, const std::string &prefix, double t0);
mgta_sdbg *graph_any(mgta_ctx *ctx, const std::string &prefix, double t0);
void graph_done(mgta_sdbg *g);
void graph_drop();
// what buildgraph and denovo leave with a worker: the built graph (and, detached, its edge stream) with the writer of its files; the
// contigs text with the writer of its file
mgta_stream *graph_hand_over(mgta_ctx *ctx, const std::string &prefix, bool detach_stream);
void graph_writer_start(std::function<void()> write_files);
void contigs_keep(char *text, uint64_t len, const std::string &path, std::function<void(const char *, uint64_t)> write);

// ---- shared pieces -------------------------------------------------------------------------------------------------------------------
// the records of a FASTA in file order: name = the header up to the first blank, sequence = its lines joined (offsets [n + 1] into seqs)
// (headers, when asked for: every header line behind its '>' as it stands in the file, without the line end)
struct FastaRecords {
    std::vector<std::string> names, headers;
    std::string seqs;
    std::vector<uint64_t> offsets;
    int64_t n() const { return (int64_t)names.size(); }
    void append_record(std::string &out, size_t i) const {               // ">header\nsequence\n"
        out += ">" + headers[i] + "\n";
        out.append(seqs, (size_t)offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
        out += "\n";
    }
};
inline FastaRecords read_fasta(const std::string &path, bool want_headers = false) {
    FastaRecords r;
    r.offsets.assign(1, 0);
    FILE *f = fopen(path.c_str(), "r");
    if (!f) die("cannot open %s", path.c_str());
    char *line = nullptr;
    size_t cap = 0;
    ssize_t n;
    bool open_rec = false;
    while ((n = getline(&line, &cap, f)) >= 0) {
        while (n > 0 && (line[n - 1] == '\n' || line[n - 1] == '\r')) line[--n] = 0;
        if (want_headers && n > 0 && line[0] == '>') r.headers.emplace_back(line + 1, (size_t)n - 1);
        while (n > 0 && (line[n - 1] == ' ' || line[n - 1] == '\t')) line[--n] = 0;
        if (n > 0 && line[0] == '>') {
            if (open_rec) r.offsets.push_back(r.seqs.size());
            size_t e = 1;
            while (e < (size_t)n && line[e] != ' ' && line[e] != '\t') ++e;
            r.names.emplace_back(line + 1, e - 1);
            open_rec = true;
        } else if (open_rec) {
            const char *b = line;
            while (*b == ' ' || *b == '\t') ++b;
            r.seqs.append(b);
        }
    }
    if (open_rec) r.offsets.push_back(r.seqs.size());
    free(line);
    fclose(f);
    return r;
}
// the nucleotide records of `nucl_path` for the protein records: one per record, in order and under the same name (`translate` writes
// them so), anything else is not this gene's pair; false after an [ERROR] line
inline bool read_paired(const char *who, const FastaRecords &prot, const std::string &prot_path, const std::string &nucl_path, FastaRecords &nucl) {
    nucl = read_fasta(nucl_path, true);
    if (nucl.names.size() != prot.names.size()) {
        fprintf(stderr, "    [ERROR] %s: %s holds %zu records, %s holds %zu: nothing written\n", who, prot_path.c_str(), prot.names.size(), nucl_path.c_str(),
                nucl.names.size());
        return false;
    }
    for (size_t i = 0; i < prot.names.size(); ++i)
        if (nucl.names[i] != prot.names[i]) {
            fprintf(stderr, "    [ERROR] %s: record %lld is %s in %s and %s in %s: nothing written\n", who, (long long)i, prot.names[i].c_str(), prot_path.c_str(),
                    nucl.names[i].c_str(), nucl_path.c_str());
            return false;
        }
    return true;
}
inline int residue_class(unsigned char b) { return (b < 128 && (b | 32) >= 'a' && (b | 32) <= 'z') ? (b | 32) - 'a' + 1 : 0; }
// the residues of the references: their ASCII letters, upper-cased; `-`, `.`, `*` and everything else go (the file may be an alignment)
inline std::pair<std::string, std::vector<uint64_t>> clean_references(const FastaRecords &raw) {
    std::string refs;
    std::vector<uint64_t> roffsets(1, 0);
    for (size_t r = 0; r < raw.names.size(); ++r) {
        for (uint64_t p = raw.offsets[r]; p < raw.offsets[r + 1]; ++p) {
            const unsigned char c = (unsigned char)raw.seqs[p];
            if (residue_class(c)) refs += (char)(c >= 'a' ? c - 32 : c);
        }
        roffsets.push_back(refs.size());
    }
    return {std::move(refs), std::move(roffsets)};
}
inline mgta_hmm *upload_hmm(mgta_ctx *ctx, const std::string &path, int *M = nullptr) {
    ProfileHmm hm;
    if (!parse_hmm(path, hm)) die("cannot open HMM %s", path.c_str());
    mgta_hmm *out = nullptr;
    if (mgta_hmm_load(ctx, hm.M, hm.A, hm.msc.data(), hm.tsc.data(), hm.max_match.data(), hm.h.data(), hm.alpha, &out) != MGTA_OK)
        die("mgta_hmm_load(%s): %s", path.c_str(), mgta_last_error());
    if (M) *M = hm.M;
    return out;
}
inline bool parse_ll(const char *text, long long *out) {                 // the whole of `text` is one integer
    char *end = nullptr;
    *out = strtoll(text, &end, 10);
    return end != text && !*end;
}
inline bool int_arg(const char *who, const char *name, const char *text, long long *out) {
    if (parse_ll(text, out)) return true;
    fprintf(stderr, "    [ERROR] %s: %s '%s' is not an integer\n", who, name, text);
    return false;
}
inline void appendf(std::string &out, const char *fmt, ...) {            // printf behind `out`, of any length
    va_list ap, again;
    va_start(ap, fmt);
    va_copy(again, ap);
    const size_t at = out.size(), n = (size_t)vsnprintf(nullptr, 0, fmt, ap);
    out.resize(at + n + 1);
    vsnprintf(&out[at], n + 1, fmt, again);
    out.resize(at + n);
    va_end(again);
    va_end(ap);
}
inline void write_or_die(const std::string &path, const std::string &text) {
    FILE *f = fopen(path.c_str(), "w");
    if (!f) die("cannot write %s", path.c_str());
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) die("cannot write %s", path.c_str());
}
// ordered-commit window and cost term of a gene's batch by its number of seeds (cli_graph.cpp; `megagta searchplan` prints it)
void search_plan(size_t ns, int *window, int *rate, long long *knee, int *rate2);

// ---- the sub-commands ------------------------------------------------------------------------------------------------------------------
typedef int SubCommand(int argc, char **argv);
SubCommand main_buildgraph, main_denovo, main_search, main_findstart, main_filterbylen, main_translate, main_buildlib;     // cli_graph.cpp
SubCommand main_coverage, main_sharecov, main_matchreads, main_samplecov, main_pileup, main_recruit;                            // cli_reads.cpp
SubCommand main_derep, main_align, main_posterior, main_cluster, main_clustertree, main_nearest, main_chimera;              // cli_protein.cpp
SubCommand main_libdump, main_sdbgcopy, main_sdbgmerge, main_hmmdump, main_searchplan, main_dumpversion;                    // cli_dev.cpp

}  // namespace mgta_cli
