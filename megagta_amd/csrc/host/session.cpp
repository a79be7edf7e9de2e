// session.cpp — main(), the table of sub-commands, and the worker session of `megagta serve`; the sub-commands (cli_*.cpp) reach what the
// session keeps between steps only through the functions of cli.hpp.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <atomic>
#include <cstring>
#include <thread>
#include "cli.hpp"

namespace mgta_cli {
// `megagta serve`: one process for all the steps of a driver run.  The sub-commands are the same functions; what a worker keeps
// between them is what a one-shot process pays for again at every step: the device context with its work memory (mapping device
// memory costs ~27 ms/GB), the read library (reads.lib.bin unpacked once), and the graph of the last `buildgraph`, which stays on
// the device for the `denovo` / `search` that follows instead of travelling through PREFIX.sdbg.* (succinct_dbg.cpp:595-723; the
// files are still written: they are the run's artefacts and what `--continue` resumes from).
struct Session {
    bool active = false;
    mgta_ctx *ctx = nullptr;
    std::string lib_key;          // path of the .bin the library was read from
    PackedReads lib;              // reversed; the contigs one step appended behind it stay for the next step that wants the same file
    bool lib_loaded = false;
    PackedReads::Mark lib_mark{}; // end of the library proper
    std::string extra_key;        // the contigs file behind it (path | size | mtime)
    bool have_extra = false;
    mgta_ctx *ctx2 = nullptr;     // second context of the device: the other lane of a two-gene search
    mgta_sdbg *graph = nullptr;   // graph of the last buildgraph, not used yet
    std::string graph_prefix;
    mgta_sdbg *cov_graph = nullptr;   // graph loaded WITH its multiplicities by the last `coverage`: serves the coverage of the next gene
    std::string cov_key;          // the graph files it came from (index path | size | mtime)
    mgta_sdbg *match_graph = nullptr; // graph loaded WITHOUT multiplicities by the last `matchreads` that found no counted graph to use
    std::string match_key;
    std::thread writer;           // PREFIX.sdbg.* of the last buildgraph being written while the next step already runs on the resident graph
    std::string writer_error;     // why that thread failed (set by the thread, read after the join)
    mgta_stream *stream = nullptr;   // the edge stream that thread downloads from the device (freed on this thread once it has joined)
    // the contigs of the last `denovo`: their FASTA text stays in memory for the `buildgraph` / `findstart` that take them as --assist_seq /
    // extra sequences (100 M reads: 4 GB of text, 8 s to read back and parse on one thread), and is written to PREFIX.contigs.fa by a thread
    // of its own behind the next step
    char *ctext = nullptr;
    uint64_t ctext_len = 0;
    std::string ctext_path;       // the file the text is (being) written to; stays set after the text is freed
    std::thread cwriter;
    std::atomic<bool> cwriter_done{true};
    std::string cwriter_error;
};
static Session g_sess;
// The graph files of the last buildgraph are complete: called before anything reads them, before the next build, at the end, and by the
// driver's "sync" request before it writes the checkpoint that says "graph built" (the reference writes its checkpoint after the files:
// megagta.py:538-586).  Returns 1 when the writer failed (disk full, ...): the failure belongs to the build, not to whatever step
// happened to be running when the thread hit it.
int writer_join() {
    if (g_sess.writer.joinable()) g_sess.writer.join();
    if (g_sess.stream) { mgta_stream_free(g_sess.stream); g_sess.stream = nullptr; }
    if (g_sess.writer_error.empty()) return 0;
    fprintf(stderr, "    [ERROR] writing the graph files of the last buildgraph failed: %s\n", g_sess.writer_error.c_str());
    fflush(stderr);
    g_sess.writer_error.clear();
    return 1;
}
// The contigs file of the last denovo is complete (and its text, if no step can want it any more, is freed): before the next denovo, at
// "sync" / "release" / the end.  Returns 1 when the writer failed.
int contigs_join(bool free_text) {
    if (g_sess.cwriter.joinable()) g_sess.cwriter.join();
    if (free_text && g_sess.ctext) { mgta_host_free(g_sess.ctext); g_sess.ctext = nullptr; g_sess.ctext_len = 0; }
    if (g_sess.cwriter_error.empty()) return 0;
    fprintf(stderr, "    [ERROR] writing the contigs of the last denovo failed: %s\n", g_sess.cwriter_error.c_str());
    fflush(stderr);
    g_sess.cwriter_error.clear();
    return 1;
}
bool in_worker() { return g_sess.active; }
// MEGAGTA_DEVICE: the GPU of this process (a rank of a multi-GPU step is started with its own; default 0); the second lane is on device 0
mgta_ctx *ctx_get(int lane) {
    mgta_ctx *&kept = lane ? g_sess.ctx2 : g_sess.ctx;
    if (g_sess.active && kept) return kept;
    mgta_ctx *ctx = mgta_ctx_create(lane ? 0 : env_int("MEGAGTA_DEVICE", 0));
    if (!ctx) die("%s", mgta_last_error());
    if (g_sess.active) kept = ctx;
    return ctx;
}
void ctx_put(mgta_ctx *ctx) { if (!g_sess.active) mgta_ctx_destroy(ctx); }
static std::string file_key(const std::string &path) {                  // "the same file": path | size | modification time
    struct stat sb;
    if (path.empty() || stat(path.c_str(), &sb) != 0) return path;
    return path + "|" + std::to_string((long long)sb.st_size) + "|" + std::to_string((long long)sb.st_mtime) + "|" + std::to_string((long long)sb.st_mtim.tv_nsec);
}
// The library of `bin_path` (reads.lib.bin), reversed, with the sequences of `extra` (a FASTA of contigs: the assist sequences of
// buildgraph, the contigs findstart scans with the reads) appended behind it, finished for upload.  `mk` = the end of the library
// proper.  The worker keeps both between steps: a multi-k run reads the contigs of a k once for the buildgraph and the findstart calls
// that use them (at 20 M reads: 0.8 GB of text, 1.5 s per parse), and never re-reads the library.
PackedReads &lib_get(const std::string &bin_path, const std::string &lib_prefix, const std::string &extra, bool extra_is_assist, PackedReads &local,
                     PackedReads::Mark &mk) {
    PackedReads &pr = g_sess.active ? g_sess.lib : local;
    if (!(g_sess.active && g_sess.lib_loaded && g_sess.lib_key == bin_path)) {
        if (g_sess.active) { g_sess.lib = PackedReads(); g_sess.lib_loaded = false; }
        if (!lib_prefix.empty()) load_read_lib(lib_prefix, /*reverse=*/true, pr);       // cx1_read2sdbg_s1.cpp:97,117
        else load_read_bin(bin_path, /*reverse=*/true, pr);
        if (g_sess.active) { g_sess.lib_loaded = true; g_sess.lib_key = bin_path; g_sess.lib_mark = pr.mark(); g_sess.extra_key.clear(); g_sess.have_extra = false; }
        else g_sess.lib_mark = pr.mark();
    }
    mk = g_sess.lib_mark;
    // the contigs this worker's own denovo has just made: taken from their text in memory (the file may still be on its way to the disk)
    // (the same FILE however it is spelled -- relative, `//`, a symlinked directory: compared by device + inode once the writer has
    // created it, by name before; advisor r5)
    auto same_file = [](const std::string &a, const std::string &b) {
        if (a == b) return true;
        struct stat sa, sb;
        return !a.empty() && !b.empty() && stat(a.c_str(), &sa) == 0 && stat(b.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
    };
    const bool from_memory = g_sess.active && !extra.empty() && !g_sess.ctext_path.empty() && same_file(extra, g_sess.ctext_path);
    // any other extra file is read from the disk: never while the background writer may still be in the middle of one
    if (g_sess.active && !extra.empty() && !from_memory && g_sess.cwriter.joinable() && contigs_join(false) != 0) die("the contigs of the last denovo are incomplete");
    const std::string key = extra.empty() ? std::string() : from_memory ? "mem|" + extra : file_key(extra);
    if (g_sess.active && g_sess.have_extra && g_sess.extra_key == key) {
        logf("library%s: still in memory", extra.empty() ? "" : " + contigs");
        return pr;
    }
    pr.rewind(mk);
    if (!extra.empty()) {
        if (from_memory && g_sess.ctext) {
            const double t0 = now_s();
            load_fasta_text(g_sess.ctext, (size_t)g_sess.ctext_len, /*reverse=*/true, pr);
            logf("contigs of %s: %zu sequences packed from memory (%.3f s)", extra.c_str(), pr.start.size() - mk.n_start, now_s() - t0);
            if (g_sess.cwriter_done.load()) contigs_join(true);                          // (written already: the text has served)
        } else {
            if (from_memory && contigs_join(true) != 0) die("%s is incomplete", extra.c_str());   // (the text is gone: the file is complete by now)
            if (extra_is_assist) load_assist_fasta(extra, /*reverse=*/true, pr);        // :121-134
            else load_fastx(extra, true, pr);
        }
    }
    pr.finish();
    if (g_sess.active) { g_sess.extra_key = key; g_sess.have_extra = true; }
    return pr;
}
PackedReads &reads_open(const std::string &lib, PackedReads &local, uint64_t *n_reads) {
    PackedReads::Mark mk;
    PackedReads &pr = lib_get(lib + ".bin", lib, "", false, local, mk);
    *n_reads = pr.start.size() - 1;
    return pr;
}
mgta_reads *reads_upload(mgta_ctx *ctx, const PackedReads &pr) {
    mgta_reads *rd = nullptr;
    if (mgta_reads_upload(ctx, pr.words.data(), pr.words.size(), pr.start.data(), pr.start.size() - 1, &rd) != MGTA_OK) die("mgta_reads_upload: %s", mgta_last_error());
    return rd;
}

// ---- the graphs of a worker: ONE policy ------------------------------------------------------------------------------------------------
// A worker holds at most three graphs on the device, and a step obtains a graph in one of three ways:
//   graph_take     the graph the last `buildgraph` left resident under this prefix, which the step consumes (denovo and search free it);
//                  else the files are loaded for this step alone.
//   graph_counted  a graph WITH multiplicities (coverage, sharecov): the counted graph of the same files; else a load with the switch on,
//                  kept as `cov_graph`.  (A graph a buildgraph hands over has no counts: the first coverage of a run loads.)
//   graph_any      any graph of these files (matchreads, samplecov, pileup): the counted graph first, then the match graph; else a load
//                  without multiplicities, kept as `match_graph`.
// "The same files" is the index file's path, size and modification time.  A load always drops ALL three resident graphs first, and
// writer_join() runs before any file is read or looked at.  A one-shot process keeps nothing: every way loads, graph_done frees.
void graph_drop() {
    if (g_sess.graph) { mgta_sdbg_free(g_sess.graph); g_sess.graph = nullptr; g_sess.graph_prefix.clear(); }
    if (g_sess.cov_graph) { mgta_sdbg_free(g_sess.cov_graph); g_sess.cov_graph = nullptr; g_sess.cov_key.clear(); }
    if (g_sess.match_graph) { mgta_sdbg_free(g_sess.match_graph); g_sess.match_graph = nullptr; g_sess.match_key.clear(); }
}
static mgta_sdbg *graph_load(mgta_ctx *ctx, const std::string &prefix, bool counted) {
    mgta_sdbg *g = nullptr;                                              // the files are copied to the device as they are and parsed there
    if (counted) mgta_ctx_keep_multiplicity(ctx, 1);
    const int lrc = mgta_sdbg_load_files(ctx, prefix.c_str(), &g);
    if (counted) mgta_ctx_keep_multiplicity(ctx, 0);
    if (lrc != MGTA_OK) die("mgta_sdbg_load_files: %s", mgta_last_error());
    return g;
}
mgta_sdbg *graph_take(mgta_ctx *ctx, const std::string &prefix, int *k_out, size_t *n_edges) {
    mgta_sdbg *g = nullptr;
    if (g_sess.active && g_sess.graph && g_sess.graph_prefix == prefix) {
        g = g_sess.graph;
        g_sess.graph = nullptr; g_sess.graph_prefix.clear();
        logf("graph %s: still on the device", prefix.c_str());
    } else {
        graph_drop();
        if (writer_join() != 0) die("the graph files of %s are incomplete", prefix.c_str());
        g = graph_load(ctx, prefix, false);
    }
    *k_out = mgta_sdbg_k(g); *n_edges = (size_t)mgta_sdbg_size(g);
    return g;
}
static mgta_sdbg *graph_kept(mgta_ctx *ctx, const std::string &prefix, double t0, bool counted) {
    if (writer_join() != 0) die("the graph files of %s are incomplete", prefix.c_str());
    const std::string key = file_key(prefix + ".sdbg_info");
    mgta_sdbg *g = nullptr;
    if (g_sess.active && g_sess.cov_graph && g_sess.cov_key == key) g = g_sess.cov_graph;
    else if (!counted && g_sess.active && g_sess.match_graph && g_sess.match_key == key) g = g_sess.match_graph;
    if (g) logf("graph %s%s: still on the device", prefix.c_str(), counted ? " with multiplicities" : "");
    else {
        graph_drop();
        g = graph_load(ctx, prefix, counted);
        if (g_sess.active) { (counted ? g_sess.cov_graph : g_sess.match_graph) = g; (counted ? g_sess.cov_key : g_sess.match_key) = key; }
    }
    logf("Number of Edges: %lld; K value: %d (load %s%.3f s)", (long long)mgta_sdbg_size(g), mgta_sdbg_k(g), counted ? "with multiplicities " : "", now_s() - t0);
    return g;
}
mgta_sdbg *graph_counted(mgta_ctx *ctx, const std::string &prefix, double t0) { return graph_kept(ctx, prefix, t0, true); }
mgta_sdbg *graph_any(mgta_ctx *ctx, const std::string &prefix, double t0) { return graph_kept(ctx, prefix, t0, false); }
void graph_done(mgta_sdbg *g) { if (!g_sess.active) mgta_sdbg_free(g); }   // (a worker's cov_graph / match_graph stay for the next step)

// ---- what buildgraph, search and denovo leave with a worker ---------------------------------------------------------------------------
mgta_stream *graph_hand_over(mgta_ctx *ctx, const std::string &prefix, bool detach_stream) {
    if (mgta_sdbg_load_resident(ctx, &g_sess.graph) != MGTA_OK) die("mgta_sdbg_load_resident: %s", mgta_last_error());
    g_sess.graph_prefix = prefix;
    // the stream leaves the context in one piece: the writer thread brings it to the host and writes the files
    if (detach_stream && mgta_sdbg_stream_detach(ctx, &g_sess.stream) != MGTA_OK) die("mgta_sdbg_stream_detach: %s", mgta_last_error());
    mgta_ctx_keep_stream(ctx, 0);
    return detach_stream ? g_sess.stream : nullptr;
}
void graph_writer_start(std::function<void()> write_files) {
    g_sess.writer = std::thread([write_files]() {
        set_soft_die(true);
        try { write_files(); }
        catch (const std::exception &e) { g_sess.writer_error = e.what(); }
    });
}
void contigs_keep(char *text, uint64_t len, const std::string &path, std::function<void(const char *, uint64_t)> write) {
    g_sess.ctext = text; g_sess.ctext_len = len; g_sess.ctext_path = path;
    g_sess.cwriter_done = false;
    g_sess.cwriter = std::thread([write, text, len]() {
        set_soft_die(true);
        try { write(text, len); }
        catch (const std::exception &e) { g_sess.cwriter_error = e.what(); }
        g_sess.cwriter_done = true;
    });
}

// ---- the sub-commands: one table for the dispatch, the usage text and the list of what is built here ------------------------------------
struct Command { const char *name; SubCommand *run; const char *help; };   // help: the line of the usage text, nullptr = not listed there
static const Command kCommands[] = {
    {"buildgraph", main_buildgraph, "build succinct de Bruijn graph"},
    {"denovo", main_denovo, "tips, bubbles, contigs of an intermediate k"},
    {"search", main_search, "HMM-guided search of gene contigs"},
    {"findstart", main_findstart, "find starting kmers of the search"},
    {"coverage", main_coverage, "per-contig k-mer coverage and abundance from the graph"},
    {"sharecov", main_sharecov, "per-contig coverage shared among the windows of the file: masses that add up"},
    {"matchreads", main_matchreads, "the reads that share a (k+1)-mer with a set of contigs"},
    {"samplecov", main_samplecov, "per-library coverage of a set of contigs, counted from the reads"},
    {"pileup", main_pileup, "the reads placed on a set of contigs: per-base depth and variants"},
    {"derep", main_derep, "the unique, non-contained records of a FASTA"},
    {"align", main_align, "protein records placed on the columns of a profile HMM"},
    {"posterior", main_posterior, "Forward score and per-residue confidence of aligned protein records"},
    {"cluster", main_cluster, "complete-linkage clusters of aligned protein records"},
    {"clustertree", main_clustertree, "those clusters at several cut-offs from one merge tree"},
    {"nearest", main_nearest, "the closest reference protein of every protein record"},
    {"chimera", main_chimera, "protein records that two references explain better than one"},
    {"filterbylen", main_filterbylen, nullptr},
    {"translate", main_translate, nullptr},
    {"buildlib", main_buildlib, nullptr},
    {nullptr, nullptr, nullptr},                                         // behind this row: not named as "built here" (version, the tests' commands)
    {"dumpversion", main_dumpversion, "dump version"},
    {"libdump", main_libdump, nullptr},
    {"sdbgcopy", main_sdbgcopy, nullptr},
    {"sdbgmerge", main_sdbgmerge, nullptr},
    {"hmmdump", main_hmmdump, nullptr},
    {"searchplan", main_searchplan, nullptr},
    {"recruit", main_recruit, nullptr},                                  // (the usage text and the "built here" list are pinned as recorded: tests/golden/cli_errors)
};
static int dispatch(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "Usage: %s <sub_program> [sub options]\n    sub-programs on the MI355X hot path:\n", argv[0]);
        for (const Command &c : kCommands)
            if (c.help) fprintf(stderr, "        %-14s%s\n", c.name, c.help);
        return 1;
    }
    const std::string sub = argv[1];
    for (const Command &c : kCommands)
        if (c.name && sub == c.name) return c.run(argc - 1, argv + 1);
    std::string built;
    for (const Command *c = kCommands; c->name; ++c) built += std::string(built.empty() ? "" : ", ") + c->name;
    fprintf(stderr, "sub-command '%s' is not built here (%s are): run it with the reference's megagta binary\n", sub.c_str(), built.c_str());
    return 1;
}

// megagta serve: requests on stdin, one per line: the sub-command's argv, tab separated; a field "<PATH" / ">PATH" redirects the
// step's stdin / stdout (filterbylen, translate, findstart).  Reply "DONE <exit code>" on the descriptor stdout had at start.  A step
// that dies takes the worker with it: the driver then reports the step as failed, as it does for a one-shot process.
static int main_serve() {
    g_sess.active = true;
    FILE *req = fdopen(dup(0), "r"), *rep = fdopen(dup(1), "w");
    if (!req || !rep) die("serve: cannot duplicate the standard descriptors");
    const int null_in = open("/dev/null", O_RDONLY);
    dup2(null_in, 0);                                                     // steps never read the request channel
    dup2(2, 1);                                                           // ... nor write into the reply channel: a step's stdout that no ">PATH" field
                                                                          // redirects (dumpversion, a stray printf) goes to stderr, never between the DONE lines
    char *line = nullptr;
    size_t cap = 0;
    ssize_t n;
    while ((n = getline(&line, &cap, req)) > 0) {
        while (n > 0 && (line[n - 1] == '\n' || line[n - 1] == '\r')) line[--n] = 0;
        if (n == 0) continue;
        std::vector<std::string> f;
        for (char *p = line, *e; ; p = e + 1) {
            e = strchr(p, '\t');
            f.emplace_back(p, e ? (size_t)(e - p) : strlen(p));
            if (!e) break;
        }
        if (f[0] == "quit") break;
        if (f[0] == "sync") {                                             // the files of the last buildgraph / denovo are on disk (or: why not)
            const int crc = contigs_join(false);
            fprintf(rep, "DONE %d\n", writer_join() | crc);
            fflush(rep);
            continue;
        }
        if (f[0] == "release") {                                          // hand the device memory back (another process is going to need it:
            graph_drop();                                                 // it reads the graph from the files, so they are complete first)
            const int wrc = writer_join() | contigs_join(true);
            if (g_sess.ctx) mgta_ctx_release_scratch(g_sess.ctx);
            if (g_sess.ctx2) mgta_ctx_release_scratch(g_sess.ctx2);
            fprintf(rep, "DONE %d\n", wrc);
            fflush(rep);
            continue;
        }
        std::string in_path, out_path;
        std::vector<char *> av;
        static char prog[] = "megagta";
        av.push_back(prog);
        for (std::string &x : f) {
            if (!x.empty() && x[0] == '<') in_path = x.substr(1);
            else if (!x.empty() && x[0] == '>') out_path = x.substr(1);
            else av.push_back(const_cast<char *>(x.c_str()));
        }
        av.push_back(nullptr);
        int save_in = -1, save_out = -1, rc = 1;
        fflush(stdout);
        if (!in_path.empty()) {
            int fd = open(in_path.c_str(), O_RDONLY);
            if (fd < 0) { fprintf(stderr, "serve: cannot open %s\n", in_path.c_str()); goto reply; }
            save_in = dup(0); dup2(fd, 0); close(fd);
            clearerr(stdin);
        }
        if (!out_path.empty()) {
            int fd = open(out_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
            if (fd < 0) { fprintf(stderr, "serve: cannot write %s\n", out_path.c_str()); goto reply; }
            save_out = dup(1); dup2(fd, 1); close(fd);
        }
        rc = dispatch((int)av.size() - 1, av.data());
    reply:
        fflush(stdout);
        if (save_out >= 0) { dup2(save_out, 1); close(save_out); }
        if (save_in >= 0) { dup2(save_in, 0); close(save_in); clearerr(stdin); }
        fprintf(rep, "DONE %d\n", rc);
        fflush(rep);
    }
    graph_drop();
    const int wrc = writer_join() | contigs_join(true);
    if (g_sess.ctx2) mgta_ctx_destroy(g_sess.ctx2);
    if (g_sess.ctx) mgta_ctx_destroy(g_sess.ctx);
    return wrc;
}

}  // namespace mgta_cli

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "serve") return mgta_cli::main_serve();
    return mgta_cli::dispatch(argc, argv);
}
