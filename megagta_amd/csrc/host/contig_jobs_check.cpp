// contig_jobs_check.cpp — stand-alone check of contig_jobs.hpp (no device, no HIP): the batches of cut_batch tile the contigs in order
// and respect the window cap, the jobs' window bases tile the batch's scratch on both strands, the reverse-complement offsets are the
// mirrored ones, the order is longest first, and check_contigs refuses what it must with the text the library has always given.
// Build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all host/contig_jobs_check.cpp -o contig_jobs_check
// and run it: it prints "ok" and returns 0, or says what failed.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../contig_jobs.hpp"

static std::string g_error;

namespace mgta {
void set_error(const char *fmt, ...) {    // the library's keeps the text for mgta_last_error; this one keeps it for the comparisons below
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
}
}  // namespace mgta

using namespace mgta;

static int fail(const char *what, uint64_t a, uint64_t b) {
    std::fprintf(stderr, "contig_jobs_check: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

// one set of contigs cut with one cap, one strand or both; returns non-zero on a violated property
static int check_cut(const std::vector<uint64_t> &off, uint64_t k, uint64_t cap, bool both) {
    const int64_t n = (int64_t)off.size() - 1;
    const std::vector<uint64_t> woff = window_offsets(off.data(), n, k);
    std::vector<CovJob> jobs;
    for (int64_t c0 = 0; c0 < n;) {
        uint64_t n_win = 0;
        const int64_t c1 = cut_batch(off.data(), n, k, c0, cap, both, jobs, &n_win);
        if (c1 <= c0 || c1 > n) return fail("a batch holds no contig, or contigs beyond the last", (uint64_t)c0, (uint64_t)c1);
        if (n_win != woff[(size_t)c1] - woff[(size_t)c0]) return fail("n_win is not the windows of the batch's contigs", n_win, woff[(size_t)c1] - woff[(size_t)c0]);
        if (n_win > cap && c1 - c0 != 1) return fail("a batch of several contigs above the cap", n_win, cap);
        if (c1 < n && n_win + contig_windows(off[(size_t)c1 + 1] - off[(size_t)c1], k) <= cap) return fail("the next contig would have fitted", (uint64_t)c1, cap);
        const size_t per_strand = (size_t)(c1 - c0);
        if (jobs.size() != per_strand * (both ? 2 : 1)) return fail("job count", jobs.size(), per_strand);
        const uint64_t n_bytes = off[(size_t)c1] - off[(size_t)c0];
        std::vector<int> seen(jobs.size(), 0);
        for (size_t j = 0; j < jobs.size(); ++j) {
            const CovJob &job = jobs[j];
            if (j && (jobs[j - 1].len < job.len || (jobs[j - 1].len == job.len && jobs[j - 1].idx >= job.idx))) return fail("not (len descending, idx ascending)", j, job.idx);
            if (job.idx >= jobs.size() || seen[job.idx]++) return fail("idx out of range or twice", job.idx, j);
            const size_t c = (size_t)c0 + (both ? job.idx / 2 : job.idx);
            const bool rc = both && (job.idx & 1);
            const uint64_t a = off[c] - off[(size_t)c0], len = off[c + 1] - off[c];
            if (job.len != len) return fail("len", job.len, len);
            // the windows of the contigs in contig order tile [0, n_win) on the given strand and [n_win, 2 n_win) on the other
            if (job.win_base != woff[c] - woff[(size_t)c0] + (rc ? n_win : 0)) return fail("win_base", job.win_base, woff[c] - woff[(size_t)c0]);
            if (job.off != (rc ? 2 * n_bytes - a - len : a)) return fail("off", job.off, a);
            if (job.off + len > (both ? 2 : 1) * n_bytes) return fail("a job beyond the batch's symbols", job.off + len, n_bytes);
        }
        c0 = c1;                                                           // (the batches tile [0, n) in order: each starts where the last ended)
    }
    return 0;
}

static int expect_refused(const char *what, bool ok, const char *text) {
    if (ok) return fail(what, 0, 0);
    if (g_error != text) {
        std::fprintf(stderr, "contig_jobs_check: %s: \"%s\" instead of \"%s\"\n", what, g_error.c_str(), text);
        return 1;
    }
    return 0;
}

int main() {
    std::mt19937_64 rng(20241020);
    for (int rep = 0; rep < 400; ++rep) {
        const uint64_t k = 1 + rng() % 40;
        const int64_t n = 1 + (int64_t)(rng() % 30);
        std::vector<uint64_t> off((size_t)n + 1, rng() % 3 ? 0 : rng() % 1000);    // (offsets need not start at 0)
        uint64_t one = 0;
        for (int64_t i = 0; i < n; ++i) {
            uint64_t len = rng() % (3 * k + 1);                            // 0 .. 3k letters
            const int shape = (int)(rng() % 8);
            if (shape == 0) len = 0;
            if (shape == 1) len = k;                                       // no window
            if (shape == 2) len = k + 1;                                   // exactly one
            off[(size_t)i + 1] = off[(size_t)i] + len;
            if (contig_windows(len, k)) one = contig_windows(len, k);
        }
        const uint64_t caps[] = {1, one ? one : 1, ~0ull, 1 + rng() % (4 * k)};
        for (uint64_t cap : caps)
            for (int both = 0; both < 2; ++both)
                if (check_cut(off, k, cap, both != 0)) return 1;
        uint64_t total = 0, longest = 0, want_total = 0, want_longest = 0;
        for (int64_t i = 0; i < n; ++i) {
            const uint64_t wn = contig_windows(off[(size_t)i + 1] - off[(size_t)i], k);
            want_total += wn;
            want_longest = std::max(want_longest, wn);
        }
        const std::string seqs((size_t)(off[(size_t)n] - off[0]) + 1, 'A');
        if (!check_contigs("who", seqs.data(), off.data(), n, k, kMaxContigLetters, kMaxCallWindows, &total, &longest)) return fail("valid offsets refused", (uint64_t)rep, 0);
        if (total != want_total || longest != want_longest) return fail("total_win / longest_win", total, longest);
    }
    // what check_contigs refuses, and its words
    const char seqs[] = "ACGT";
    const uint64_t descending[] = {0, 10, 5}, too_long[] = {0, 1, 2, 2 + kMaxContigLetters + 1}, fine[] = {0, 2, 4};
    if (expect_refused("descending offsets", check_contigs("mgta_contig_coverage", seqs, descending, 2, 20, kMaxContigLetters, 0, nullptr, nullptr),
                       "mgta_contig_coverage: contig 1: offsets must ascend, a contig holds < 2^32 letters")) return 1;
    if (expect_refused("descending offsets, no length cap", check_contigs("mgta_reads_pileup", seqs, descending, 2, 20, 0, 0, nullptr, nullptr),
                       "mgta_reads_pileup: contig 1: offsets must ascend")) return 1;
    if (expect_refused("a contig over the length cap", check_contigs("mgta_reads_match_contigs", seqs, too_long, 3, 20, kMaxContigLetters, 0, nullptr, nullptr),
                       "mgta_reads_match_contigs: contig 2: offsets must ascend, a contig holds < 2^32 letters")) return 1;
    uint64_t total = 0;
    if (!check_contigs("mgta_reads_pileup", seqs, too_long, 3, 20, 0, 0, &total, nullptr) || total != kMaxContigLetters + 1 - 20) return fail("no length cap asked, yet refused", total, 0);
    if (expect_refused("letters without seqs", check_contigs("mgta_contig_share_coverage", nullptr, fine, 2, 20, kMaxContigLetters, kMaxCallWindows, nullptr, nullptr),
                       "mgta_contig_share_coverage: contig 0: offsets must ascend, a contig holds < 2^32 letters")) return 1;
    const uint64_t empty[] = {7, 7, 7};
    if (!check_contigs("who", nullptr, empty, 2, 20, kMaxContigLetters, kMaxCallWindows, &total, nullptr) || total != 0) return fail("empty contigs need no seqs", total, 0);
    const uint64_t many[] = {0, kMaxContigLetters, 2 * kMaxContigLetters};
    if (expect_refused("more windows than a share counts", check_contigs("mgta_contig_sample_coverage", seqs, many, 2, 20, kMaxContigLetters, kMaxCallWindows, nullptr, nullptr),
                       "mgta_contig_sample_coverage: more than 2^32 - 1 windows in the call (a share is a 32-bit count); contig 1 is the first beyond")) return 1;
    std::puts("ok");
    return 0;
}
