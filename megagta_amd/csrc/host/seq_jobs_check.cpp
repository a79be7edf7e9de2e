// seq_jobs_check.cpp — stand-alone check of seq_jobs.hpp (no device, no HIP): the checks of a set of sequences refuse what they must
// with the text the library has always given at each of its seven call sites, the order is longest first and stable, cut_cells
// respects the cap with one item at least and keeps the running sums, ref_columns gives every column its class and the first-column
// bit, and waves_that_fit halves the waves exactly where the LDS budget says.  Build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all host/seq_jobs_check.cpp -o seq_jobs_check
// and run it: it prints "ok" and returns 0, or says what failed.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../seq_jobs.hpp"

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

static int fail(const char *what, uint64_t a = 0, uint64_t b = 0) {
    std::fprintf(stderr, "seq_jobs_check: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

static int expect_refused(const char *what, bool ok, const std::string &text) {
    if (ok) return fail(what);
    if (g_error != text) {
        std::fprintf(stderr, "seq_jobs_check: %s: \"%s\" instead of \"%s\"\n", what, g_error.c_str(), text.c_str());
        return 1;
    }
    return 0;
}

// one call site: who, its words, its cap and how its texts name the item and the cap
struct Site { const char *who; const SeqWords *w; uint64_t max_len; const char *unit, *limit, *descending, *over, *count, *null_letters; };

static int check_texts() {
    const char *first = "< 2^32 letters in the first occurrences";
    const Site sites[7] = {
        {"mgta_seqs_derep", &kSequences, 0xFFFFFFFFull, "letters", first, "mgta_seqs_derep: sequence 1: offsets must ascend",
         "mgta_seqs_derep: sequence 2 holds 4294967296 letters (the limit is < 2^32 letters in the first occurrences)",
         "mgta_seqs_derep: n = 2147483648 (the limit is n < 2^31 sequences)", "mgta_seqs_derep: seqs must not be NULL"},
        {"mgta_seqs_align", &kSequences, 4096, "residues", nullptr, "mgta_seqs_align: sequence 1: offsets must ascend",
         "mgta_seqs_align: sequence 2 holds 4097 residues (the limit is 4096 residues per sequence)",
         "mgta_seqs_align: n = 2147483648 (the limit is n < 2^31 sequences)", "mgta_seqs_align: seqs must not be NULL"},
        {"mgta_seqs_posterior", &kSequences, 4096, "residues", nullptr, "mgta_seqs_posterior: sequence 1: offsets must ascend",
         "mgta_seqs_posterior: sequence 2 holds 4097 residues (the limit is 4096 residues per sequence)",
         "mgta_seqs_posterior: n = 2147483648 (the limit is n < 2^31 sequences)", "mgta_seqs_posterior: seqs must not be NULL"},
        {"mgta_seqs_nearest", &kContigs, 4096, "residues", nullptr, "mgta_seqs_nearest: contig 1: offsets must ascend",
         "mgta_seqs_nearest: contig 2 holds 4097 residues (the limit is 4096 residues per contig)",
         "mgta_seqs_nearest: n = 2147483648 (the limit is n < 2^31 contigs)", "mgta_seqs_nearest: seqs must not be NULL"},
        {"mgta_seqs_nearest", &kReferences, 4096, "residues", nullptr, "mgta_seqs_nearest: reference 1: ref_offsets must ascend",
         "mgta_seqs_nearest: reference 2 holds 4097 residues (the limit is 4096 residues per reference)",
         "mgta_seqs_nearest: n_ref = 2147483648 (the limit is n_ref < 2^31 references)", "mgta_seqs_nearest: refs must not be NULL"},
        {"mgta_seqs_chimera", &kContigs, 4096, "residues", nullptr, "mgta_seqs_chimera: contig 1: offsets must ascend",
         "mgta_seqs_chimera: contig 2 holds 4097 residues (the limit is 4096 residues per contig)",
         "mgta_seqs_chimera: n = 2147483648 (the limit is n < 2^31 contigs)", "mgta_seqs_chimera: seqs must not be NULL"},
        {"mgta_seqs_chimera", &kReferences, 4096, "residues", nullptr, "mgta_seqs_chimera: reference 1: ref_offsets must ascend",
         "mgta_seqs_chimera: reference 2 holds 4097 residues (the limit is 4096 residues per reference)",
         "mgta_seqs_chimera: n_ref = 2147483648 (the limit is n_ref < 2^31 references)", "mgta_seqs_chimera: refs must not be NULL"},
    };
    for (const Site &s : sites) {
        const uint64_t descending[] = {0, 10, 5}, over[] = {3, 3, 5, 5 + s.max_len + 1}, at_cap[] = {3, 3, 5, 5 + s.max_len}, empty[] = {7, 7, 7};
        if (expect_refused("descending offsets", check_seq_offsets(s.who, *s.w, descending, 2, s.max_len, s.unit, s.limit), s.descending)) return 1;
        if (expect_refused("an item over the cap", check_seq_offsets(s.who, *s.w, over, 3, s.max_len, s.unit, s.limit), s.over)) return 1;
        if (!check_seq_offsets(s.who, *s.w, at_cap, 3, s.max_len, s.unit, s.limit)) return fail("an item at the cap refused");
        if (!check_seq_offsets(s.who, *s.w, nullptr, 0, s.max_len, s.unit, s.limit)) return fail("n = 0 refused");
        if (!check_seq_offsets(s.who, *s.w, empty, 2, s.max_len, s.unit, s.limit)) return fail("items of length 0 refused");
        if (expect_refused("n = 2^31", check_seq_count(s.who, *s.w, 1ll << 31), s.count)) return 1;
        if (!check_seq_count(s.who, *s.w, (1ll << 31) - 1) || !check_seq_count(s.who, *s.w, 0)) return fail("a count below 2^31 refused");
        if (expect_refused("letters and no text", check_seq_letters(s.who, *s.w, nullptr, 1), s.null_letters)) return 1;
        if (!check_seq_letters(s.who, *s.w, nullptr, 0) || !check_seq_letters(s.who, *s.w, "A", 1)) return fail("no letters, or letters with their text, refused");
    }
    for (const char *who : {"mgta_seqs_nearest", "mgta_seqs_chimera"}) {
        if (expect_refused("2^31 columns", check_ref_columns(who, 1ull << 31),
                           std::string(who) + ": the references hold 2147483648 residues together (the limit is fewer than 2^31 residues in all references)")) return 1;
        if (!check_ref_columns(who, (1ull << 31) - 1)) return fail("2^31 - 1 columns refused");
    }
    return 0;
}

static int check_order() {
    const uint64_t off[] = {100, 103, 103, 108, 111, 116, 116, 117};       // lengths 3 0 5 3 5 0 1, offsets not from 0
    const std::vector<uint64_t> rel = rel_offsets(off, 7);
    if (rel[0] != 0 || rel[7] != 17 || rel[3] != 8) return fail("rel_offsets", rel[7], rel[3]);
    const std::vector<uint32_t> order = longest_first(rel), want{2, 4, 0, 3, 6, 1, 5};
    if (order != want) return fail("longest first, equal lengths in input order");
    if (!longest_first(rel_offsets(off, 0)).empty()) return fail("the order of no item");
    return 0;
}

// batches of `len` x `wid` under `cap`: the sizes of the batches, and the running sums inside each
static int check_cut(const std::vector<uint64_t> &len, const std::vector<uint64_t> &wid, uint64_t cap, const std::vector<uint32_t> &want_sizes) {
    const uint32_t n = (uint32_t)len.size();
    std::vector<uint64_t> cell_base, path_base;
    std::vector<uint32_t> sizes;
    for (uint32_t b0 = 0; b0 < n;) {
        uint64_t cells = 0, path_bytes = 0;
        const uint32_t b1 = cut_cells(b0, n, cap, [&](uint32_t k) { return len[k]; }, [&](uint32_t k) { return wid[k]; }, cell_base, &path_base, &cells, &path_bytes);
        if (b1 <= b0 || b1 > n) return fail("a batch holds no item, or items beyond the last", b0, b1);
        if (cell_base.size() != b1 - b0 || path_base.size() != b1 - b0) return fail("bases per item", cell_base.size(), b1 - b0);
        uint64_t c = 0, p = 0;
        for (uint32_t k = b0; k < b1; ++k) {
            if (cell_base[k - b0] != c || path_base[k - b0] != p) return fail("cell_base / path_base are not the running sums", k, cap);
            c += len[k] * wid[k]; p += len[k] + wid[k];
        }
        if (cells != c || path_bytes != p) return fail("cells / path_bytes of the batch", cells, c);
        if (cells > cap && b1 - b0 != 1) return fail("a batch of several items above the cap", cells, cap);
        if (b1 < n && cells + len[b1] * wid[b1] <= cap) return fail("the next item would have fitted", b1, cap);
        std::vector<uint64_t> again;
        uint64_t cells2 = 0;
        if (cut_cells(b0, n, cap, [&](uint32_t k) { return len[k]; }, [&](uint32_t k) { return wid[k]; }, again, nullptr, &cells2) != b1 || cells2 != cells || again != cell_base)
            return fail("without path_base the cut differs", b0, b1);
        sizes.push_back(b1 - b0);
        b0 = b1;
    }
    if (sizes != want_sizes) return fail("batch sizes", sizes.size(), cap);
    return 0;
}

static int check_cuts() {
    const std::vector<uint64_t> len{9, 7, 7, 2}, m10(4, 10);             // 90, 70, 70, 20 cells: a model of 10 columns
    if (check_cut(len, m10, 1, {1, 1, 1, 1})) return 1;
    if (check_cut(len, m10, 90, {1, 1, 2})) return 1;                     // the first item's cells: the second waits
    if (check_cut(len, m10, 91, {1, 1, 2})) return 1;                     // one more: it still does
    if (check_cut(len, m10, 159, {1, 2, 1})) return 1;
    if (check_cut(len, m10, 160, {2, 2})) return 1;
    if (check_cut(len, m10, 250, {4})) return 1;                          // the sum: one batch
    if (check_cut(len, m10, ~0ull, {4})) return 1;
    const std::vector<uint64_t> holes{0, 5, 0, 0, 5, 0};
    if (check_cut(holes, std::vector<uint64_t>(6, 10), 50, {4, 2})) return 1;      // items of length 0 cost nothing
    if (check_cut(holes, std::vector<uint64_t>(6, 10), 1, {1, 1, 2, 1, 1})) return 1;   // ... but a batch already above the cap takes nothing more
    const std::vector<uint64_t> l2{4, 4, 3, 3}, w2{10, 2, 0, 7};          // widths per item, as in nearest's trace pass: 40, 8, 0, 21 cells
    if (check_cut(l2, w2, 40, {1, 3})) return 1;
    if (check_cut(l2, w2, 48, {3, 1})) return 1;
    if (check_cut(l2, w2, 69, {4})) return 1;
    return 0;
}

static int check_columns() {
    const struct { unsigned char b; uint32_t cls; } classes[] = {{'A', 1}, {'a', 1}, {'Z', 26}, {'z', 26}, {'@', 0}, {'[', 0}, {127, 0}, {128, 0}, {255, 0}, {'`', 0}, {'{', 0}, {'A' + 128, 0}, {'a' + 128, 0}};
    for (const auto &c : classes)
        if (residue_class(c.b) != c.cls) return fail("residue_class", c.b, residue_class(c.b));
    // empty references at the front, in the middle and at the end; ref_offsets[0] != 0
    const std::string text = std::string("###") + "Az" + "m*\xC1" + "Q";
    const uint64_t roff[] = {3, 3, 5, 5, 5, 8, 9, 9};
    std::vector<uint32_t> rstart;
    std::vector<uint8_t> rcls;
    ref_columns(text.data(), roff, 7, rstart, rcls);
    const std::vector<uint32_t> want_start{0, 0, 2, 2, 2, 5, 6, 6};
    const std::vector<uint8_t> want_cls{1 | 32, 26, 13 | 32, 0, 0, 17 | 32};
    if (rstart != want_start) return fail("rstart");
    if (rcls != want_cls) return fail("rcls: classes and the first-column bit");
    ref_columns(nullptr, roff + 2, 2, rstart, rcls);                       // only empty references: no column, and no letter is read
    if (!rcls.empty() || rstart != std::vector<uint32_t>{0, 0, 0}) return fail("references without residues");
    return 0;
}

static int check_waves() {
    // align's 16 B per row in 80 KB, posterior's 20 B in 82 KB, nearest's 9 B in 80 KB behind `sub`; the longest item (4 096 rows) leaves
    // align and posterior one wave and nearest, whose rows are small, two (864 + 2 * 4096 * 9 = 74 592 bytes)
    const struct { size_t row_bytes, fixed, budget, last4; int at_4096; } k[] = {{16, 128, 80 * 1024, 1278, 1}, {20, 128, 82 * 1024, 1048, 1}, {9, 27 * 32, 80 * 1024, 2251, 2}};
    for (const auto &g : k) {
        if (g.fixed + 4 * g.last4 * g.row_bytes > g.budget || g.fixed + 4 * (g.last4 + 1) * g.row_bytes <= g.budget) return fail("the check's own edge", g.row_bytes, g.last4);
        if (waves_that_fit(1, g.row_bytes, g.fixed, g.budget) != 4) return fail("one row", g.row_bytes);
        if (waves_that_fit(g.last4, g.row_bytes, g.fixed, g.budget) != 4) return fail("the last rows_lds of 4 waves", g.row_bytes, g.last4);
        if (waves_that_fit(g.last4 + 1, g.row_bytes, g.fixed, g.budget) != 2) return fail("one row more halves the waves", g.row_bytes, g.last4 + 1);
        if (waves_that_fit(4096, g.row_bytes, g.fixed, g.budget) != g.at_4096) return fail("the waves of 4096 rows", g.row_bytes);
        if (waves_that_fit(1 << 20, g.row_bytes, g.fixed, g.budget) != 1) return fail("never fewer than one wave", g.row_bytes);
    }
    return 0;
}

int main() {
    if (check_texts() || check_order() || check_cuts() || check_columns() || check_waves()) return 1;
    std::puts("ok");
    return 0;
}
