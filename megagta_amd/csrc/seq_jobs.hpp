// seq_jobs.hpp — the host side of every call that takes a set of protein sequences (seqs + offsets): the checks of the count, the
// offsets and the letters, the offsets relative to the first letter, the order longest first, the cut of that order into batches of at
// most `cap` cells, the reference columns (one class byte per residue of the concatenated references) and the waves a workgroup gets
// for the LDS rows its waves need.  mgta_seqs_derep (its checks and offsets), mgta_seqs_align, mgta_seqs_posterior, mgta_seqs_nearest
// and mgta_seqs_chimera are written on it.  Plain C++ (no HIP headers): a stand-alone host check (host/seq_jobs_check.cpp) shares it
// with the library and brings its own set_error.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#if defined(__HIPCC__)
#define MGTA_HD __host__ __device__
#else
#define MGTA_HD
#endif

namespace mgta {

void set_error(const char *fmt, ...);     // (common.hpp; defined by the library, and by the host check for itself)

// what a set is called in the error texts: its items, and the arguments that hold their number, their offsets and their letters
struct SeqWords { const char *noun, *count, *offsets, *letters; };
constexpr SeqWords kSequences{"sequence", "n", "offsets", "seqs"}, kContigs{"contig", "n", "offsets", "seqs"}, kReferences{"reference", "n_ref", "ref_offsets", "refs"};

// The three checks of a set, apart because every entry point has checks of its own between them and the first error wins: false with
// the error set in the name of `who`.
inline bool check_seq_count(const char *who, const SeqWords &w, int64_t n) {
    if (n < (1ll << 31)) return true;
    set_error("%s: %s = %lld (the limit is %s < 2^31 %ss)", who, w.count, (long long)n, w.count, w.noun);
    return false;
}

// the offsets ascend and no item holds more than max_len `unit`; limit (or NULL: "<max_len> <unit> per <noun>") is how the text names the cap
inline bool check_seq_offsets(const char *who, const SeqWords &w, const uint64_t *offsets, int64_t n, uint64_t max_len, const char *unit = "residues", const char *limit = nullptr) {
    for (int64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) { set_error("%s: %s %lld: %s must ascend", who, w.noun, (long long)i, w.offsets); return false; }
        if (offsets[i + 1] - offsets[i] > max_len) {
            char own[96];
            std::snprintf(own, sizeof own, "%llu %s per %s", (unsigned long long)max_len, unit, w.noun);
            set_error("%s: %s %lld holds %llu %s (the limit is %s)", who, w.noun, (long long)i, (unsigned long long)(offsets[i + 1] - offsets[i]), unit, limit ? limit : own);
            return false;
        }
    }
    return true;
}

inline bool check_seq_letters(const char *who, const SeqWords &w, const void *letters, uint64_t n_letters) {
    if (!n_letters || letters) return true;
    set_error("%s: %s must not be NULL", who, w.letters);
    return false;
}

// all references of a call are one run of columns, and a column number is 31 bits
inline bool check_ref_columns(const char *who, uint64_t n_cols) {
    if (n_cols < (1ull << 31)) return true;
    set_error("%s: the references hold %llu residues together (the limit is fewer than 2^31 residues in all references)", who, (unsigned long long)n_cols);
    return false;
}

// offsets counted from the first letter of the call, [n + 1]
inline std::vector<uint64_t> rel_offsets(const uint64_t *offsets, int64_t n) {
    std::vector<uint64_t> rel((size_t)n + 1);
    for (int64_t i = 0; i <= n; ++i) rel[(size_t)i] = offsets[i] - offsets[0];
    return rel;
}

// 0 .. n - 1, longest first, so that no wave starts a long item when the others are about to finish; equal lengths stay in input order
template <class LenOf> std::vector<uint32_t> longest_first(uint32_t n, LenOf len_of) {
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return len_of(x) > len_of(y); });
    return order;
}
inline std::vector<uint32_t> longest_first(const std::vector<uint64_t> &rel) {
    return longest_first((uint32_t)rel.size() - 1, [&](uint32_t i) { return rel[i + 1] - rel[i]; });
}

// The batch that starts at item b0 of n: the items [b0, b1) -- as many as hold at most `cap` cells together, one at least -- b1
// returned.  Item k has len_of(k) * width_of(k) cells (the model's columns for every item, or the columns of the item's own
// reference) and a path slot of len_of(k) + width_of(k) bytes; cell_base and path_base (or NULL) take the running sums, [b1 - b0].
template <class LenOf, class WidthOf>
uint32_t cut_cells(uint32_t b0, uint32_t n, uint64_t cap, LenOf len_of, WidthOf width_of, std::vector<uint64_t> &cell_base, std::vector<uint64_t> *path_base, uint64_t *cells_out,
                   uint64_t *path_bytes_out = nullptr) {
    uint32_t b1 = b0;
    uint64_t cells = 0, path_bytes = 0;
    cell_base.clear();
    if (path_base) path_base->clear();
    while (b1 < n) {
        const uint64_t L = len_of(b1), W = width_of(b1);
        if (b1 > b0 && cells + L * W > cap) break;
        cell_base.push_back(cells);
        if (path_base) path_base->push_back(path_bytes);
        cells += L * W; path_bytes += L + W;
        ++b1;
    }
    *cells_out = cells;
    if (path_bytes_out) *path_bytes_out = path_bytes;
    return b1;
}

// 1 .. 26 for an ASCII letter of either case, else 0
MGTA_HD inline uint32_t residue_class(uint32_t b) {
    const uint32_t c = (b | 32u) - 'a';
    return (b < 128u && c < 26u) ? c + 1u : 0u;
}

constexpr uint32_t kFirstColumn = 32;     // bit of a column's byte: the first column of its reference (bits 0-4: the class)

// The columns of the references: rstart [n_ref + 1] where every reference starts in the run (from ref_offsets[0]), rcls one byte per
// column, the class of its residue, | kFirstColumn on the first column of every reference that has residues.
inline void ref_columns(const char *refs, const uint64_t *ref_offsets, int64_t n_ref, std::vector<uint32_t> &rstart, std::vector<uint8_t> &rcls) {
    rstart.resize((size_t)n_ref + 1);
    for (int64_t r = 0; r <= n_ref; ++r) rstart[(size_t)r] = (uint32_t)(ref_offsets[r] - ref_offsets[0]);
    const uint32_t nc = rstart[(size_t)n_ref];
    rcls.resize(nc);
    for (uint32_t g = 0; g < nc; ++g) rcls[g] = (uint8_t)residue_class((unsigned char)refs[ref_offsets[0] + g]);
    for (int64_t r = 0; r < n_ref; ++r)
        if (rstart[(size_t)r + 1] > rstart[(size_t)r]) rcls[rstart[(size_t)r]] |= kFirstColumn;
}

// waves of a workgroup (4, 2 or 1): as many as keep `fixed` bytes and rows_lds rows of row_bytes per wave inside the LDS budget
inline int waves_that_fit(size_t rows_lds, size_t row_bytes, size_t fixed, size_t budget) {
    int waves = 4;
    while (waves > 1 && fixed + (size_t)waves * rows_lds * row_bytes > budget) waves >>= 1;
    return waves;
}

}  // namespace mgta
