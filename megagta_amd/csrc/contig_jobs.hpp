// contig_jobs.hpp — the host side of every call that takes a set of contigs (seqs + offsets): the check of the offsets, the cut of the
// contigs into batches of at most `cap` windows, the job list of a batch (one strand or both, longest first) and the window offsets.
// mgta_contig_coverage, mgta_reads_match_contigs, mgta_contig_share_coverage, mgta_contig_sample_coverage (coverage.hip) and
// mgta_reads_pileup (pileup.hip) are written on it.  Plain C++ (no HIP headers): a stand-alone host check (host/contig_jobs_check.cpp)
// shares it with the library and brings its own set_error.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace mgta {

void set_error(const char *fmt, ...);     // (common.hpp; defined by the library, and by the host check for itself)

struct CovJob {                           // one strand of one contig of a batch
    uint64_t off;                         // its first letter in the batch's symbols
    uint64_t win_base;                    // its first window in the batch's per-window scratch
    uint32_t len, idx;                    // letters; one strand: the contig's number inside the batch, both: 2 * number + strand
};

constexpr uint64_t kMaxContigLetters = 0xFFFFFFF0ull;     // the length cap of the calls that have one (max_len below)
constexpr uint64_t kMaxCallWindows = 0xFFFFFFFFull;       // the window cap of the calls whose shares are 32-bit counts (max_win below)

inline uint64_t contig_windows(uint64_t len, uint64_t k) { return len > k ? len - k : 0; }

// The offsets of n contigs: they ascend, no contig is longer than max_len (0 = no cap), letters come with seqs, and the call holds at
// most max_win windows (0 = no cap).  false with the error set, in the name of `who`, at the first contig that breaks a rule.
// Out (either may be NULL): the windows of the call and of its longest contig.
inline bool check_contigs(const char *who, const char *seqs, const uint64_t *offsets, int64_t n, uint64_t k, uint64_t max_len, uint64_t max_win, uint64_t *total_win,
                          uint64_t *longest_win) {
    uint64_t total = 0, longest = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i] || (max_len && offsets[i + 1] - offsets[i] > max_len) || (offsets[i + 1] > offsets[i] && !seqs)) {
            set_error("%s: contig %lld: offsets must ascend%s", who, (long long)i, max_len ? ", a contig holds < 2^32 letters" : "");
            return false;
        }
        const uint64_t wn = contig_windows(offsets[i + 1] - offsets[i], k);
        total += wn;
        longest = std::max(longest, wn);
        if (max_win && total > max_win) {
            set_error("%s: more than 2^32 - 1 windows in the call (a share is a 32-bit count); contig %lld is the first beyond", who, (long long)i);
            return false;
        }
    }
    if (total_win) *total_win = total;
    if (longest_win) *longest_win = longest;
    return true;
}

// The batch that starts at contig c0: the contigs [c0, c1) -- as many as hold at most `cap` windows together, one at least -- as jobs,
// c1 returned.  Offsets and window bases count from the batch's first letter and window.  both_strands: every contig is a second job
// for its reverse complement, which lies mirrored behind the batch's n_bytes symbols (the reverse complement of [a, a + len) at
// [2 n_bytes - a - len, 2 n_bytes - a)) and whose windows lie n_win behind the contig's.  The jobs leave longest first, so that no
// group starts a long contig when the others are about to finish; ties by idx: the order is fixed.
inline int64_t cut_batch(const uint64_t *offsets, int64_t n, uint64_t k, int64_t c0, uint64_t cap, bool both_strands, std::vector<CovJob> &jobs, uint64_t *n_win_out) {
    int64_t c1 = c0;
    uint64_t n_win = 0;
    jobs.clear();
    while (c1 < n) {
        const uint64_t len = offsets[c1 + 1] - offsets[c1], wn = contig_windows(len, k);
        if (c1 > c0 && n_win + wn > cap) break;
        jobs.push_back(CovJob{offsets[c1] - offsets[c0], n_win, (uint32_t)len, (uint32_t)(c1 - c0) * (both_strands ? 2u : 1u)});
        n_win += wn;
        ++c1;
    }
    if (both_strands) {
        const uint64_t n_bytes = offsets[c1] - offsets[c0];
        const size_t n_given = jobs.size();
        for (size_t j = 0; j < n_given; ++j) {
            const CovJob f = jobs[j];
            jobs.push_back(CovJob{2 * n_bytes - f.off - f.len, n_win + f.win_base, f.len, f.idx + 1u});
        }
    }
    std::sort(jobs.begin(), jobs.end(), [](const CovJob &a, const CovJob &b) { return a.len != b.len ? a.len > b.len : a.idx < b.idx; });
    *n_win_out = n_win;
    return c1;
}

// the first window of every contig in the call's per-window outputs, [n + 1]; lens (or NULL): the letters of every contig
inline std::vector<uint64_t> window_offsets(const uint64_t *offsets, int64_t n, uint64_t k, std::vector<uint32_t> *lens = nullptr) {
    std::vector<uint64_t> woff((size_t)n + 1, 0);
    if (lens) lens->resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        if (lens) (*lens)[(size_t)i] = (uint32_t)len;
        woff[(size_t)i + 1] = woff[(size_t)i] + contig_windows(len, k);
    }
    return woff;
}

}  // namespace mgta
