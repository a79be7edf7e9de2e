// segment_split_check.cpp — stand-alone check of segment_split.hpp (no device, no HIP): the packer's ranges tile the segment in
// order, respect the tile sizes, and stay within the bounds the list capacities of split_list_caps are derived from.  Build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all host/segment_split_check.cpp -o segment_split_check
// and run it: it prints "ok" and returns 0, or says what failed.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../segment_split.hpp"

using namespace mgta;

struct Range { uint32_t cls; uint64_t first, end; };

static int fail(const char *what, uint64_t a, uint64_t b) {
    std::fprintf(stderr, "segment_split_check: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

// one segment: counts of its digit values -> ranges; returns non-zero on a violated property
static int check_segment(const std::vector<uint64_t> &counts, uint64_t first, uint32_t local_tile, uint32_t lds_cap, uint64_t (&n_cls)[kSplitClasses]) {
    std::vector<Range> out;
    auto emit = [&](uint32_t cls, uint64_t a, uint64_t b) { out.push_back(Range{cls, a, b}); };
    SplitPacker pk(first, local_tile, lds_cap);
    for (uint64_t c : counts) pk.step(c, emit);
    pk.finish(emit);
    uint64_t cnt = 0, non_empty = 0;
    for (uint64_t c : counts) { cnt += c; non_empty += c > 0; }
    if (out.size() > non_empty) return fail("more ranges than non-empty digit values", out.size(), non_empty);
    uint64_t at = first, small = 0;
    size_t v = 0;                                                     // the ranges are whole pieces, in digit order
    for (const Range &r : out) {
        if (r.first != at || r.end <= r.first) return fail("ranges do not tile the segment in order", r.first, at);
        const uint64_t len = r.end - r.first;
        uint64_t got = 0, pieces = 0;
        while (got < len && v < counts.size()) { got += counts[v]; pieces += counts[v] > 0; ++v; }
        if (got != len) return fail("a range cuts a piece", got, len);
        if (r.cls == kSplitSmall) { if (len > local_tile) return fail("small range above the local tile", len, local_tile); ++small; }
        else if (r.cls == kSplitMid) { if (pieces != 1 || len <= local_tile || len > lds_cap) return fail("mid range out of its class", len, pieces); }
        else if (r.cls == kSplitNext) { if (pieces != 1 || len <= lds_cap) return fail("next range out of its class", len, pieces); }
        else return fail("unknown class", r.cls, 0);
        n_cls[r.cls]++;
        at = r.end;
    }
    if (at != first + cnt) return fail("ranges do not cover the segment", at, first + cnt);
    if (small > 2 * (cnt / local_tile) + 1) return fail("more small ranges than 2 cnt / tile + 1", small, cnt);
    return 0;
}

int main() {
    std::mt19937_64 rng(20240917);
    const uint32_t tiles[][2] = {{4096, 8192}, {2048, 4096}, {2048, 2048}, {64, 128}, {1, 1}};
    for (const auto &t : tiles) {
        const uint32_t local_tile = t[0], lds_cap = t[1];
        for (int rep = 0; rep < 140; ++rep) {
            // an array of n keys cut into segments; those longer than lds_cap are split (one level of the route)
            const uint64_t n = 1 + rng() % ((uint64_t)lds_cap * 64);
            const SplitCaps caps = split_list_caps(n, local_tile, lds_cap);
            uint64_t n_cls[kSplitClasses] = {0, 0, 0}, at = 0;
            while (at < n) {
                uint64_t cnt = 1 + rng() % (4 * (uint64_t)lds_cap);
                if (rep % 7 == 0) cnt = lds_cap + 1 + rng() % 3;           // as many segments as can be
                if (cnt > n - at) cnt = n - at;
                if (cnt > lds_cap) {
                    const int vals = 1 << (1 + rng() % 8);
                    std::vector<uint64_t> counts(vals, 0);
                    const int shape = (int)(rng() % 5);
                    for (uint64_t i = 0; i < cnt; ++i) {
                        uint64_t v = rng() % vals;
                        if (shape == 1) v = rng() % 3 ? 0 : v;             // one heavy value
                        if (shape == 2) v = v & ~(rng() % 4);             // few values
                        if (shape == 3) v = 0;                             // one bin (the kernel passes such a segment on whole)
                        counts[v % vals]++;
                    }
                    if (shape == 4) {                                      // alternating 1 and local_tile: the worst case of the packing
                        std::fill(counts.begin(), counts.end(), 0);
                        uint64_t left = cnt;
                        for (int v = 0; v < vals && left; ++v) { const uint64_t c = std::min<uint64_t>(left, v & 1 ? local_tile : 1); counts[v] = c; left -= c; }
                        counts[vals - 1] += left;
                    }
                    if (check_segment(counts, at, local_tile, lds_cap, n_cls)) return 1;
                }
                at += cnt;
            }
            if (n_cls[kSplitSmall] > caps.n_small) return fail("small list capacity", n_cls[kSplitSmall], caps.n_small);
            if (n_cls[kSplitMid] > caps.n_mid) return fail("mid list capacity", n_cls[kSplitMid], caps.n_mid);
            if (n_cls[kSplitNext] > caps.n_next) return fail("next list capacity", n_cls[kSplitNext], caps.n_next);
        }
    }
    // the sizes of the flagship workload: no overflow of the 64-bit arithmetic, lists far below the key buffers
    const SplitCaps big = split_list_caps(7200000000ull, 4096, 8192);
    if (big.bytes() > 7200000000ull * 12 / 256) return fail("lists above 1/256 of a key buffer", big.bytes(), 0);
    std::puts("ok");
    return 0;
}
