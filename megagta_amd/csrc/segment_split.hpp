// segment_split.hpp — host-checkable arithmetic of the oversized-segment route of the SdBG build's sort (sdbg_build.hip, 4b):
// how the pieces of one split level are packed into finish ranges, and how many list entries a level can produce at most.
// Plain C++ (no HIP headers): the device kernel and a stand-alone host check share it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MGTA_SPLIT_HD __host__ __device__ __forceinline__
#else
#define MGTA_SPLIT_HD inline
#endif

namespace mgta {

// where a piece (the keys of one digit value of a split segment) or a packed range of pieces goes
enum SplitClass : uint32_t {
    kSplitSmall = 0,   // a range of whole pieces, <= local_tile keys in all: LSD passes in the LDS of a shared CU (local_lsd_kernel)
    kSplitMid = 1,     // one piece of local_tile < keys <= lds_cap: the LDS of a whole CU (segment_lds_kernel)
    kSplitNext = 2,    // one piece of more than lds_cap keys: split again on the next digit down
    kSplitClasses = 3
};

// Greedy packing of the pieces of ONE split segment, in digit order.  Feed the count of every digit value in ascending order to
// step(), then call finish(); emit(cls, first, end) is called once per range, with positions counted from `first` of the constructor.
// Two small ranges that follow each other with no larger piece in between hold more than local_tile keys together (the second one
// was opened because its first piece did not fit the first any more), and every mid / next piece holds more than local_tile keys
// itself: a segment of cnt keys yields at most 2 cnt / local_tile + 1 small ranges.
struct SplitPacker {
    uint64_t pos, run_first;
    uint32_t run_len, local_tile, lds_cap;
    MGTA_SPLIT_HD SplitPacker(uint64_t first, uint32_t local_tile_, uint32_t lds_cap_)
        : pos(first), run_first(first), run_len(0), local_tile(local_tile_), lds_cap(lds_cap_) {}
    template <class Emit>
    MGTA_SPLIT_HD void flush(Emit &emit) {
        if (run_len) emit(kSplitSmall, run_first, run_first + run_len);
        run_len = 0;
    }
    template <class Emit>
    MGTA_SPLIT_HD void step(uint64_t c, Emit &emit) {
        if (c == 0) return;
        if (c > (uint64_t)local_tile) {
            flush(emit);
            emit(c > (uint64_t)lds_cap ? kSplitNext : kSplitMid, pos, pos + c);
        } else if ((uint64_t)run_len + c > (uint64_t)local_tile) {
            flush(emit);
            run_first = pos;
            run_len = (uint32_t)c;
        } else {
            if (run_len == 0) run_first = pos;
            run_len += (uint32_t)c;
        }
        pos += c;
    }
    template <class Emit>
    MGTA_SPLIT_HD void finish(Emit &emit) { flush(emit); }
};

// Entries ONE level can append to each list when the array holds n keys.  The segments a level splits are disjoint and longer than
// lds_cap each, so there are fewer than n / lds_cap of them; with the packer's bound they yield at most 2 n / local_tile + n / lds_cap
// small ranges.  Mid pieces are disjoint and longer than local_tile, next pieces (and segments passed on unsplit) disjoint and longer
// than lds_cap.  (+ 1: the divisions round down.)
struct SplitCaps {
    uint64_t n_small, n_mid, n_next;
    // bytes of the lists of a sort: small, mid and two next lists (a level reads one and fills the other), two 64-bit words per
    // entry, and a line of counters
    uint64_t bytes() const { return (n_small + n_mid + 2 * n_next) * 16 + 64; }
};
inline SplitCaps split_list_caps(uint64_t n, uint32_t local_tile, uint32_t lds_cap) {
    SplitCaps c;
    c.n_next = n / lds_cap + 1;
    c.n_small = 2 * (n / local_tile + 1) + c.n_next;
    c.n_mid = lds_cap > local_tile ? n / local_tile + 1 : 0;
    return c;
}

}  // namespace mgta
