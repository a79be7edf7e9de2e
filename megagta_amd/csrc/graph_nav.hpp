// graph_nav.hpp -- navigation over the device graph that the A* path does not need (succinct_dbg.cpp:99-371,503-593): the last edge of a
// node, the edges into and out of a node, the simple-path steps, Label and the reverse complement of an edge.  denovo.hip walks the graph
// with them, graph.hip answers mgta_sdbg_navigate with them; every function has internal linkage, so each of the two compiles its own copy.
#pragma once
#include "graph.hpp"

namespace mgta {
namespace {

constexpr int kMaxK = 255;

// ---- navigation the A* path does not need (succinct_dbg.cpp:99-371) -----------------------------------------------------------
__device__ inline int64_t d_last_index(const GraphDev &g, int64_t x) {   // GetLastIndex = rs_last_.Succ, succinct_dbg.h:105
    uint64_t li = (uint64_t)x >> 6;
    uint64_t m = g.lines[li].last >> (x & 63);
    if (m) return x + __ffsll((long long)m) - 1;
    while (++li < g.n_lines) {
        uint64_t w = g.lines[li].last;
        if (w) return (int64_t)(li << 6) + __ffsll((long long)w) - 1;
    }
    return g.size;
}

// edges that point to the node of x (IncomingEdges / UniquePrev* / NodeIndegreeZero / DeleteAllEdges share this scan)
template <bool ALL>
__device__ inline int d_incoming_scan(const GraphDev &g, int64_t x, int64_t *in) {
    int64_t first = g_backward(g, x);
    const int c = g_W(g, first);
    int ones = g_last_or_tip(g, first), n = 0;
    if (ALL || g_valid(g, first)) in[n++] = first;
    for (int64_t y = first + 1; ones < 5 && y < g.size; ++y) {
        ones += g_last_or_tip(g, y);
        const int cur = g_W(g, y);
        if (cur == c) break;
        if (cur == c + 4 && (ALL || g_valid(g, y)) && n < 8) in[n++] = y;
    }
    return n;
}
template <bool ALL>
__device__ inline int d_node_edges(const GraphDev &g, int64_t node, int64_t *out) {   // the node's own edges, from its last one downwards
    int64_t e = d_last_index(g, node);
    int n = 0;
    do {
        if ((ALL || g_valid(g, e)) && n < 8) out[n++] = e;
        --e;
    } while (e >= 0 && !g_last_or_tip(g, e));
    return n;
}
__device__ inline int d_outgoing(const GraphDev &g, int64_t e, int64_t *out) {   // OutgoingEdges, valid edge ids in descending order
    if (!g_valid(g, e)) return -1;
    int n = 0;
    int64_t x = g_forward(g, e);
    do {
        if (g_valid(g, x) && n < 8) out[n++] = x;
        --x;
    } while (x >= 0 && !g_last_or_tip(g, x));
    return n;
}
__device__ inline int d_incoming(const GraphDev &g, int64_t e, int64_t *in) {
    if (!g_valid(g, e)) return -1;
    return d_incoming_scan<false>(g, e, in);
}
__device__ inline bool node_outdegree_zero(const GraphDev &g, int64_t node) { int64_t t[8]; return d_node_edges<false>(g, node, t) == 0; }
__device__ inline bool node_indegree_zero(const GraphDev &g, int64_t node) { int64_t t[8]; return d_incoming_scan<false>(g, node, t) == 0; }
__device__ inline int64_t unique_prev_node(const GraphDev &g, int64_t node) {
    int64_t t[8];
    return d_incoming_scan<false>(g, node, t) == 1 ? d_last_index(g, t[0]) : -1;
}
__device__ inline int64_t unique_next_node(const GraphDev &g, int64_t node) {
    int64_t t[8];
    return d_node_edges<false>(g, node, t) == 1 ? d_last_index(g, g_forward(g, t[0])) : -1;
}
__device__ inline int64_t unique_next_edge(const GraphDev &g, int64_t e) {
    int64_t t[8];
    return d_outgoing(g, e, t) == 1 ? t[0] : -1;
}
__device__ inline int64_t unique_prev_edge(const GraphDev &g, int64_t e) {
    int64_t t[8];
    return d_incoming(g, e, t) == 1 ? t[0] : -1;
}
__device__ inline int64_t prev_simple(const GraphDev &g, int64_t e) {   // PrevSimplePathEdge
    int64_t p = unique_prev_edge(g, e);
    return p != -1 && unique_next_edge(g, p) != -1 ? p : -1;
}
__device__ inline int64_t next_simple(const GraphDev &g, int64_t e) {   // NextSimplePathEdge
    int64_t n = unique_next_edge(g, e);
    return n != -1 && unique_prev_edge(g, n) != -1 ? n : -1;
}

__device__ inline void d_label(const GraphDev &g, int64_t e, uint8_t *seq) {   // Label, succinct_dbg.cpp:503-528 (symbols 1..4)
    int64_t x = e;
    for (int i = g.k - 1; i >= 0; --i) {
        if (g_tip(g, x)) {
            int64_t tr = g_rank_tip(g, x) - 1;
            for (int j = 0; j <= i; ++j) seq[i - j] = (uint8_t)(g_tip_char(g, tr, j) + 1);
            break;
        }
        x = g_backward(g, x);
        int c = g_W(g, x);
        seq[i] = (uint8_t)(c > 4 ? c - 4 : c);
    }
}
__device__ inline int64_t edge_reverse_complement(const GraphDev &g, int64_t e) {   // succinct_dbg.cpp:551-593
    if (!g_valid(g, e)) return -1;
    uint8_t seq[kMaxK + 2];
    d_label(g, e, seq);
    int w = g_W(g, e);
    seq[g.k] = (uint8_t)(w > 4 ? w - 4 : w);
    for (int i = 0, j = g.k; i <= j; ++i, --j) {
        uint8_t a = (uint8_t)(5 - seq[i]), b = (uint8_t)(5 - seq[j]);
        seq[i] = b; seq[j] = a;
    }
    return g_index_edge(g, seq);
}

}  // namespace
}  // namespace mgta
