"""The navigation of the succinct de Bruijn graph restated in numpy, from the bit vectors alone (no code shared with the device or the oracle).

rank = cumsum, select = nonzero, everything else written out from its definition (succinct_dbg.h:155-170, succinct_dbg.cpp:78-127,
503-593).  tests/test_graph_nav_host.py pins this restatement to the oracle's C calls and to the reference's own probe files;
tests/test_graph_nav_gpu.py compares mgta_sdbg_navigate with it.  Also here: the seeded inputs both files use, and the count of the hard
paths (a)-(g) of the forward-descriptor chain that an input takes.
"""
from __future__ import annotations

import numpy as np

UNTOUCHED, UNDEFINED = -2, -3          # MGTA_NAV_UNTOUCHED, MGTA_NAV_UNDEFINED (include/megagta_hip.h)


def _bits(words: np.ndarray, n: int) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little")[:n].astype(bool)


class NavRef:
    def __init__(self, k, f, W, last, tip, invalid, multi1, tip_labels, words_per_tip):
        self.k, self.size = int(k), int(W.size)
        self.f = [int(x) for x in f]
        self.W = W.astype(np.int64)
        self.lab = np.where(self.W > 4, self.W - 4, self.W)                 # the out-label of an edge, 0 for $
        self.last, self.tip, self.invalid, self.multi1 = last, tip, invalid, multi1
        self.tip_labels, self.wpt = np.asarray(tip_labels, dtype=np.uint32), int(words_per_tip)
        self.n_lines = (self.size + 63) // 64
        self.cum_last = np.concatenate([[0], np.cumsum(last)]).astype(np.int64)          # cum[p + 1] = ones in [0..p]
        self.cum_tip = np.concatenate([[0], np.cumsum(tip)]).astype(np.int64)
        self.pos_last = np.nonzero(last)[0].astype(np.int64)
        self.total_last = int(self.pos_last.size)
        self.cum_w, self.pos_w, self.total_w = {}, {}, {}
        for c in range(1, 5):
            m = self.W == c                                                  # plain symbols only: c + 4 is not counted
            self.cum_w[c] = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
            self.pos_w[c] = np.nonzero(m)[0].astype(np.int64)
            self.total_w[c] = int(self.pos_w[c].size)
        self.pos_stop = np.nonzero(last | tip)[0].astype(np.int64)           # a node's edges end below the next lower last | tip bit
        self.rank_f = [int(self.cum_last[max(x, 0)]) for x in self.f]        # Rank(f[i] - 1)
        self._l = None
        self._by_kmer = None

    # ---- construction ---------------------------------------------------------------------------------------------------------
    @classmethod
    def from_oracle(cls, og):
        bv, n = og.bitvectors(), og.size
        by = np.ascontiguousarray(bv["w"], dtype="<u8").view(np.uint8)
        W = np.empty(by.size * 2, np.uint8)
        W[0::2], W[1::2] = by & 15, by >> 4
        wpt = bv["tip_labels"].size // og.num_tips if og.num_tips else (2 * og.k + 31) // 32
        return cls(og.k, og.f, W[:n], _bits(bv["last"], n), _bits(bv["tip"], n), _bits(bv["invalid"], n), _bits(bv["multi1"], n),
                   bv["tip_labels"], wpt)

    @classmethod
    def from_records(cls, k, records, bucket_items, tips=(), words_per_tip=None):
        """from the stream's 16-bit records: W = bits 0-3, last = bit 4, tip = bit 5, stored multiplicity = bits 8-15"""
        rec = np.asarray(records, dtype=np.uint16).astype(np.int64)
        W, tip = (rec & 15).astype(np.uint8), ((rec >> 5) & 1).astype(bool)
        f = [-1, 0] + [int(x) for x in np.cumsum(np.asarray(bucket_items, dtype=np.int64).reshape(4, -1).sum(axis=1))]
        return cls(k, f, W, ((rec >> 4) & 1).astype(bool), tip, tip | (W == 0), (rec >> 8) <= 1, tips,
                   (2 * k + 31) // 32 if words_per_tip is None else words_per_tip)

    # ---- rank / select (rank_and_select.h:153,560: ones in [0..pos]; the r-th one, 0-based) --------------------------------------
    def rank_last(self, pos): return self.cum_last[np.asarray(pos, np.int64) + 1]
    def rank_tip(self, pos): return self.cum_tip[np.asarray(pos, np.int64) + 1]

    def rank_w(self, c, pos):
        pos, c = np.asarray(pos, np.int64), np.broadcast_to(np.asarray(c, np.int64), np.shape(pos))
        out = np.zeros(pos.shape, np.int64)
        for a in range(1, 5):
            out = np.where(c == a, self.cum_w[a][pos + 1], out)
        return out

    @staticmethod
    def _select(positions, size, r):
        r = np.asarray(r, np.int64)
        if positions.size == 0:
            return np.where(r < 0, -1, size).astype(np.int64)
        return np.where(r < 0, -1, np.where(r >= positions.size, size, positions[np.clip(r, 0, positions.size - 1)])).astype(np.int64)

    def select_last(self, r): return self._select(self.pos_last, self.size, r)

    def select_w(self, c, r):
        r, c = np.asarray(r, np.int64), np.broadcast_to(np.asarray(c, np.int64), np.shape(r))
        out = np.zeros(r.shape, np.int64)
        for a in range(1, 5):
            out = np.where(c == a, self._select(self.pos_w[a], self.size, r), out)
        return out

    # ---- Forward / Backward ------------------------------------------------------------------------------------------------
    def fd_r(self, e):
        """the Select argument of Forward(e): rank_f[a] + Rank(a, e) - 1, a = the out-label (plain occurrences only are counted)"""
        e = np.asarray(e, np.int64)
        a = self.lab[e]
        return np.asarray(self.rank_f, np.int64)[np.clip(a, 0, 4)] + self.rank_w(np.clip(a, 1, 4), e) - 1

    def forward(self, e):
        e = np.asarray(e, np.int64)
        return np.where(self.lab[e] == 0, UNDEFINED, self.select_last(self.fd_r(e)))

    def node_last_char(self, x):
        x = np.asarray(x, np.int64)
        return sum((self.f[i] <= x).astype(np.int64) for i in range(1, 5))     # the i with f[i] <= x < f[i + 1]

    def backward(self, e):
        e = np.asarray(e, np.int64)
        a = self.node_last_char(e)
        cnt = self.rank_last(e - 1) - np.asarray(self.rank_f, np.int64)[a]
        return np.where(self.tip[e] | (a == 0), UNDEFINED, self.select_w(np.clip(a, 1, 4), cnt))

    def last_index(self, e):
        """the first position >= e with a `last` bit, size when there is none"""
        i = np.searchsorted(self.pos_last, np.asarray(e, np.int64), "left")
        return np.concatenate([self.pos_last, [self.size]])[i]

    # ---- OutgoingEdges: the valid edges of the node Forward(e) points to, from its last edge down to above the next lower last | tip bit
    def node_low(self, x):
        """the nearest last | tip position strictly below x, -1 when there is none"""
        i = np.searchsorted(self.pos_stop, np.asarray(x, np.int64), "left")
        return np.where(i > 0, self.pos_stop[np.clip(i - 1, 0, None)], -1)

    def outgoing(self, e, packed=True):
        """-> int64[n, 5]: degree (-1 = e is not valid), then id << 4 | multi1 << 3 | label (or plain ids), -1 in unused slots"""
        e = np.asarray(e, np.int64)
        out = np.full((e.size, 5), -1, np.int64)
        ok = ~self.invalid[e]
        x = np.where(ok, self.forward(e), 0)
        inside = ok & (x >= 0) & (x < self.size)
        assert inside[ok].all(), "Forward of a valid edge leaves the graph: not a stream a build produces"
        y = self.node_low(x)
        assert int((x - y)[inside].max(initial=0)) <= 9
        deg = np.zeros(e.size, np.int64)
        for j in range(9):
            c = x - j
            take = inside & (c > y)
            take &= ~self.invalid[np.clip(c, 0, self.size - 1)]
            cc = np.clip(c, 0, self.size - 1)
            val = (cc << 4) | (self.multi1[cc].astype(np.int64) << 3) | self.lab[cc] if packed else cc
            put = take & (deg < 4)
            out[np.nonzero(put)[0], 1 + deg[put]] = val[put]
            deg += take
        out[:, 0] = np.where(ok, np.minimum(deg, 4), -1)
        return out

    # ---- the forward descriptor of an edge and one step of the chain (graph.hpp: g_fd_of, g_outset_from, g_outset_get_fd) ----------
    def hint(self, e):
        """fwd_hint[a - 1] of e's line as graph_hint_kernel defines it: the line of the `last` bit that Forward of the last plain a
        BEFORE e's line selects (rank clamped to 0), the last line when that rank is past the end"""
        e = np.asarray(e, np.int64)
        a = np.clip(self.lab[e], 1, 4)
        r0 = np.asarray(self.rank_f, np.int64)[a] + self.rank_w(a, (e >> 6 << 6) - 1) - 1
        return np.where(r0 >= self.total_last, self.n_lines - 1, self.select_last(np.maximum(r0, 0)) >> 6)

    def out_fd(self, e, r=None, hint=None):
        """-> int64[n, 29] as MGTA_NAV_OUT_FD lays it out; r / hint None = "none" (the descriptor is read from e's own line)"""
        e = np.asarray(e, np.int64)
        n = e.size
        out = np.full((n, 29), UNTOUCHED, np.int64)
        if r is None:
            ok = ~self.invalid[e]
            r = np.where(ok, self.fd_r(e), -1)
        else:
            ok, r = np.ones(n, bool), np.asarray(r, np.int64)
        has = ok & (r >= 0) & (r < self.total_last)
        x = np.where(has, self.select_last(r), 0)
        y = self.node_low(x)
        deg = np.zeros(n, np.int64)
        for j in range(9):
            c = x - j
            cc = np.clip(c, 0, self.size - 1)
            take = has & (c > y) & ~self.invalid[cc]
            put = take & (deg < 4)
            rows, slot = np.nonzero(put)[0], deg[put]
            same_line = (cc >> 6) == (x >> 6)
            val = (cc << 4) | (self.multi1[cc].astype(np.int64) << 3) | self.lab[cc]
            fr, fh = np.where(same_line, self.fd_r(cc), 0), np.where(same_line, self.hint(cc), -1)
            for base, v in ((1, val), (5, fr), (9, fh), (17, val), (21, fr), (25, fh)):
                out[rows, base + slot] = v[put]
            deg += take
        deg = np.where(ok, np.minimum(deg, 4), -1)
        out[:, 0] = deg
        out[:, 13:17] = deg[:, None]
        return out

    # ---- IncomingEdges and the simple-path steps (succinct_dbg.cpp:99-127,173-225) -- one edge at a time, over plain lists ------------
    def _lists(self):
        if self._l is None:
            every = np.arange(self.size, dtype=np.int64)
            out = self.outgoing(every, packed=False)
            self._l = dict(W=self.W.tolist(), stop=(self.last | self.tip).tolist(), invalid=self.invalid.tolist(),
                           back=self.backward(every).tolist(), od=out[:, 0].tolist(), o0=out[:, 1].tolist())
        return self._l

    def incoming1(self, e: int):
        """the edges into the node of e: Backward(e) -- the one plain occurrence of the node's last character that points to it -- and the
        c + 4 edges that follow it before the next plain c (at most four more nodes on), the valid ones of them"""
        l = self._lists()
        W, stop, invalid = l["W"], l["stop"], l["invalid"]
        if invalid[e]:
            return -1, []
        first = l["back"][e]
        assert 0 <= first < self.size
        c, ones, res = W[first], int(stop[first]), []
        if not invalid[first]:
            res.append(first)
        y = first + 1
        while ones < 5 and y < self.size:
            ones += stop[y]
            if W[y] == c:
                break
            if W[y] == c + 4 and not invalid[y]:
                res.append(y)
            y += 1
        return len(res), res

    def incoming(self, e):
        e = np.asarray(e, np.int64)
        out = np.full((e.size, 5), -1, np.int64)
        for i, x in enumerate(e.tolist()):
            d, ids = self.incoming1(x)
            out[i, 0] = d
            out[i, 1:1 + len(ids[:4])] = ids[:4]
        return out

    def _unique_next(self, e: int) -> int:
        l = self._lists()
        return l["o0"][e] if l["od"][e] == 1 else -1

    def _unique_prev(self, e: int) -> int:
        d, ids = self.incoming1(e)
        return ids[0] if d == 1 else -1

    def prev_simple(self, e):
        """the one edge into e's node, if that edge in turn has e as its one way out"""
        res = []
        for x in np.asarray(e, np.int64).tolist():
            p = self._unique_prev(x)
            res.append(p if p != -1 and self._unique_next(p) != -1 else -1)
        return np.array(res, np.int64)

    def next_simple(self, e):
        res = []
        for x in np.asarray(e, np.int64).tolist():
            nx = self._unique_next(x)
            res.append(nx if nx != -1 and self._unique_prev(nx) != -1 else -1)
        return np.array(res, np.int64)

    # ---- Label (succinct_dbg.cpp:503-528) and EdgeReverseComplement (:551-593) ------------------------------------------------------
    def tip_char(self, tip_rank, j):
        t = self.tip_labels[tip_rank * self.wpt + (j >> 4)].astype(np.int64)
        return (t >> ((15 - (j & 15)) * 2)) & 3

    def label(self, e):
        """-> uint8[n, k], symbols 1..4: walk Backward reading W until a tip, whose stored label gives the rest"""
        x = np.asarray(e, np.int64).copy()
        seq = np.zeros((x.size, self.k), np.uint8)
        active = np.ones(x.size, bool)
        for i in range(self.k - 1, -1, -1):
            at_tip = active & self.tip[x]
            if at_tip.any():
                rows = np.nonzero(at_tip)[0]
                tr = self.rank_tip(x[rows]) - 1
                for j in range(i + 1):
                    seq[rows, i - j] = self.tip_char(tr, j) + 1
                active &= ~at_tip
            if not active.any():
                break
            rows = np.nonzero(active)[0]
            b = self.backward(x[rows])
            assert ((b >= 0) & (b < self.size)).all()
            x[rows] = b
            seq[rows, i] = self.lab[b]
        return seq

    def reverse_complement(self, e):
        """the edge whose (k+1)-mer is the reverse complement of e's, -1 when the graph has none (or e is not valid).  IndexBinarySearchEdge
        finds a (k+1)-mer at an edge of a node that is no tip, whatever its validity bit says."""
        if self._by_kmer is None:
            every = np.nonzero(~self.tip & (self.lab > 0))[0]
            km = np.concatenate([self.label(every), self.lab[every, None].astype(np.uint8)], axis=1)
            self._by_kmer = {}
            for x, row in zip(every.tolist(), km):
                assert self._by_kmer.setdefault(row.tobytes(), x) == x, "two edges with one (k+1)-mer"
        e = np.asarray(e, np.int64)
        km = np.concatenate([self.label(e), self.lab[e, None].astype(np.uint8)], axis=1)
        rc = (5 - km[:, ::-1]).astype(np.uint8)
        return np.array([-1 if self.invalid[x] else self._by_kmer.get(row.tobytes(), -1) for x, row in zip(e.tolist(), rc)], np.int64)

    # ---- which hard paths of the descriptor chain the edges of this graph take ----------------------------------------------------
    def paths(self) -> dict:
        """over every valid edge e: (a) the node Forward(e) points to begins and ends in the target line; (b) it continues into the
        line before (valid edges there); (c) bit 63 of the line before is a last | tip bit (the node begins at bit 0 of the target line);
        (d) / (e) the hint of e is one / two or more lines before the target line; (f) e carries a + 4 and no plain a precedes it in
        its line; (g) the most lines Select walks from its sample (the line of the 64 * (r >> 6)-th one), for `last` and per symbol"""
        e = np.nonzero(~self.invalid)[0].astype(np.int64)
        x = self.forward(e)
        li, y = x >> 6, self.node_low(x)
        in_line = (y >= (li << 6)) | (li == 0)
        prev63 = (li << 6) - 1
        c = ~in_line & (y == prev63)
        lo_valid = np.zeros(e.size, bool)
        for j in range(1, 9):                                                 # a valid edge of the node in the line before
            p = np.clip(prev63 - j + 1, 0, self.size - 1)
            lo_valid |= ~in_line & (prev63 - j + 1 > y) & ~self.invalid[p]
        early = li - self.hint(e)
        assert (early >= 0).all(), "a hint behind its target: the look-up only walks forwards"
        a = self.lab[e]
        before = self.rank_w(a, e - 1) - self.rank_w(a, (e >> 6 << 6) - 1)     # plain a in e's line before e
        walk = {}
        for name, pos in [("last", self.pos_last)] + [(f"w{s}", self.pos_w[s]) for s in range(1, 5)]:
            r = np.arange(pos.size)
            walk[name] = int(((pos >> 6) - (pos[r >> 6 << 6] >> 6)).max(initial=0))
        return dict(edges=int(e.size), a=int(in_line.sum()), b=int(lo_valid.sum()), c=int(c.sum()), d=int((early == 1).sum()),
                    e=int((early >= 2).sum()), f=int(((self.W[e] > 4) & (before == 0)).sum()), g=walk)


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------
def _revcomp(r):
    return (3 - r[::-1]).astype(np.uint8)


def reads_random(seed, k, genome_len, n_reads, max_len=300):
    """reads of a random genome, both strands, a few with one wrong base (as test_fuzz_navigation_vs_oracle draws them)"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, genome_len).astype(np.uint8)
    reads = []
    for _ in range(n_reads):
        L = int(rng.integers(k + 1, max(k + 2, min(genome.size, max_len))))
        p = int(rng.integers(0, genome.size - L + 1))
        r = genome[p:p + L].copy()
        if rng.random() < 0.15:
            r[int(rng.integers(0, L))] = int(rng.integers(0, 4))
        reads.append(_revcomp(r) if rng.random() < 0.5 else r)
    return reads


def reads_low_complexity(seed=11, k=21, genome_len=6000, n_reads=150):
    """a genome of A and C with a rare G or T (one base in 150), read mostly from one strand: within the block of nodes that end in one
    letter a symbol is then absent over dozens of lines, so Select walks far from its sample; plus poly-A reads (one node that is its
    own successor) and deep overlap (runs of multi1 = 0)"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 2, genome_len).astype(np.uint8)                  # A / C
    rare = rng.choice(genome_len, genome_len // 150, replace=False)
    genome[rare] = rng.integers(2, 4, rare.size)                              # a rare G / T
    reads = []
    for _ in range(n_reads):
        L = int(rng.integers(k + 1, 200))
        p = int(rng.integers(0, genome_len - L + 1))
        r = genome[p:p + L].copy()
        reads.append(r if rng.random() < 0.8 else _revcomp(r))               # mostly one strand: A / C rich
    reads += [np.zeros(int(rng.integers(k + 5, 120)), np.uint8) for _ in range(12)]
    return reads


def reads_tip_heavy(seed=12, k=21, genome_len=3000, n_reads=150):
    """reads of a genome plus many reads that follow it up to a branch point and end a few bases after a wrong base"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, genome_len).astype(np.uint8)
    reads = []
    for _ in range(n_reads):
        L = int(rng.integers(k + 20, 200))
        p = int(rng.integers(0, genome_len - L + 1))
        reads.append(genome[p:p + L].copy())
    for _ in range(n_reads * 2):
        p = int(rng.integers(0, genome_len - k - 10))
        r = genome[p:p + k + int(rng.integers(2, 8))].copy()
        r[k] = (r[k] + int(rng.integers(1, 4))) & 3                            # the branch: the base after the first k-mer
        reads.append(r)
    return reads


def reads_dense(seed=13, k=9, n_reads=2500):
    """random reads at k = 9: 4^10 possible edges, most of them present, so in- and out-degree 4 nearly everywhere"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, 400).astype(np.uint8) for _ in range(n_reads)]


def synthetic_records(seed=21, n_lines=300, tail=37):
    """records that are no graph at all, for rank / select alone: random W (0..8) / last / tip over ~300 lines, with lines that hold no
    `last` bit, lines of all ones, and symbol 4 present only in the first and in the last line"""
    rng = np.random.default_rng(seed)
    n = n_lines * 64 + tail
    W = rng.integers(0, 9, n)
    W[W == 4] = 8
    W[[3, 17, 60]] = 4
    W[[n - 1, n - 5]] = 4
    W[64 * 40:64 * 90] = rng.integers(5, 9, 64 * 50)                          # fifty lines without any plain symbol
    last = rng.random(n) < 0.6
    tip = rng.random(n) < 0.1
    for li in (0, 5, 6, 7, 100, n_lines - 1):
        last[li * 64:(li + 1) * 64] = False                                   # no `last` bit in the line
    for li in (1, 8, 101, 150):
        last[li * 64:(li + 1) * 64] = True                                    # all ones
        tip[li * 64:(li + 1) * 64] = True
    last[64 * 200:64 * 230] = False                                           # thirty lines in a row without one
    mult = rng.integers(0, 4, n)
    rec = (W | (last.astype(np.int64) << 4) | (tip.astype(np.int64) << 5) | (mult << 8)).astype(np.uint16)
    bucket_items = np.zeros(65536, np.int64)
    bucket_items[[0, 20000, 40000, 60000]] = [n // 4, n // 4, n // 4, n - 3 * (n // 4)]
    return rec, bucket_items


def reads_fan(k=9):
    """path (e) by construction: 64 nodes A t S (t = every 3-mer, S a fixed 5-mer) that are neighbours in the graph's order (they share the
    suffix S) have one out-edge each, a plain A, so they fill one 64-edge line with 64 plain A; the 64 nodes t S A these point to carry
    four out-edges each and so spread over four lines: the hint of that line (the target of the plain A before it) lies up to four
    lines before the targets of its later edges"""
    import itertools
    S = [1, 2, 3, 1, 0]
    assert k == 9
    return [np.array([0, *t, *S, 0, c], np.uint8) for t in itertools.product(range(4), repeat=3) for c in range(4)]


def reads_small(seed, k, palindrome):
    """short reads along a random genome, to grow a small graph read by read; a palindromic (k+1)-mer first (k odd) makes the number of
    edges odd, a palindromic k-mer (k even) the number of nodes: every other one comes with its reverse complement"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, 600).astype(np.uint8)
    reads = []
    if palindrome:
        half = rng.integers(0, 4, (k + 1) // 2).astype(np.uint8)           # k odd: a palindromic edge; k even: a palindromic node
        reads.append(np.concatenate([half, _revcomp(half), rng.integers(0, 4, 1 - k % 2).astype(np.uint8)]))
    p = 0
    while p + k + 3 < genome.size:
        reads.append(genome[p:p + k + 1 + int(rng.integers(0, 3))].copy())
        p += int(rng.integers(1, 3)) if rng.random() < 0.9 else k + 2
    return reads


def _totals(og):
    last = og.rank_last(og.size - 1)
    return last, [og.rank_w(c, og.size - 1) for c in range(1, 5)]


# name -> (group, k, how to get the reads or the graph).  Group a: the goldens; b: line and sample edges; c: low complexity, tips, dense.
SMALL = {
    "one_line": (9, True, lambda og: 20 < og.size < 64),
    "size_65": (9, True, lambda og: og.size == 65),
    "size_127": (21, True, lambda og: og.size == 127),
    "size_128": (44, False, lambda og: og.size == 128),
    "size_129": (95, True, lambda og: og.size == 129),
    "size_191": (9, True, lambda og: og.size == 191),
    "size_192": (64, False, lambda og: og.size == 192),
    "last_64": (21, False, lambda og: _totals(og)[0] == 64),
    "last_65": (32, True, lambda og: _totals(og)[0] == 65),
    "w_64": (79, False, lambda og: 64 in _totals(og)[1] and 65 not in _totals(og)[1]),
    "w_65": (32, False, lambda og: 65 in _totals(og)[1]),
}
GOLDEN = {"ragged29": ("ragged", 29), "ragged47": ("ragged", 47), "toy44": ("toy", 44)}
SEEDED = {"rand32": (32, lambda: reads_random(31, 32, 3000, 300)), "lowcomplex": (21, reads_low_complexity), "tips": (21, reads_tip_heavy), "dense": (9, reads_dense), "fan": (9, reads_fan)}
GROUPS = {"a": list(GOLDEN), "b": list(SMALL) + ["rand32"], "c": ["lowcomplex", "tips", "dense", "fan"]}
_CACHE = {}


def get_input(name, oracle, golden_dir):
    """-> dict(name, k, packed, start, stream (oracle.Stream), og (oracle.Graph), ref (NavRef)); built once per process"""
    import os
    from megagta_amd import readlib
    if name in _CACHE:
        return _CACHE[name]
    if name in GOLDEN:
        case, k = GOLDEN[name]
        packed, start = readlib.load_for_build(os.path.join(golden_dir, case, "reads.lib"))
        stream = oracle.Stream.build(packed, start, k, threads=4)
        og = oracle.Graph(stream)
    elif name in SEEDED:
        k, fn = SEEDED[name]
        packed, start = readlib.pack_for_build(fn())
        stream = oracle.Stream.build(packed, start, k, threads=4)
        og = oracle.Graph(stream)
    else:
        k, pal, accept = SMALL[name]
        for seed in range(100, 140):
            reads = reads_small(seed, k, pal)
            lo, hit = 1, None
            for m in range(1, len(reads) + 1):
                packed, start = readlib.pack_for_build(reads[:m])
                stream = oracle.Stream.build(packed, start, k, threads=1)
                og = oracle.Graph(stream)
                if accept(og):
                    hit = m
                    break
                if og.size > 600:
                    break
            if hit:
                break
        else:
            raise AssertionError(f"{name}: no seed gives the graph asked for")
    _CACHE[name] = dict(name=name, k=k, packed=packed, start=start, stream=stream, og=og, ref=NavRef.from_oracle(og))
    return _CACHE[name]
