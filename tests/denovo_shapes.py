"""Designed read sets for `denovo`: graphs that sit on the limits of Trim, BranchGroup::Search / Pop and the device's reach walk.

Every shape is a handful of explicit haplotype strings, error free, tiled into reads at every offset (min_count 1), so the graph and the
coverage of every edge are what the generator says.  make(name) -> (reads: list[str], info: dict); info["k"], info["runs"] (the
(max_tip_len, no_bubble, min_contig) settings the shape is run with) and what the shape is meant to show.  tests/test_denovo_limits.py
states the expectations; tests/golden/make_golden_denovo_limits.py records the reference binary's one-thread output for GOLDEN_SHAPES.

Also here, over tests/graph_nav_ref.py's NavRef (numpy, no code shared with the device or the oracle): BranchGroup::Search restated
(search), the edges a reach walk counts (region), and the ordered rounds of the device's PopBubbles as its head comment states them
(model_rounds)."""
from __future__ import annotations

import itertools
import zlib

import numpy as np

CODE = {c: i for i, c in enumerate("ACGT")}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
MAX_BRANCHES, REACH_MAX, REACH_FRONTIER, NARROW_MAX = 16, 16384, 2048, 512     # the limits as shipped (denovo.hip)


def revcomp(s: str) -> str:
    return "".join(COMP[c] for c in reversed(s))


def as_arrays(reads):
    return [np.array([CODE[c] for c in r], dtype=np.uint8) for r in reads]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _rand(rng, n: int) -> str:
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _other(rng, *avoid) -> str:
    return str(rng.choice([c for c in "ACGT" if c not in avoid]))


def tile(hap: str, read_len: int, copies: int = 1):
    """every substring of read_len, at every offset: an inner (k+1)-mer is covered (read_len - k) * copies times"""
    if len(hap) <= read_len:
        return [hap] * copies
    return [hap[p:p + read_len] for p in range(len(hap) - read_len + 1)] * copies


def check_unique_kmers(haps, k):
    """no k-mer twice within a haplotype, and none shared between the two strands: the graph is the drawing, nothing else"""
    fwd = set()
    for h in haps:
        own = [h[p:p + k] for p in range(len(h) - k + 1)]
        assert len(set(own)) == len(own), "a k-mer repeats inside a haplotype"
        fwd.update(own)
    assert not any(revcomp(x) in fwd for x in fwd), "a k-mer and its reverse complement: the strands touch"


# ---- 1. tips -------------------------------------------------------------------------------------------------------------------------
TIP_T = (1, 2, 3, 4, 6, 7, 8, 9, 10, 41, 42, 43, 149, 150, 151)       # T - 1, T, T + 1 for max_tip_len T = 2, 3, 7, 8, 9, 2k = 42, 150
TIP_RUNS = (2, 3, 7, 8, 9, 150, 0, -1)
MARGIN = 200                                                          # more nodes than the longest walk (max_tip_len 150) takes


def tips_removed(t, max_tip_len, k):
    """Trim(len) walks i = 1 .. len - 1 and needs step t to see the junction (or the far end of a free piece): a tip of t nodes goes
    iff t <= len - 1, and the largest len RemoveTips uses is max_tip_len itself (2, 4, 8, ... stay below it)"""
    T = 2 * k if max_tip_len == -1 else max_tip_len
    return T > 0 and t <= T - 1


def tips_backbone(k=21):
    """one backbone; for every t an out-tip (leaves the backbone) and an in-tip (joins it) of t nodes, each at a junction of its own"""
    rng = _rng("tips_backbone")
    gap = 40
    B = _rand(rng, 2 * MARGIN + 2 * gap * len(TIP_T))
    haps, reads = [B], tile(B, k + 11)
    for i, t in enumerate(TIP_T):
        p = MARGIN + 2 * gap * i
        s = _rand(rng, t)
        out = B[p - k:p] + _other(rng, B[p]) + s[1:]                  # t new nodes, the last without a way out
        q = p + gap
        inn = s[::-1][:t - 1] + _other(rng, B[q - 1]) + B[q:q + k]    # t new nodes, the first without a way in
        haps += [out, inn]
        reads += tile(out, k + 11) + tile(inn, k + 11)
    check_unique_kmers(haps, k)
    want = {T: 4 * sum(tips_removed(t, T, k) for t in TIP_T) for T in TIP_RUNS}       # out and in, both strands
    return reads, dict(k=k, runs=[(T, True, 0) for T in TIP_RUNS], n_tips=want)


def tips_free(k=21):
    """free-standing pieces of t nodes (k + t - 1 bases): in-degree 0 at one end, out-degree 0 at the other; node_indegree_zero decides"""
    rng = _rng("tips_free")
    ts = [t for t in TIP_T if t >= 2]                                  # (one node alone has no edge: not in a graph)
    haps = [_rand(rng, k + t - 1) for t in ts] + [_rand(rng, 2 * MARGIN)]
    check_unique_kmers(haps, k)
    reads = [r for h in haps for r in tile(h, k + 11)]
    want = {T: 2 * sum(tips_removed(t, T, k) for t in ts) for T in TIP_RUNS}
    return reads, dict(k=k, runs=[(T, True, 0) for T in TIP_RUNS], n_tips=want)


def tips_nested(k=21):
    """a tip on a tip (a branch of 3 nodes whose first node carries a branch of 1), leaving and joining the backbone, and two tips
    (2 and 3 nodes) on one junction, leaving and joining.  Trim(2) takes the inner branch; only then is the outer one a tip of 3 nodes
    for Trim(4) -- on the snapshot of a single Trim(max_tip_len) its walk would stop at the inner junction after two nodes"""
    rng = _rng("tips_nested")
    B = _rand(rng, 2 * MARGIN + 200)
    p1, p2, p3, p4 = MARGIN, MARGIN + 50, MARGIN + 100, MARGIN + 150
    o = _other(rng, B[p1]) + _rand(rng, 2)
    outer_out = B[p1 - k:p1] + o
    inner_out = outer_out[1:k + 1] + _other(rng, o[1])                # leaves the outer branch's first node
    i3 = _rand(rng, 2) + _other(rng, B[p2 - 1])
    outer_in = i3 + B[p2:p2 + k]
    inner_in = _other(rng, i3[1]) + outer_in[2:k + 2]                 # joins the outer branch's last node
    a = _other(rng, B[p3])
    twin_out = [B[p3 - k:p3] + a + _rand(rng, 1), B[p3 - k:p3] + _other(rng, B[p3], a) + _rand(rng, 2)]
    b = _other(rng, B[p4 - 1])
    twin_in = [_rand(rng, 1) + b + B[p4:p4 + k], _rand(rng, 2) + _other(rng, B[p4 - 1], b) + B[p4:p4 + k]]
    haps = [B, outer_out, inner_out, outer_in, inner_in] + twin_out + twin_in
    check_unique_kmers(haps, k)
    reads = [r for h in haps for r in tile(h, k + 11)]
    # per strand: the two inner branches from max_tip_len 2 on, the twins of 2 nodes from 3 on, the outer branches and the twins of 3 from 4 on
    want = {0: 0, 2: 4, 3: 8, 4: 16, 7: 16, 150: 16}
    return reads, dict(k=k, runs=[(T, True, 0) for T in want], n_tips=want)


# ---- 2. bubble length ----------------------------------------------------------------------------------------------------------------
def bubble_span(k, delta, n_snps):
    """two haplotypes, n_snps linked SNPs (neighbours at most k apart: no (k+1)-mer between them is shared), first to last k + delta
    bases: begin edge, k + 1 + span differing edges, end edge at j = k + 2 + span, and the search looks at j < 2k + 4"""
    rng = _rng(f"bubble_span_{k}_{delta}_{n_snps}")
    span, flank = k + delta, k + 20
    A = _rand(rng, 2 * flank + span + 1)
    sites = [flank + round(span * i / (n_snps - 1)) for i in range(n_snps)]
    assert all(b - a <= k for a, b in zip(sites, sites[1:])) and sites[-1] - sites[0] == span
    Bl = list(A)
    for s in sites:
        Bl[s] = _other(rng, A[s])
    B = "".join(Bl)
    check_unique_kmers([A, B], k)
    pops = k + 2 + span < 2 * k + 4
    begin = [A[sites[0] - k - 1:sites[0]], revcomp(A[sites[-1] + 1:sites[-1] + k + 2])]        # the edges whose out-edges are the alleles
    return tile(A, k + 11) + tile(B, k + 11), dict(k=k, runs=[(150, False, 0), (0, False, 0)], span=span, pops=pops, begin=begin,
                                                   n_bubbles=2 if pops else 0, n_candidates=2 if pops else 0, n_contigs=1 if pops else 4,
                                                   n_rounds=1 if pops else 0)


# ---- 3. branch count -----------------------------------------------------------------------------------------------------------------
def branch_count(H, k=21):
    """H haplotypes that differ at sites 5 bases apart inside one window: two sites of four alleles give up to 16 branches, a third site
    the 17th and 18th.  A branch split after the begin edge shares its first edges with its sibling, so Pop undoes itself: what the
    limit of 16 decides is whether the window's begin edges are candidates, never the contigs"""
    rng = _rng("branch_count")                                         # (one base sequence for every H)
    flank = k + 20
    base = _rand(rng, 2 * flank + 11)
    s = [flank, flank + 5, flank + 10]
    combos = sorted(itertools.product(range(4), repeat=2), key=lambda ij: (max(ij), ij))   # (0,0) (0,1) (1,0) (1,1) ...: both sites vary from H = 3 on
    combos = [(i, j, 0) for i, j in combos] + [(0, 0, 1), (0, 1, 1)]
    haps = []
    for a in combos[:H]:
        h = list(base)
        for site, x in zip(s, a):
            h[site] = "ACGT"[(CODE[base[site]] + x) & 3]
        haps.append("".join(h))
    check_unique_kmers(haps, k)
    last = s[2] if H > 16 else s[1]
    begin = [base[s[0] - k - 1:s[0]], revcomp(base[last + 1:last + k + 2])]
    return [r for h in haps for r in tile(h, k + 11)], dict(k=k, runs=[(0, False, 0)], H=H, begin=begin, is_candidate=H <= MAX_BRANCHES,
                                                            n_bubbles=0, n_candidates=2 if H <= MAX_BRANCHES else 0,
                                                            n_rounds=2 if H <= MAX_BRANCHES else 0)     # (one for the pass, one for the pass over the pops that undid themselves)


# ---- 4. one site, designed coverage --------------------------------------------------------------------------------------------------
def single_site(cov, k=21):
    """one site, allele i ("ACGT"[i]) covered cov[i] times (reads of k + 1 bases: one edge each).  An edge weighs 1 (seen once) or 2;
    every branch has the same number of edges, so the heaviest alleles tie and `>=` keeps the LAST of them in out-edge order -- edges
    leave a node from its last (T) down to its first (A): the smallest letter of the tie on this strand, the smallest complement, that
    is the largest letter, on the other strand"""
    rng = _rng("single_site")
    flank = k + 20
    base = _rand(rng, 2 * flank + 1)
    haps = [base[:flank] + "ACGT"[i] + base[flank + 1:] for i in range(len(cov))]
    check_unique_kmers(haps, k)
    weight = [1 if c == 1 else 2 for c in cov]
    tie = [i for i, w in enumerate(weight) if w == max(weight)]
    window = lambda i: haps[i][flank - k:flank + k + 1]
    keep = sorted({tie[0], tie[-1]})
    return [r for h, c in zip(haps, cov) for r in tile(h, k + 1, c)], dict(
        k=k, runs=[(0, False, 0), (-1, False, 0)], n_bubbles=2, n_candidates=2, n_contigs=1, n_rounds=1, survivors=[window(i) for i in keep],
        losers=[window(i) for i in range(len(cov)) if i not in keep])


# ---- 5. fans -------------------------------------------------------------------------------------------------------------------------
FAN_TAIL = 8                                                           # edges between a bubble's end edge and the split


def _stem(rng, k, n_snps=1):
    """flank, SNP (, k + 3 bases, SNP), the end edge and FAN_TAIL more: -> (the two haplotypes, the begin edges of every bubble, this
    strand's first)"""
    flank = k + 20
    sites = [flank + (k + 3) * i for i in range(n_snps)]
    A = _rand(rng, sites[-1] + 1 + k + 1 + FAN_TAIL)
    Bl = list(A)
    for s in sites:
        Bl[s] = _other(rng, A[s])
    return [A, "".join(Bl)], [A[s - k - 1:s] for s in sites] + [revcomp(A[s + 1:s + k + 2]) for s in sites]


def fan(F, S, k=31):
    """S independent stems, one SNP bubble each; FAN_TAIL edges after the bubble's end the stem splits into F random continuations of
    2k + 10 bases, one read each.  The forward region of a begin edge (2k + 4 levels) runs k + 2 + FAN_TAIL levels to the split and the
    rest inside the fan: F = 4 stays under the narrow walk's 512 edges, F = 100 takes the wide walk and fits, F = 1500 passes 16384 edges
    with no level over 2048, F = 2100 puts more than 2048 edges on one level long before that.  (S = 4 for the two small fans; one stem
    of 1500 or 2100 continuations is 2 to 3 x 10^5 edges already.)"""
    rng = _rng(f"fan_{F}_{S}")
    reads, begin, haps = [], [], []
    for _ in range(S):
        st, b = _stem(rng, k)
        haps += st
        begin += b
        reads += tile(st[0], k + 11) + tile(st[1], k + 11)
        reads += [st[0][-k:] + _rand(rng, 2 * k + 10) for _ in range(F)]
    check_unique_kmers(haps, k)
    regime = {4: "narrow", 100: "wide", 1500: "seen", 2100: "frontier"}[F]
    return reads, dict(k=k, runs=[(0, False, 0)], F=F, S=S, begin=begin, regime=regime, n_bubbles=2 * S, n_candidates=2 * S,
                       n_rounds=1)          # (nothing a candidate reads lies in another one's reach: fitting or not, every check passes at once)


def _trie_levels(strings, depth):
    return [len({s[:d] for s in strings if len(s) >= d}) for d in range(1, depth + 1)]


def fan_chain(kind, over, k=31):
    """Two stems of two bubbles A, B each, k + 3 apart, so that A's reach holds B's begin edge.  A is the lower edge: it commits first and
    B's check fails in that round.  The first stem ends in a fan that puts B's region exactly AT a shipped limit (over = 0:
    it still fits) or one edge past it (over = 1): kind "seen": 16384 / 16385 edges in all, no level over 1500; kind "frontier": 2048 /
    2049 edges on the widest level, under 8000 in all.  A region that fits only waits; one that does not fit and fails its check is the
    round's barrier and holds back the second stem too, whose B then needs a round more: the number of rounds shows the verdict."""
    rng = _rng(f"fan_chain_{kind}")                                     # (one drawing for both sides of the limit)
    max_len = 2 * k + 4
    depth = max_len - (k + 2 + FAN_TAIL)                               # levels of B's region that lie inside the fan
    reads, begin, haps = [], [], []
    order = lambda e: (e[k - 1::-1], e[k])                               # edges are sorted by their node's k-mer read backwards, then by their own symbol
    while len(haps) < 4:                                               # A < B < A' < B' as edges: drawn until it is so
        st, b = _stem(rng, k, 2)
        if order(b[0]) < order(b[1]) and (not begin or order(begin[1]) < order(b[0])):
            haps += st
            begin += b
            reads += tile(st[0], k + 11) + tile(st[1], k + 11)
    check_unique_kmers(haps, k)
    root = haps[0][-k:]
    if kind == "frontier":                                             # 2048 (+ over) distinct strings of 8 bases: the last level is the widest
        seen = set()
        while len(seen) < REACH_FRONTIER + 1:
            seen.add(_rand(rng, 8))
        conts = sorted(seen)[:REACH_FRONTIER] + ([sorted(seen)[REACH_FRONTIER]] if over else [])
    else:                                                              # a trie of exactly the number of edges that is missing up to 16384 (+ over)
        target = REACH_MAX + over - (2 * k + 4 + FAN_TAIL)             # less the begin edge, 2 (k + 1) branch edges, the end edge and the tail
        conts = [_rand(rng, depth) for _ in range(600)]
        while sum(_trie_levels(conts, depth)) < target - depth:
            conts.append(_rand(rng, depth))
        while (have := sum(_trie_levels(conts, depth))) < target:      # a sibling that leaves an existing string `need` levels before the end
            need = min(depth - 8, target - have)
            stem = conts[int(rng.integers(0, len(conts)))][:depth - need]
            used = {s[len(stem)] for s in conts if s.startswith(stem) and len(s) > len(stem)}
            if len(used) < 4:
                conts.append(stem + _other(rng, *used) + _rand(rng, need - 1))
    reads += [root + c for c in conts]
    return reads, dict(k=k, runs=[(0, False, 0)], kind=kind, over=over, begin=begin, n_bubbles=8, n_candidates=8, n_rounds=2 + over)


# ---- 6. closed shapes ----------------------------------------------------------------------------------------------------------------
def ring(snp, k=21):
    """a 300-base sequence tiled round its end: a cycle of simple edges on either strand, no edge of which ends a path; with one SNP,
    a ring with a bubble"""
    rng = _rng("ring")
    R = _rand(rng, 300)
    haps = [R] + ([R[:150] + _other(rng, R[150]) + R[151:]] if snp else [])
    check_unique_kmers([h + h[:k - 1] for h in haps], k)
    return [r for h in haps for r in tile(h + h[:k + 10], k + 11)], dict(k=k, runs=[(150, False, 0), (0, False, 0)], n_bubbles=2 if snp else 0)


SHAPES = {"tips_backbone": (tips_backbone, ()), "tips_free": (tips_free, ()), "tips_nested": (tips_nested, ())}
for _k, _d, _n in [(21, 0, 3), (21, 1, 3), (21, 2, 3), (21, 0, 2), (21, 0, 5), (21, 1, 5), (21, 2, 5), (32, 1, 3), (32, 2, 3), (63, 1, 3), (63, 2, 3)]:
    SHAPES[f"span_k{_k}_p{_d}_s{_n}"] = (bubble_span, (_k, _d, _n))
for _h in (4, 15, 16, 17, 18):
    SHAPES[f"branches_{_h}"] = (branch_count, (_h,))
for _c in [(1, 2, 5), (5, 2, 1), (2, 2), (1, 1, 1, 1), (3, 1, 3, 1)]:
    SHAPES["site_" + "_".join(map(str, _c))] = (single_site, (_c,))
for _f, _s in [(4, 4), (100, 4), (1500, 1), (2100, 1)]:
    SHAPES[f"fan_{_f}"] = (fan, (_f, _s))
for _kind in ("seen", "frontier"):
    for _o in (0, 1):
        SHAPES[f"chain_{_kind}_{_o}"] = (fan_chain, (_kind, _o))
SHAPES["ring"] = (ring, (False,))
SHAPES["ring_snp"] = (ring, (True,))
GOLDEN_SHAPES = [n for n in SHAPES if not n.startswith("chain_")]      # (the chains are the fans' regions again: oracle and model only)
SPAN_SHAPES = [n for n in SHAPES if n.startswith("span_")]
BRANCH_SHAPES = [n for n in SHAPES if n.startswith("branches_")]
SITE_SHAPES = [n for n in SHAPES if n.startswith("site_")]
FAN_SHAPES = [n for n in SHAPES if n.startswith("fan_")]
CHAIN_SHAPES = [n for n in SHAPES if n.startswith("chain_")]
TIP_SHAPES = ["tips_backbone", "tips_free", "tips_nested"]


def make(name):
    fn, args = SHAPES[name]
    return fn(*args)


# ---- restatements over NavRef ---------------------------------------------------------------------------------------------------------
def _out(ref, e):
    row = ref.outgoing(np.array([e], np.int64), packed=False)[0]
    return [int(x) for x in row[1:1 + max(int(row[0]), 0)]]


def _weight(ref, e):
    return 2 - int(ref.multi1[e])


def search(ref, begin, max_branches=MAX_BRANCHES, reads=None, max_len=None):
    """BranchGroup::Search (branch_group.cpp:22-103) -> (branches, weights) or None.  reads (a list): every edge whose validity the
    search looks at is appended, in the order the device's search hands them to its sink"""
    sink = reads.append if reads is not None else (lambda e: None)
    if ref.invalid[begin]:
        return None
    sink(begin)
    out = _out(ref, begin)
    for x in out:
        sink(x)
    if len(out) <= 1 or len(out) > max_branches:
        return None
    branches, weights = [[begin]], [0]
    for j in range(1, 2 * ref.k + 4 if max_len is None else max_len):
        for i in range(len(branches)):
            out = _out(ref, branches[i][-1])
            for x in out:
                sink(x)
            if not out:
                return None                       # a dead end: the reference runs on and never converges
            if len(branches) + len(out) - 1 > max_branches:
                return None
            w0 = weights[i]
            head = branches[i][:]
            branches[i].append(out[0])
            weights[i] = w0 + _weight(ref, out[0])
            for x in out[1:]:
                branches.append(head + [x])
                weights.append(w0 + _weight(ref, x))
        for b in branches:
            d, inc = ref.incoming1(b[-1])
            for x in inc:
                sink(x)
            if d != 1 and any(all(o[j - 1] != x for o in branches) for x in inc):
                return None
        end = branches[0][-1]
        out = _out(ref, end)
        for x in out:
            sink(x)
        if len(out) == 1 and all(b[-1] == end for b in branches):
            return (branches, weights) if begin != end else None
    return None


def candidates(ref, max_branches=MAX_BRANCHES):
    """the valid edges a search succeeds from, ascending"""
    every = np.nonzero(~ref.invalid)[0].astype(np.int64)
    deg = ref.outgoing(every, packed=False)[:, 0]
    return [int(e) for e in every[deg >= 2] if search(ref, int(e), max_branches) is not None]


def edge_of(ref, og, kmer1):
    """the edge that spells this (k+1)-mer: looked up by the oracle's index, confirmed by the restated Label"""
    e = og.index_edge(kmer1)
    assert e >= 0, kmer1
    lab = "".join("ACGT"[c - 1] for c in ref.label(np.array([e]))[0]) + "ACGT"[int(ref.lab[e]) - 1]
    assert lab == kmer1
    return int(e)


def region(ref, begin, levels=None):
    """the reach walk's counts: -> (edges seen, begin included; new edges per level), over `levels` (2k + 4) forward steps"""
    seen = np.array([begin], np.int64)
    cur, per_level = seen, []
    for _ in range(2 * ref.k + 4 if levels is None else levels):
        if cur.size == 0:
            break
        o = ref.outgoing(cur, packed=False)[:, 1:]
        new = np.setdiff1d(np.unique(o[o >= 0]), seen)
        per_level.append(int(new.size))
        seen = np.union1d(seen, new)
        cur = new
    return int(seen.size), per_level


def reach(ref, begin):
    """the edges within 2k + 4 forward steps of begin, begin first"""
    seen = np.array([begin], np.int64)
    cur, found = seen, [begin]
    for _ in range(2 * ref.k + 4):
        if cur.size == 0:
            break
        o = ref.outgoing(cur, packed=False)[:, 1:]
        cur = np.setdiff1d(np.unique(o[o >= 0]), seen)
        found += cur.tolist()
        seen = np.union1d(seen, cur)
    return found


def verdict(seen, per_level, reach_max=REACH_MAX, frontier=REACH_FRONTIER, narrow_max=NARROW_MAX):
    """which walk takes the region and whether it fits: the level at which a walk stops is the first at which the running count passes
    the limit or the level holds more than `frontier` edges"""
    total = 1
    for n in per_level:
        total += n
        if n > frontier and total <= reach_max:
            return "frontier"
        if total > reach_max:
            return "seen" if n <= frontier else "both"
    return "narrow" if seen <= narrow_max else "wide"


def model_rounds(ref, cands, fits):
    """The ordered rounds of the device's PopBubbles as the head comment of denovo.hip states them, for a list of candidates that fits one
    window.  fits(begin) says whether a candidate's region fits its scratch.  Every pending candidate stamps, with its rank, its reach
    (the edges within 2k + 4 forward steps and the valid edges into them) or, if the region does not fit, what its search reads today;
    the lowest rank wins an edge.  A candidate commits iff every edge its search reads carries its own stamp and no lower candidate
    whose region does not fit failed its check.  -> the number of rounds, CHANGING ref.invalid as the pops do."""
    pending, rounds, marked, again, known_big = list(cands), 0, set(), [], set()
    for second in (False, True):
        while pending:
            rounds += 1
            ref._l = None                                              # (the cached lists of the graph as it was)
            owner, big = {}, {}
            for rank, b in enumerate(pending):
                if ref.invalid[b]:
                    continue
                big[b] = b in known_big or not fits(b)                 # (once it did not fit, a candidate is not walked again)
                if big[b]:
                    known_big.add(b)
                    mine = []
                    search(ref, b, reads=mine)
                else:
                    mine = [b] + [x for e in reach(ref, b)[1:] for x in [e] + ref.incoming1(e)[1]]
                for e in mine:
                    owner.setdefault(e, rank)                          # ranks ascend: the first to ask is the lowest
            barrier, verdicts = len(pending), []
            for rank, b in enumerate(pending):
                mine = []
                found = search(ref, b, reads=mine)
                ok = all(owner.get(e) == rank for e in mine if not ref.invalid[e])
                verdicts.append((ok, found))
                if not ok and big.get(b):
                    barrier = min(barrier, rank)
            keep = []
            for rank, b in enumerate(pending):
                ok, found = verdicts[rank]
                if not ok or rank > barrier:
                    keep.append(b)
                elif found and not _pop(ref, marked, *found):
                    again.append(b)
            assert len(keep) < len(pending), "the lowest pending candidate always commits"
            pending = keep
        if second:
            break
        pending, again = again, []
    ref._l = None
    return rounds


def _pop(ref, marked, branches, weights):
    """BranchGroup::Pop (branch_group.cpp:105-141), one thread"""
    best = max(range(len(branches)), key=lambda i: (weights[i], i))       # `>=`: the last of the heaviest
    locked = []
    for b in branches:
        for e in b[1:-1]:
            if e in marked:
                for u in locked:
                    marked.discard(u)
                    ref.invalid[u] = False
                return False
            marked.add(e)
            locked.append(e)
            ref.invalid[e] = True
    for e in branches[best][1:-1]:
        ref.invalid[e] = False
        marked.discard(e)
    return True
