"""What tests/test_walk_edges_host.py and tests/test_walk_edges_gpu.py share: the inputs, the (k+1)-mer -> edge dict, the census of the
branches of the forward step, and the expectations over strings.  No fixtures, no device.

The window walk (csrc/walk.hpp) finds the edge of every (k+1)-letter window: an index search for the first window, one forward step
(cov_step) per further window.  The loop stands in five places -- walk_next / walk_contig, share_walk_kernel, match_walk_kernel,
sample_scan_kernel, pile_scan_kernel -- and the tests hold each of them to the EDGE, not to a number that several edges share.

The device that shows an edge id through the existing calls: a record's high byte is its stored multiplicity, 255 = "the full count is
the next `large` word".  With every high byte at 255 and large[i] = i + 1 the multiplicity of edge i is i + 1 (tagged_stream), so a
per-window coverage IS the id + 1 of the edge the walk found, 0 for none.  That needs size < 65 535 and moves only the multi1 bits,
which the walk does not read.

Expected ids never come from the device: edge_of maps label(e) + the letter of W(e) to e, from the oracle's Label alone, for every edge
with W != 0 whose node is no tip.  A tip node is left out because IndexBinarySearchEdge never answers one (succinct_dbg.cpp:455-457:
"a tip never matches"); its stored label stands for $ x1 .. x(k-1) with the $ read as A, which is no k-mer of the input.  The host test
asserts that the oracle's index search finds none of them, and pins the dict to that search on present and absent windows.

A tip node has no edge into it, so no step lands on one and no search finds one: in a graph as loaded, the edges with W != 0 whose
validity bit is set -- the tip edges -- are starts only in the census.  The walk does start from edges whose validity bit is set once
`denovo` has consumed the bits; census(w, invalid=...) counts those starts, and the device test repeats every call on such a graph.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

from tests import graph_nav_ref as R

KS = (20, 31, 32, 63, 64, 95, 127)
DENOVO_KS = (31, 64)
SEEDS = {k: 900 + k for k in KS}
DNA = "ACGT"
SYM = "$ACGT"
_COMP = str.maketrans("ACGT", "TGCA")
MIN_READS = 20000                      # of the read walks
_CACHE = {}


def rc(s: str) -> str:
    return s.translate(_COMP)[::-1]


def to_str(codes) -> str:
    return "".join(DNA[c] for c in codes)


def make_reads(k: int) -> list:
    from megagta_amd import synth
    return synth.make_strain_mix(SEEDS[k], n_genomes=3, genome_len=1600, read_len=max(100, k + 40), snp_every=60, tricky=True)


def get(k: int, oracle) -> dict:
    """-> dict(k, reads, read_strs, packed, start, stream, es, og, ref (graph_nav_ref.NavRef), kmer (label + letter per edge, None where
    W = 0), starts (the edges with W != 0), edge_of); built once per process"""
    if k in _CACHE:
        return _CACHE[k]
    from megagta_amd import readlib
    reads = make_reads(k)
    packed, start = readlib.pack_for_build(reads)
    stream = oracle.Stream.build(packed, start, k)                          # -m 1: tips, $ edges and minus edges
    og = oracle.Graph(stream)
    ref = R.NavRef.from_oracle(og)
    lab = ref.lab.tolist()
    kmer = [og.label(e) + SYM[lab[e]] if lab[e] else None for e in range(og.size)]
    tip = ref.tip.tolist()
    edge_of = {kmer[e]: e for e in range(og.size) if kmer[e] is not None and not tip[e]}
    w = dict(k=k, reads=reads, read_strs=[to_str(r) for r in reads], packed=packed, start=start, stream=stream, es=stream.edges(), og=og, ref=ref,
             kmer=kmer, starts=np.nonzero(ref.W != 0)[0].astype(np.int64), edge_of=edge_of)
    _CACHE[k] = w
    return w


def tagged_stream(es, cls):
    """the stream with the multiplicity of edge i set to i + 1, as a `cls` (api.EdgeStream)"""
    n = es.records.size
    assert n < 65535
    return cls(k=es.k, words_per_tip=es.words_per_tip, bucket_items=es.bucket_items, records=(es.records | np.uint16(0xFF00)).astype(np.uint16),
               large=np.arange(1, n + 1, dtype=np.uint16), tips=es.tips)


# ---- the census: which branches of cov_step the steps of a graph take ----------------------------------------------------------------
def census(w: dict, invalid=None) -> dict:
    """Every step (e, c), e an edge with W != 0 and c a next letter, as cov_step (csrc/walk.hpp) takes it, from the bit vectors, f and
    the ranks alone (graph_nav_ref.NavRef: rank = cumsum, select = nonzero):
        a = the out-label of e;  r = rank_f[a] + Rank(a, e) - 1;  x = Select(last, r), the last edge of the target node;
        hint = fwd_hint[a - 1] of e's line as graph_hint_kernel leaves it (NavRef.hint);
        found = the edge in (the next lower last | tip bit, x] labelled c or c + 4, scanned from x downwards, -1 for none.
    -> dict(e int64[n], found int64[n, 4], hint_miss bool[n] (x's line lies behind the hint: the `while` runs), straddle bool[n, 4] (found in
    another line than x's), final bool[n] (e is the graph's last edge: total_w instead of the line's ranks), invalid bool[n] (the validity
    bit of e; `invalid` = bits to use in place of the loaded graph's), minus bool[n] (W > 4), r_beyond (steps with r >= total_last or < 0))"""
    ref = w["ref"]
    e = w["starts"]
    r = ref.fd_r(e)
    inside = (r >= 0) & (r < ref.total_last)
    x = np.where(inside, ref.select_last(np.clip(r, 0, ref.total_last - 1)), 0)
    y = ref.node_low(x)
    assert int((x - y).max()) <= 9                                         # a node has at most 8 edges (c and c + 4) and a $
    found = np.full((e.size, 4), -1, np.int64)
    for c in range(1, 5):
        for j in range(9):
            p = x - j
            hit = inside & (p > y) & (ref.lab[np.clip(p, 0, ref.size - 1)] == c) & (found[:, c - 1] < 0)
            found[hit, c - 1] = p[hit]
    bits = ref.invalid if invalid is None else invalid
    return dict(e=e, found=found, hint_miss=inside & ((x >> 6) > ref.hint(e)), straddle=(found >= 0) & ((found >> 6) != (x >> 6)[:, None]),
                final=e == ref.size - 1, invalid=bits[e], minus=ref.W[e] > 4, r_beyond=int((~inside).sum()))


def census_counts(cz: dict) -> dict:
    """the numbers the conditions are about; every one counts steps (e, c)"""
    f = cz["found"] >= 0
    per_step = lambda m: m[:, None] & np.ones((1, 4), bool)
    return dict(starts=int(cz["e"].size), found=int(f.sum()), none=int((~f).sum()), hint_miss=int(per_step(cz["hint_miss"]).sum()),
                hint_miss_found=int((per_step(cz["hint_miss"]) & f).sum()), straddle=int(cz["straddle"].sum()),
                final_found=int((per_step(cz["final"]) & f).sum()), invalid_found=int((per_step(cz["invalid"]) & f).sum()),
                minus_found=int((per_step(cz["minus"]) & f).sum()), r_beyond=cz["r_beyond"])


def invalid_after_denovo(w: dict, oracle):
    """-> (bool[size] validity bits after the oracle's denovo(150, False, 0), uint64 words of the same).  The oracle runs on a graph of
    its own of the TAGGED stream, read back from its files: `denovo` weighs an edge by its multi1 bit, which the tagging clears."""
    import os
    import tempfile
    from megagta_amd import api
    if "after_denovo" not in w:
        tagged = tagged_stream(w["es"], api.EdgeStream)
        with tempfile.TemporaryDirectory() as tmp:
            api.write_sdbg(os.path.join(tmp, "tagged"), tagged)
            stream = oracle.Stream.read(os.path.join(tmp, "tagged"))
        es = stream.edges()
        assert np.array_equal(es.records, tagged.records) and np.array_equal(es.large, tagged.large) and np.array_equal(es.tips, tagged.tips)
        og = oracle.Graph(stream)
        assert np.array_equal(og.bitvectors()["invalid"], w["og"].bitvectors()["invalid"]) and not og.bitvectors()["multi1"].any()
        og.denovo(150, False, 0)
        words = og.invalid_now()
        w["after_denovo"] = (R._bits(words, og.size), words)
    return w["after_denovo"]


# ---- the contig walks --------------------------------------------------------------------------------------------------------------------
def step_contigs(w: dict) -> list:
    """label(e) + W(e) + c for every edge e with W != 0 and every c, in the order of census()['found'].ravel(): k + 2 letters, window 0 is
    searched and window 1 is stepped (for an edge of a tip node window 0 has no edge, and window 1 is searched too)"""
    return [s + c for s in (w["kmer"][e] for e in w["starts"].tolist()) for c in DNA]


def straddle_contigs(w: dict, cz: dict) -> list:
    """the four 3-window extensions of every straddle step: the step behind it must carry the line of the edge found"""
    out = []
    for i, c in zip(*np.nonzero(cz["straddle"])):
        s = w["kmer"][int(cz["e"][i])] + DNA[c]
        out += [s + c2 for c2 in DNA]
    return out


def read_contigs(w: dict) -> list:
    """every read of the mix, and that read with one substituted base: long walks that leave the graph and return"""
    rng = np.random.default_rng(7000 + w["k"])
    out = list(w["read_strs"])
    for s in w["read_strs"]:
        at = int(rng.integers(0, len(s)))
        out.append(s[:at] + DNA[(DNA.index(s[at]) + int(rng.integers(1, 4))) % 4] + s[at + 1:])
    return out


def expected_ids(edge_of: dict, k: int, seqs: list):
    """-> (ids int64 back to back, -1 = no edge; offsets int64[n + 1]): a dict lookup per window"""
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([max(0, len(s) - k) for s in seqs], out=off[1:])
    get = edge_of.get
    ids = np.fromiter((get(s[p:p + k + 1], -1) for s in seqs for p in range(len(s) - k)), np.int64, int(off[-1]))
    return ids, off


def walk_counts(ids: np.ndarray, off: np.ndarray):
    """-> (searched bool[windows], walked bool[windows]): a window is searched when it is the first of its sequence or the window before
    it has no edge, and found by a step when both it and the window before it have an edge"""
    first = np.zeros(ids.size, bool)
    first[off[:-1][np.diff(off) > 0]] = True
    prev = np.concatenate([[-1], ids[:-1]])
    searched = first | (prev < 0)
    return searched, ~searched & (ids >= 0)


# ---- the read walks ----------------------------------------------------------------------------------------------------------------------
def canonical(w: dict) -> dict:
    """edge -> its canonical number: 1 + min(id(w), id(rc w)), 1 + the id alone where rc(w) has no edge.  (The + 1 -- the tag the lower
    of the two edges carries in the tagged graph -- gives every number a bit: edge 0 is an edge like any other, and with the plain id
    it would sit in none of the 16 calls.)"""
    edge_of = w["edge_of"]
    return {e: 1 + min(e, edge_of.get(rc(s), e)) for s, e in edge_of.items()}


def walk_reads(w: dict, cz: dict) -> list:
    """The reads of the read walks: the 2-window strings (step_contigs) of every hint-miss, straddle, final-edge and from-invalid step
    and their reverse complements (a read stored reversed is walked along its reverse complement, so the same step is then taken
    from the other copy), a seeded sample of the rest up to MIN_READS and at least 4 000, reads of k - 1, k, k + 1 and 0 letters; in a
    seeded random order"""
    k = w["k"]
    rng = np.random.default_rng(8000 + k)
    two = step_contigs(w)
    special = np.nonzero((cz["hint_miss"] | cz["final"] | cz["invalid"])[:, None] | cz["straddle"])
    special = np.unique(special[0] * 4 + special[1])
    rest = np.setdiff1d(np.arange(len(two)), special)
    reads = [two[i] for i in special.tolist()]
    reads += [rc(s) for s in reads]
    reads += [two[i] for i in rng.choice(rest, max(4000, MIN_READS - len(reads)), replace=False).tolist()]
    for i in rng.choice(rest, 12, replace=False).tolist():
        reads += [two[i][:n] for n in (k - 1, k, k + 1, 0)]
    return [reads[i] for i in rng.permutation(len(reads)).tolist()]


def read_expectation(w: dict, reads: list, reverse: bool) -> dict:
    """what the walk along every read finds, by dict lookups alone.  reverse = the reads are stored reversed: the walk runs along the
    reverse complement.  -> dict(ids, off (per read, in walk order), canon int64[windows] (the canonical number of the window's edge, -1
    for none), hits int64[16, n_reads] (the windows whose canonical number has bit b set), found int64[n_reads], walked, searched,
    windows)"""
    canon_of = w["canon"] if "canon" in w else w.setdefault("canon", canonical(w))
    ids, off = expected_ids(w["edge_of"], w["k"], [rc(s) for s in reads] if reverse else reads)
    canon = np.array([canon_of[e] if e >= 0 else -1 for e in ids.tolist()], np.int64)
    read_of = np.repeat(np.arange(len(reads)), np.diff(off))
    hits = np.zeros((16, len(reads)), np.int64)
    for b in range(16):
        np.add.at(hits[b], read_of[(canon >= 0) & ((canon >> b) & 1 == 1)], 1)
    found = np.bincount(read_of[ids >= 0], minlength=len(reads)).astype(np.int64)
    searched, walked = walk_counts(ids, off)
    return dict(ids=ids, off=off, canon=canon, hits=hits, found=found, walked=int(walked.sum()), searched=int(searched.sum()), windows=int(ids.size))


def canon_contigs(w: dict, bit=None) -> list:
    """one (k+1)-letter contig per canonical number, ascending; bit = b: of those with bit b set"""
    canon_of = w["canon"] if "canon" in w else w.setdefault("canon", canonical(w))
    return [w["kmer"][c - 1] for c in sorted(set(canon_of.values())) if bit is None or (c >> bit) & 1]


def window_counts(w: dict, contigs: list, reads: list, reverse: bool) -> np.ndarray:
    """per (k+1)-letter contig: the windows of the walk (along the reverse complement of a read stored reversed) equal to it or to its
    reverse complement, counted on strings.  (A window that equals rc(w) counts where rc(w) has an edge; a window that is its own
    reverse complement counts once.)"""
    k = w["k"]
    n = Counter(s[p:p + k + 1] for s in ([rc(s) for s in reads] if reverse else reads) for p in range(len(s) - k))
    return np.array([n[c] + (n[rc(c)] if rc(c) != c and rc(c) in w["edge_of"] else 0) for c in contigs], np.int64)


# ---- the same over strings alone, for the host test -----------------------------------------------------------------------------------------
def brute_force(graph_reads: list, k: int, contig_sets: list, reads: list, reverse: bool):
    """-> (hit windows per read for every set of contigs, walked, searched) with no graph at all: the edges of a `-m 1` graph are the
    (k+1)-mers of its reads on both strands; a window hits when it is one of them and equals a contig window on either strand"""
    win = lambda s: [s[p:p + k + 1] for p in range(len(s) - k)]
    edges = {x for s in graph_reads for x in win(s)}
    edges |= {rc(x) for x in edges}
    windows = [win(rc(s) if reverse else s) for s in reads]
    walked = searched = 0
    for ws in windows:
        on = [x in edges for x in ws]
        for p, o in enumerate(on):
            if p and on[p - 1]:
                walked += o
            else:
                searched += 1
    hits = []
    for contigs in contig_sets:
        both = {x for c in contigs for x in win(c)}
        both |= {rc(x) for x in both}
        both &= edges
        hits.append(np.array([sum(x in both for x in ws) for ws in windows], np.int64))
    return hits, walked, searched
