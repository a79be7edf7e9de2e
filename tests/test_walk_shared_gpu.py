"""The read walk that match_walk_kernel, sample_scan_kernel and pile_scan_kernel each write out (csrc/coverage.hip, csrc/pileup.hip)
is one walk: on one set of reads the three read-consuming calls -- Graph.match_reads with counts, Graph.contig_sample_coverage with one
library and Graph.pileup -- must tell one story, in both storage orders of the reads.

The reads take every branch of the walk: no window and exactly one; a first base at every residue of the packed position mod 16; a
substituted base in the middle, so that a step fails, k + 1 windows have no edge and an index search brings the walk back; copies of
contig pieces on both strands; random reads.  The graph is the `-m 1` graph of OTHER reads (error-free reads that tile the genome), so a
window has an edge exactly when it is a (k+1)-mer of the genome on either strand, and every expectation is a count over strings."""
import numpy as np
import pytest

from megagta_amd import readlib

pytestmark = pytest.mark.gpu
DNA = "ACGT"
COMP = str.maketrans("ACGT", "TGCA")
K = 20
GENOME = 3000


def rc(s):
    return s.translate(COMP)[::-1]


def to_str(codes):
    return "".join(DNA[c] for c in codes)


def to_codes(s):
    return np.array([DNA.index(c) for c in s], dtype=np.uint8)


def windows(s):
    return [s[p:p + K + 1] for p in range(len(s) - K)]


def make_inputs(seed=20):
    rng = np.random.default_rng(seed)
    genome = to_str(rng.integers(0, 4, GENOME))
    # the graph: reads of 100 letters every 50, every second one reverse-complemented -- every window of the genome is an edge
    graph_reads = [genome[p:p + 100] for p in range(0, GENOME - 99, 50)]
    graph_reads = [rc(s) if i % 2 else s for i, s in enumerate(graph_reads)]
    contigs = []
    for i in range(40):                                                    # pieces of the first two thirds of the genome
        n = int(rng.integers(60, 201))
        p = int(rng.integers(0, 2000 - n))
        contigs.append(rc(genome[p:p + n]) if i % 3 == 0 else genome[p:p + n])
    reads = [genome[7:7 + n] for n in (0, 1, 5, K - 1, K, K + 1, K + 1, K + 2)]     # no window, exactly one, two
    for i in range(130):                                                   # copies of contig pieces, both strands, every length
        c = contigs[i % len(contigs)]
        n = int(rng.integers(K + 1, min(120, len(c)) + 1))
        p = int(rng.integers(0, len(c) - n + 1))
        reads.append(rc(c[p:p + n]) if i % 2 else c[p:p + n])
    for i in range(130):                                                   # a substituted base in the middle: out of the graph and back
        n = int(rng.integers(3 * K, 121))
        p = int(rng.integers(0, GENOME - n + 1))
        s = genome[p:p + n]
        at = int(rng.integers(K + 2, n - K - 2))
        s = s[:at] + DNA[(DNA.index(s[at]) + 1 + i % 3) % 4] + s[at + 1:]
        reads.append(rc(s) if i % 2 else s)
    for _ in range(130):                                                   # random reads
        reads.append(to_str(rng.integers(0, 4, int(rng.integers(0, 121)))))
    order = rng.permutation(len(reads))
    return genome, graph_reads, contigs, [reads[i] for i in order]


def expectation(genome, contigs, reads, reverse):
    """hit_windows per read, and the walk's counters: a window is searched when the window before it ON THE WALK has no edge (or there
    is none), and found by a step when both have one.  reverse = the walk runs along the reverse complement: last window first."""
    edges = set(windows(genome))
    edges |= {rc(w) for w in edges}
    both = {w for c in contigs for w in windows(c)}
    both |= {rc(w) for w in both}
    hits = np.array([sum(w in both and w in edges for w in windows(s)) for s in reads], dtype=np.uint32)
    walked = searched = 0
    for s in reads:
        on = [w in edges for w in windows(s)]
        if reverse:
            on.reverse()
        for p, e in enumerate(on):
            if p and on[p - 1]:
                walked += e
            else:
                searched += 1
    return hits, walked, searched


@pytest.fixture(scope="module")
def world():
    from megagta_amd import api
    ctx = api.Context(0)
    genome, graph_reads, contigs, reads = make_inputs()
    g = api.Graph(ctx, ctx.build_sdbg(ctx.upload_reads(*readlib.pack_for_build([to_codes(s) for s in graph_reads])), K))
    yield dict(ctx=ctx, g=g, genome=genome, contigs=contigs, reads=reads)
    ctx.close()


def test_inputs_take_every_branch(world):
    reads, genome = world["reads"], world["genome"]
    lens = np.array([len(s) for s in reads])
    start = np.concatenate([[0], np.cumsum(lens)])
    assert 350 <= len(reads) <= 450 and lens.max() <= 120 and len(world["contigs"]) == 40
    assert {0, K, K + 1} <= set(lens.tolist())
    for first in (start[:-1], start[1:]):                                  # the first walked base, as sequenced and stored reversed
        assert {int(x) % 16 for x, n in zip(first, lens) if n > K} == set(range(16))
    hits, walked, searched = expectation(genome, world["contigs"], reads, False)
    n_with = int((lens > K).sum())
    assert searched > n_with + 100 and walked > 1000                       # steps fail and searches restart
    assert (hits > 0).sum() > 100 and (hits[lens > K] == 0).sum() > 50
    edges = set(windows(genome)) | {rc(w) for w in windows(genome)}
    assert any((lambda on: any(on[p] and not on[p + 1] for p in range(len(on) - 1)) and any(not on[p] and on[p + 1] for p in range(len(on) - 1)))
               ([w in edges for w in windows(s)]) for s in reads)          # out in the middle and back


@pytest.mark.parametrize("reverse", [True, False], ids=["stored_reversed", "stored_as_sequenced"])
def test_three_read_scans_tell_one_story(world, reverse):
    ctx, g, contigs, reads = world["ctx"], world["g"], world["contigs"], world["reads"]
    arrs = [to_codes(s) for s in reads]
    if reverse:
        packed, start = readlib.pack_for_build(arrs)
    else:
        start = np.zeros(len(arrs) + 1, dtype=np.uint64)
        np.cumsum([a.size for a in arrs], out=start[1:])
        packed = readlib.pack_codes(np.concatenate(arrs))
    rd = ctx.upload_reads(packed, start)
    try:
        m = g.match_reads(rd, contigs, counts=True, reads_reversed=reverse)
        s = g.contig_sample_coverage(rd, [len(reads)], contigs, reads_reversed=reverse)
        p = g.pileup(rd, contigs, reads_reversed=reverse)
    finally:
        rd.free()
    want, walked, searched = expectation(world["genome"], contigs, reads, reverse)
    ms, ss, ps = m["stats"], s["stats"], p["stats"]
    print("hit windows", int(m["hit_windows"].sum()), int(s["lib_hit_windows"][0]), ps["n_hit_windows"], "expected", int(want.sum()))
    print("read windows", ms["n_read_windows"], ss["n_read_windows"], ps["n_read_windows"])
    print("walked", ms["n_walked"], ss["n_read_walked"], ps["n_read_walked"], "expected", walked)
    print("searches", ms["n_index_searches"], ss["n_read_index_searches"], ps["n_read_index_searches"], "expected", searched)
    assert np.array_equal(m["hit_windows"], want)
    assert int(m["hit_windows"].sum()) == int(s["lib_hit_windows"][0]) == ps["n_hit_windows"] == ss["n_hit_windows"]
    assert ms["n_read_windows"] == ss["n_read_windows"] == ps["n_read_windows"] == sum(max(0, len(x) - K) for x in reads)
    assert ms["n_walked"] == ss["n_read_walked"] == ps["n_read_walked"] == walked
    assert ms["n_index_searches"] == ss["n_read_index_searches"] == ps["n_read_index_searches"] == searched
    assert np.array_equal(m["bits"], want > 0) and ms["n_matched_reads"] == int((want > 0).sum())
