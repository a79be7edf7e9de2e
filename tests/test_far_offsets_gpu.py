"""Every stage that indexes the packed reads by start[r], on reads whose base offsets lie around and beyond 2^31 and 2^32.

The toy golden library (6000 reads of 150 bp, its k = 44 graph pinned to the reference binary's files) sits behind about 97.6 M filler
reads of 44 bases (helpers.reads_behind_marks; the layout itself is checked by test_far_offsets_host.py).  A filler read holds no
window of any stage, so every stage must give exactly what it gives for the payload alone, read numbers mapped through `ids`.  An
offset narrowed to 32 or 31 bits still lies inside the array: there the filler holds random bits (the decoys), so a wrapped read
yields foreign k-mers.  Every expectation comes from the payload alone: the oracle, the goldens and the Python restatements of the
stage tests.  One upload per mode serves all stages."""
import os

import numpy as np
import pytest

from megagta_amd import readlib
from tests import helpers as H
from tests import test_matchreads_gpu as MR
from tests import test_phase_gpu as PH
from tests import test_pileup_gpu as PL
from tests import test_samplecov_gpu as SC

pytestmark = pytest.mark.gpu

K = 44
FILL_LEN = 44                                  # <= k for the build at k = 44, < k for findstart at 45 and 72, < k + 1 for the window stages
SEED = 7
N_CONTIGS = 24


def strings(reads):
    return ["".join("ACGT"[x] for x in r) for r in reads]


@pytest.fixture(scope="module")
def payload(golden_dir, oracle):
    """the payload alone, on the host: reads, the oracle's k = 44 stream, the longest contigs of its graph, and the expectations that
    need no device (computed once, never changed)"""
    toy = os.path.join(golden_dir, "toy")
    reads = readlib.load_lib_bin(os.path.join(toy, "reads.lib"))
    strs = strings(reads)
    packed, start = readlib.pack_for_build(reads)
    ost = oracle.Stream.build(packed, start, K, threads=4)
    edges = ost.edges()
    assert edges.records.size > 10_000
    text, _ = oracle.Graph(ost).denovo(150, False, K + 2)
    seqs = sorted((l for l in text.splitlines() if l and l[0] != ">"), key=lambda s: (-len(s), s))[:N_CONTIGS]
    n1, n2 = H.split_payload(len(reads))
    # ... and pieces of the reads that lie across the marks and of the first read of B3, so that these reads match and are placed
    seqs += [strs[n1 // 2][10:140], MR.rc(strs[(n1 + n2) // 2]), strs[n2][5:120]]
    return dict(toy=toy, reads=reads, strs=strs, packed=packed, start=start, edges=edges, seqs=seqs, n=len(reads), n1=n1, n2=n2, at_marks=(n1 // 2, (n1 + n2) // 2, n2),
                golden=H.load_streams(os.path.join(toy, "sdbg_streams.json"))[str(K)])


@pytest.fixture(scope="module")
def alone(payload):
    """the payload uploaded alone: what the device says about it without any filler (findstart's raw hits, pileup's placements)"""
    from megagta_amd import api
    ctx = api.Context(0)
    rd = ctx.upload_reads(payload["packed"], payload["start"])
    g = api.Graph(ctx, payload["edges"])
    yield dict(ctx=ctx, rd=rd, g=g)
    g.free()
    rd.free()
    ctx.close()


def upload(ctx, reads, mode):
    packed, start, ids = H.reads_behind_marks(reads, FILL_LEN, mode, SEED)
    rd = ctx.upload_reads(packed, start)
    return rd, ids, int(start.size - 1), (packed.size + 16) * 4 + start.size * 8


@pytest.fixture(scope="module")
def far(request, payload):
    """the layout of one mode on the device, in a context of its own; the host copy is dropped after the upload"""
    from megagta_amd import api
    ctx = api.Context(0)
    rd, ids, n_reads, dev_bytes = upload(ctx, payload["reads"], request.param)
    assert n_reads > 90_000_000 and ids[payload["n2"]] > ids[payload["n1"] - 1] + 1_000_000
    yield dict(mode=request.param, ctx=ctx, rd=rd, ids=ids, n_reads=n_reads, dev_bytes=dev_bytes)
    rd.free()
    ctx.close()


BOTH_MODES = pytest.mark.parametrize("far", ["straddle", "exact"], indirect=True)
STRADDLE = pytest.mark.parametrize("far", ["straddle"], indirect=True)


def same_stream(got, want):
    assert got.k == want.k and got.words_per_tip == want.words_per_tip
    assert np.array_equal(got.bucket_items, want.bucket_items)
    assert np.array_equal(got.records, want.records)
    assert np.array_equal(got.large, want.large)
    assert np.array_equal(got.tips, want.tips)
    assert got.md5() == want.md5()


# ---- the build ------------------------------------------------------------------------------------------------------------------------
@BOTH_MODES
def test_build_m1(far, payload):
    """-m 1, k = 44: the whole range, a bucket sub-range, and a memory limit that forces several range passes"""
    ctx, rd, o = far["ctx"], far["rd"], payload["edges"]
    g = ctx.build_sdbg(rd, K)
    same_stream(g, o)
    assert g.md5() == payload["golden"]["md5"]                            # == the reference's buildgraph output
    assert g.stats["n_kmers"] == payload["n"] * (150 - K) and g.stats["n_reads"] == far["n_reads"]
    b0, b1 = 12345, 42346
    part = ctx.build_sdbg(rd, K, bucket_range=(b0, b1))
    lo, hi = int(o.bucket_items[:b0].sum()), int(o.bucket_items[:b1].sum())
    assert hi - lo > 10_000 and np.array_equal(part.records, o.records[lo:hi])
    assert np.array_equal(part.bucket_items[b0:b1], o.bucket_items[b0:b1]) and part.bucket_items.sum() == hi - lo
    ctx.set_mem_limit(far["dev_bytes"] + (24 << 20))                      # 24 MB next to the resident reads, as test_multi_pass_bucket_ranges
    try:
        many = ctx.build_sdbg(rd, K)
    finally:
        ctx.set_mem_limit(0)
    assert many.stats["n_passes"] > 1
    same_stream(many, o)
    assert many.md5() == payload["golden"]["md5"]


@BOTH_MODES
def test_build_m2_mercy(far, payload, oracle):
    """-m 2 --need_mercy, k = 44: stage 1, the mercy edges and stage 2"""
    ctx = far["ctx"]
    o = oracle.Stream.build_solid(payload["packed"], payload["start"], K, 2, True, threads=4)
    oe = o.edges()
    assert 10_000 < oe.records.size < payload["edges"].records.size
    g = ctx.build_sdbg(far["rd"], K, min_count=2, need_mercy=True)
    same_stream(g, oe)
    assert np.array_equal(ctx.last_counting(), o.counting) and o.counting.sum() > 0
    ctx.release_scratch()


# ---- findstart ------------------------------------------------------------------------------------------------------------------------
def check_findstart(far, payload, alone, rd, reversed_storage, k):
    from megagta_amd import findstart
    from oracle import findstart_oracle as F
    faa = os.path.join(payload["toy"], "ref_aligned.faa")
    words, mpos = findstart.reference_words(faa, k // 3)
    pw = findstart.pack_words(words, k // 3)
    ids, order = far["ids"], ["read", "pos_strand", "ref"]
    want_hits, _ = findstart.find_hits(alone["ctx"], alone["rd"], True, k, pw)
    # the toy library holds 93 distinct seeds at k = 45 and 29 at k = 72 (several reads each)
    assert want_hits.size > 50
    want_hits["read"] = ids[want_hits["read"].astype(np.int64)]
    hits, _ = findstart.find_hits(far["ctx"], rd, reversed_storage, k, pw)
    assert np.array_equal(np.sort(hits, order=order), np.sort(want_hits, order=order))
    local = {int(g): i for i, g in enumerate(ids)}
    lines = findstart.seed_lines(hits, lambda g: payload["strs"][local[g]], words, mpos, k)
    assert lines == F.find_start(faa, payload["strs"], k)
    assert len(lines) > (50 if k == 45 else 25)
    return lines


@BOTH_MODES
@pytest.mark.parametrize("k", [45, 72])
def test_findstart_reversed_storage(far, payload, alone, k):
    lines = check_findstart(far, payload, alone, far["rd"], True, k)
    if k == 45:
        assert lines == sorted(l.rstrip("\n") for l in open(os.path.join(payload["toy"], "44_rplB_starting_kmers.txt")) if l.strip())


@STRADDLE
def test_findstart_forward_storage(far, payload, alone):
    """the reads stored as sequenced: a layout of its own, the same read numbers"""
    rd, ids, n_reads, _ = upload(far["ctx"], [r[::-1] for r in payload["reads"]], "straddle")
    try:
        assert np.array_equal(ids, far["ids"]) and n_reads == far["n_reads"]
        for k in (45, 72):
            check_findstart(far, payload, alone, rd, False, k)
    finally:
        rd.free()


# ---- the stages that look the reads' windows up in a graph ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def far_graph(far, payload):
    from megagta_amd import api
    g = api.Graph(far["ctx"], payload["edges"])
    yield g
    g.free()


@STRADDLE
def test_match_contigs(far, far_graph, payload):
    want, n_marked = MR.brute_force_hits(payload["strs"], payload["seqs"], K)
    n1, n2 = payload["n1"], payload["n2"]
    assert all((want[a:b] > 0).any() and (want[a:b] == 0).any() for a, b in ((0, n1), (n1, n2), (n2, payload["n"])))      # matches in every block
    assert all(want[r] > 50 for r in payload["at_marks"])               # the reads across the marks and the first one of B3 among them
    full = far_graph.match_reads(far["rd"], payload["seqs"], counts=True)
    fast = far_graph.match_reads(far["rd"], payload["seqs"])
    ids = far["ids"]
    hits = np.zeros(far["n_reads"], dtype=np.uint32)
    hits[ids] = want
    assert np.array_equal(full["hit_windows"], hits)
    for res in (full, fast):
        assert np.array_equal(np.flatnonzero(res["bits"]), ids[want > 0])
        st = res["stats"]
        assert st["n_matched_reads"] == int((want > 0).sum()) and st["n_reads"] == far["n_reads"]
        assert st["n_read_windows"] == payload["n"] * (150 - K) and st["n_marked_edges"] == n_marked


@STRADDLE
def test_sample_coverage(far, far_graph, payload):
    """library 0 is the first filler run, the filler between B1 and B2 a library of its own between the payload's"""
    ids, n, n1, n2 = far["ids"], payload["n"], payload["n1"], payload["n2"]
    local = [1, 1, 701, n1, n1 + 337, n2 + 1, n]                          # a one-read library, an empty one, ends inside every block and across B2 | B3
    want = SC.restate(payload["strs"], local, payload["seqs"], K)
    assert sum(want["lib_hit_windows"]) > 0 and all(h > 0 for j, h in enumerate(want["lib_hit_windows"]) if j not in (0, 1))
    assert any(r["n_covered"] for r in want["rows"]) and max(want["per_window_share"]) >= 1
    ends = [int(ids[0])] + [int(ids[e - 1]) + 1 for e in local[:4]] + [int(ids[n1])] + [int(ids[e - 1]) + 1 for e in local[4:]]
    assert ends == sorted(ends) and ends[-1] == far["n_reads"]
    payload_cols, filler_cols = [1, 2, 3, 4, 6, 7, 8], [0, 5]
    res = far_graph.contig_sample_coverage(far["rd"], ends, payload["seqs"], per_window=True)
    for key in ("mass", "per_window_count"):
        assert not res[key][:, filler_cols].any(), key
    assert not res["lib_hit_windows"][filler_cols].any()
    SC.check_result(dict(res, mass=res["mass"][:, payload_cols], per_window_count=res["per_window_count"][:, payload_cols],
                         lib_hit_windows=res["lib_hit_windows"][payload_cols]), want)


@pytest.fixture(scope="module")
def placed(alone, payload):
    """pileup(per_read=True) of the payload alone, against the restatement: the placements `phase` is given, and its sites"""
    want = PL.restate(payload["strs"], payload["seqs"], K, PL.read_windows(payload["strs"], K))
    res = alone["g"].pileup(alone["rd"], payload["seqs"], per_read=True)
    PL.check_result(res, want, "the payload alone")
    return dict(want=want, res=res)


@STRADDLE
def test_pileup(far, far_graph, payload, placed):
    want = placed["want"]
    n1, n2 = payload["n1"], payload["n2"]
    got_placed = np.array([r["n_placed"] for r in want["reads"]])
    assert all((got_placed[a:b] > 0).any() for a, b in ((0, n1), (n1, n2), (n2, payload["n"])))           # reads placed in every block
    assert any(r["n_mismatch"] for r in want["reads"]) and all(got_placed[r] == 1 for r in payload["at_marks"])
    res = far_graph.pileup(far["rd"], payload["seqs"], per_read=False)
    assert res["reads"] is None
    PL.check_result(res, dict(want, stats=dict(want["stats"], n_reads=far["n_reads"])), "behind the marks")


@STRADDLE
def test_phase(far, payload, placed):
    """the payload as two paired libraries (B1; B2 and B3) behind and around unpaired filler libraries whose reads are not placed"""
    ids, n, n1 = far["ids"], payload["n"], payload["n1"]
    place = placed["res"]["reads"]
    counts, off = placed["res"]["counts"], placed["res"]["offsets"]
    # sites: the positions where the placed reads show two letters or more
    sites = [np.flatnonzero((counts[int(off[i]):int(off[i + 1])] > 0).sum(axis=1) >= 2) for i in range(len(payload["seqs"]))]
    assert sum(s.size for s in sites) >= 1 and int((place["n_placed"] == 1).sum()) >= 1
    lens = [len(s) for s in payload["seqs"]]
    for i in range(N_CONTIGS, len(sites)):                                 # the pieces of the reads at the marks: sites along them, variant or not
        sites[i] = np.union1d(sites[i], [3, lens[i] // 2, lens[i] - 2])
    assert all(place["n_placed"][r] == 1 and place["contig"][r] >= N_CONTIGS for r in payload["at_marks"])
    tuples = [(int(r["contig"]), int(r["diag"]), int(r["orient"]), int(r["n_placed"])) for r in place]
    want = PH.restate(payload["strs"], tuples, [(n1, True), (n, True)], lens, [s.tolist() for s in sites])
    assert want["stats"]["n_fragments"] > 0 and want["stats"]["n_alleles"] > 0 and int((want["site_counts"] > 0).sum(axis=1).max()) >= 2
    everyone = np.zeros(far["n_reads"], dtype=place.dtype)                # filler reads: zero records, n_placed = 0
    everyone[ids] = place
    libs = [(int(ids[0]), False), (int(ids[n1 - 1]) + 1, True), (int(ids[n1]), False), (far["n_reads"], True)]
    res = far["ctx"].phase(far["rd"], everyone, libs, lens, sites)
    PH.check_result(res, dict(want, stats=dict(want["stats"], n_reads=far["n_reads"])), "behind the marks")
