"""Every stage that indexes the packed reads by start[r], on reads whose base offsets lie around and beyond 2^31 and 2^32.

The toy golden library (6000 reads of 150 bp, its k = 44 graph pinned to the reference binary's files) sits behind about 97.6 M filler
reads of 44 bases (helpers.reads_behind_marks; the layout itself is checked by test_far_offsets_host.py).  A filler read holds no
window of any stage and no stretch of 20 residues in any frame, so every stage must give exactly what it gives for the payload alone,
read numbers mapped through `ids`.  An offset narrowed to 32 or 31 bits still lies inside the array: there the filler holds random bits
(the decoys), so a wrapped read yields foreign k-mers and foreign residues.  Every expectation comes from the payload alone: the oracle,
the goldens, the Python restatements of the stage tests and the device on the payload uploaded without filler.  One upload per mode
serves all stages.

The stages: the build (-m 1, and -m 2 with mercy edges), findstart (both storage orders), match_reads, contig_sample_coverage, pileup,
gapped pileup, phase, and recruit (global mode in both layouts and both storage orders, local mode).  COVERED names the tests of every
entry point of include/megagta_hip.h that takes the reads; test_far_offsets_host.py fails when the header gains one that is not named
here."""
import os

import numpy as np
import pytest

from megagta_amd import hmm as HM
from megagta_amd import readlib
from tests import helpers as H
from tests import recruit_local_ref as LREF
from tests import recruit_ref as REF
from tests import test_gapped_gpu as GP
from tests import test_matchreads_gpu as MR
from tests import test_phase_gpu as PH
from tests import test_pileup_gpu as PL
from tests import test_recruit_gpu as RC
from tests import test_samplecov_gpu as SC

pytestmark = pytest.mark.gpu

K = 44
FILL_LEN = 44                                  # <= k for the build at k = 44, < k for findstart at 45 and 72, < k + 1 for the window stages
SEED = 7
N_CONTIGS = 24

# every function of include/megagta_hip.h that takes a `const mgta_reads *`, and the tests of this module that run it behind the marks
# (tests/test_far_offsets_host.py holds the two tables against the header)
COVERED = {
    "mgta_sdbg_build_resident": ["test_build_m1", "test_build_m2_mercy"],
    "mgta_findstart": ["test_findstart_reversed_storage", "test_findstart_forward_storage"],
    "mgta_reads_match_contigs": ["test_match_contigs"],
    "mgta_contig_sample_coverage": ["test_sample_coverage"],
    "mgta_reads_pileup": ["test_pileup"],
    "mgta_reads_pileup_gapped": ["test_pileup_gapped"],
    "mgta_reads_phase": ["test_phase"],
    "mgta_reads_recruit": ["test_recruit_global", "test_recruit_local", "test_findstart_forward_storage"],
}
# ... and those that take the reads and never index bases by start[r], each with the reason (none today)
NOT_READ = {}


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
def test_findstart_forward_storage(far, far_model, payload, alone, recruited):
    """the reads stored as sequenced: a layout of its own, the same read numbers.  Global recruit reads the same upload with
    reads_reversed = False: the reads it translates are the payload's, so the expectation is the one of test_recruit_global"""
    rd, ids, n_reads, _ = upload(far["ctx"], [r[::-1] for r in payload["reads"]], "straddle")
    try:
        assert np.array_equal(ids, far["ids"]) and n_reads == far["n_reads"]
        for k in (45, 72):
            check_findstart(far, payload, alone, rd, False, k)
        check_far_recruit(far, far_model, rd, recruited, GLOBAL_PARAMS, reads_reversed=False)
    finally:
        rd.free()


# ---- recruit --------------------------------------------------------------------------------------------------------------------------
# min_aa is the default; the thresholds are test inputs.  At the default of 20 bits only the read across 2^31 of the three reads at the
# marks is recruited (the other two score -9.9 and -5.8 nats in global mode, 6.7 and 10.6 in local mode), so each mode gets a threshold
# just below its lowest of the three: all three are then recruited, and in every block reads with a score stay below it.
GLOBAL_PARAMS = dict(min_aa=20, min_score=-10.0)
LOCAL_PARAMS = dict(min_aa=20, min_score=6.0, local=True)


@pytest.fixture(scope="module")
def gene_model(payload):
    return HM.parse_hmm(os.path.join(payload["toy"], "for_enone.hmm"))


@pytest.fixture(scope="module")
def alone_model(alone, gene_model):
    from megagta_amd import api
    dev = api.DeviceHmm(alone["ctx"], gene_model)
    yield dev
    dev.free()


@pytest.fixture(scope="module")
def far_model(far, gene_model):
    from megagta_amd import api
    dev = api.DeviceHmm(far["ctx"], gene_model)
    yield dev
    dev.free()


def recruit_preconditions(ref, want, payload, min_aa):
    """on the expectation alone: a filler read is unscored, reads are recruited (and scored reads are not) in every block, the three
    reads at the marks are recruited, in frames of both strands"""
    for n in (FILL_LEN, FILL_LEN - 1, 1):                                 # poly-A: 14 K (or F) in every frame, no stop and no 20 residues
        assert ref.stretches([np.zeros(n, dtype=np.uint8)], min_aa) == [], n
    assert REF.frames(np.zeros(FILL_LEN, dtype=np.uint8)) == ["K" * 14] * 3 + ["F" * 14] * 3
    bits, recs = want["bits"], want["recs"]
    for a, b in ((0, payload["n1"]), (payload["n1"], payload["n2"]), (payload["n2"], payload["n"])):
        assert bits[a:b].sum() >= 10 and sum(r["status"] == 0 and not h for r, h in zip(recs[a:b], bits[a:b])) >= 10, (a, b)
    assert all(bits[r] for r in payload["at_marks"])
    frames = {recs[i]["frame"] for i in np.flatnonzero(bits)}
    assert len(frames) >= 2 and max(frames) >= 3 and min(frames) < 3
    assert int(want["col_depth"].max()) >= 2 and want["stats"]["n_unscored"] < payload["n"] // 2


@pytest.fixture(scope="module")
def recruited(payload, alone, alone_model, gene_model):
    """global mode on the payload alone.  Yardstick (b) of tests/recruit_ref.py on every read: translation, stretch and frame choice in
    Python around Context.align of the `alone` context (the plain yardstick (a) takes 7 s on the 29 828 stretches of the 6000 reads);
    yardstick (a) on about 50 reads, the three at the marks among them.  The device on the payload alone equals it on every record."""
    reads, p = payload["reads"], GLOBAL_PARAMS
    want = REF.recruit(gene_model, reads, p["min_aa"], p["min_score"], scorer=RC.align_scorer(alone["ctx"], alone_model))
    recruit_preconditions(REF, want, payload, p["min_aa"])
    low = [i for i, w in enumerate(want["recs"]) if w["status"] == 0 and not want["bits"][i]]
    sample = sorted(set(payload["at_marks"]) | set(np.flatnonzero(want["bits"])[:20].tolist() + low[:20] + list(range(10))))
    plain = REF.recruit(gene_model, [reads[i] for i in sample], p["min_aa"], p["min_score"])
    for k, i in enumerate(sample):
        assert RC.eight(plain["recs"][k]["score"]) == RC.eight(want["recs"][i]["score"]) and plain["recs"][k] == want["recs"][i], i
        assert bool(plain["bits"][k]) == bool(want["bits"][i]), i
    got = alone["ctx"].recruit(alone_model, alone["rd"], params=p, recs=True)
    RC.assert_is(got, want, "the payload alone")
    return want


@pytest.fixture(scope="module")
def recruited_local(payload, alone, alone_model, gene_model, recruited):
    """local mode on the payload alone: tests/recruit_local_ref.py in plain Python on every read (about 10 s, once), and the device on the
    payload alone equal to it on every record.  Reads that only the local rule finds are among them: asserted here, on the CPU."""
    reads, p = payload["reads"], LOCAL_PARAMS
    want = LREF.recruit(gene_model, reads, p["min_aa"], p["min_score"])
    recruit_preconditions(LREF, want, payload, p["min_aa"])
    # the global rule at the same threshold, from the global expectation's records: reads it leaves out and the local rule takes
    glob = REF.outputs(recruited["recs"], recruited["stretches"], gene_model.M, p["min_score"])["bits"]
    only = want["bits"] & ~glob
    assert only.sum() >= 100 and not (glob & ~want["bits"]).any()
    assert all(only[a:b].any() for a, b in ((0, payload["n1"]), (payload["n1"], payload["n2"]), (payload["n2"], payload["n"])))
    assert want["recs"] != recruited["recs"]
    got = alone["ctx"].recruit(alone_model, alone["rd"], params=p, recs=True)
    RC.assert_is(got, want, "the payload alone, local")
    return want


def check_far_recruit(far, dev, rd, want, params, reads_reversed=True):
    """Context.recruit on the far layout: the bits of the payload's recruited reads at their numbers and no other bit, the payload's column
    depth and stats, every filler read unscored; then a prefix that ends on the read at the 2^31 mark"""
    ids, n = far["ids"], len(want["bits"])
    res = far["ctx"].recruit(dev, rd, params=params, recs=False, cols=True, reads_reversed=reads_reversed)
    assert res["recs"] is None                                            # (97.6 M records would be 2.3 GB for nothing)
    assert len(res["bits"]) == far["n_reads"] and np.array_equal(np.flatnonzero(res["bits"]), ids[want["bits"]])
    assert res["col_depth"].tolist() == want["col_depth"].tolist()
    st = want["stats"]
    assert {f: res["stats"][f] for f in REF.STABLE} == dict(st, n_reads=far["n_reads"], n_unscored=st["n_unscored"] + far["n_reads"] - n)
    assert list(res["stats"]["n_recruited_frame"]) == st["n_recruited_frame"] and sum(st["n_recruited_frame"]) == int(want["bits"].sum())
    return res


def check_far_recruit_prefix(far, dev, payload, want, params):
    """n_short_reads ends on the read at the 2^31 mark (across it, or the last one below it): the bits of the payload reads up to and
    including that read and nothing else"""
    ids, at = far["ids"], payload["at_marks"][0]
    n_short = int(ids[at]) + 1
    res = far["ctx"].recruit(dev, far["rd"], n_short_reads=n_short, params=params, recs=False, cols=False)
    head = want["bits"][:at + 1]
    assert head[at] and head.sum() >= 5 and want["bits"][at + 1:].any()
    assert res["recs"] is None and res["col_depth"] is None and len(res["bits"]) == n_short
    assert np.array_equal(np.flatnonzero(res["bits"]), ids[:at + 1][head])
    assert res["stats"]["n_reads"] == n_short and res["stats"]["n_recruited"] == int(head.sum())


@BOTH_MODES
def test_recruit_global(far, far_model, payload, recruited):
    check_far_recruit(far, far_model, far["rd"], recruited, GLOBAL_PARAMS)
    check_far_recruit_prefix(far, far_model, payload, recruited, GLOBAL_PARAMS)


@STRADDLE
def test_recruit_local(far, far_model, recruited_local):
    """every run of 20 residues between stops, the best placement of any substring: 2695 more stretches than the global rule scores, and
    reads that only this rule recruits (asserted in the fixture).  No prefix call here: the bound on the reads is the one code of both
    modes, and a call over the filler costs more than any other stage of this module (six frames of 97.6 M reads, half a second)"""
    check_far_recruit(far, far_model, far["rd"], recruited_local, LOCAL_PARAMS)


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


def planted_indels(pieces):
    """the three pieces of the reads at the marks, each with one indel at least k + 1 letters from either end, placed where it cannot be
    moved without a mismatch -> ([contig], [(pos on the contig, len as a gap record holds it)]): the first read lacks 3 letters of its
    contig, the second (its piece is the reverse complement) holds 2 letters that its contig lacks, the third lacks 1 letter"""
    def unlike(*letters):
        return next(c for c in "ACGT" if c not in letters)
    out, planted = [], []
    p = pieces[0]
    at = len(p) // 2
    out.append(p[:at] + unlike(p[at]) + "A" + unlike(p[at - 1]) + p[at:])
    planted.append((at, 3))
    p = pieces[1]
    at = len(p) // 2
    while p[at - 1] == p[at + 1] or p[at] == p[at + 2]:
        at += 1
    out.append(p[:at] + p[at + 2:])
    planted.append((at, -2))
    p = pieces[2]
    at = len(p) // 2
    out.append(p[:at] + unlike(p[at], p[at - 1]) + p[at:])
    planted.append((at, 1))
    for p, c, (at, ln) in zip(pieces, out, planted):
        assert len(c) == len(p) + ln and at >= K + 1 and len(c) - at - max(ln, 0) >= K + 1
    return out, planted


@pytest.fixture(scope="module")
def gapped(payload, alone):
    """the contigs of the graph and, IN PLACE of the three intact pieces of the reads at the marks, the same pieces with an indel each.
    (Next to its intact piece a read is never placed across a gap: the intact piece gives it the higher score, 130, 150 and 115 against
    123, 142 and 110 behind the gap penalty, and only the best score is placed.)  The restatement of test_gapped_gpu, its preconditions,
    and the device on the payload alone against it, so that a failure of the far run points at the offsets"""
    strs, marks = payload["strs"], payload["at_marks"]
    contigs, planted = planted_indels(payload["seqs"][N_CONTIGS:])
    seqs = payload["seqs"][:N_CONTIGS] + contigs
    want = GP.restate(strs, seqs, K, GP.read_windows(strs, K))
    for j, (r, (pos, ln)) in enumerate(zip(marks, planted)):              # one gap row per read at a mark, on its contig, where it was planted
        rows = [g for g in want["gaps"] if g["read"] == r]
        assert len(rows) == 1 and (rows[0]["contig"], rows[0]["pos"], rows[0]["len"], rows[0]["unique"]) == (N_CONTIGS + j, pos, ln, 1), (r, rows)
        assert rows[0]["orient"] == (j == 1) and want["reads"][r]["n_placed"] == 1
    n1, n2 = payload["n1"], payload["n2"]
    assert all(any(a <= g["read"] < b for g in want["gaps"]) for a, b in ((0, n1), (n1, n2), (n2, payload["n"])))
    assert any(g["read"] not in marks for g in want["gaps"])              # reads beside them cross the indels too
    ungapped = [r for r, w in enumerate(want["reads"]) if w["n_placed"] and w["diag"] == w["diag2"]]
    assert len(ungapped) > 500 and want["stats"]["n_inserted"] >= 2 and want["stats"]["n_deleted"] >= 4
    res = alone["g"].pileup_gapped(alone["rd"], seqs, per_read=True)
    GP.check_result(res, want, "the payload alone")
    return dict(seqs=seqs, want=want)


@STRADDLE
def test_pileup_gapped(far, far_graph, gapped):
    want, ids = gapped["want"], far["ids"]
    res = far_graph.pileup_gapped(far["rd"], gapped["seqs"], per_read=False)
    assert res["reads"] is None
    far_want = dict(want, reads=[], gaps=[dict(g, read=int(ids[g["read"]])) for g in want["gaps"]], stats=dict(want["stats"], n_reads=far["n_reads"]))
    GP.check_result(dict(res, reads=()), far_want, "behind the marks")    # (no per-read records were asked for: none to compare)


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
