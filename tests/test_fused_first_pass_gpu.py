"""The key writer of a bucket-range pass that does the first global sort pass on the way (MGTA_SORT_FUSED): every case builds under a
memory limit that splits the buckets into 2..8 ranges and compares the stream of the fused build (with MGTA_SORT_FUSED=2: the
writer's output is checked on the device) with the CPU oracle's and with the same build under MGTA_SORT_FUSED=0.  Which route ran is
read off stats["n_passes"] / stats["n_fused_passes"], so no case passes by falling back -- but the one that is about the fall-back."""
import numpy as np
import pytest

from megagta_amd import readlib, synth

pytestmark = pytest.mark.gpu


def _same(gpu, orc):
    assert gpu.k == orc.k and gpu.words_per_tip == orc.words_per_tip
    assert np.array_equal(gpu.bucket_items, orc.bucket_items)
    assert np.array_equal(gpu.records, orc.records)
    assert np.array_equal(gpu.large, orc.large)
    assert np.array_equal(gpu.tips, orc.tips)
    assert gpu.md5() == orc.md5()


def _same_slice(gpu, orc, b0, b1):
    """a build of the buckets [b0, b1) against that slice of the oracle's whole stream"""
    lo, hi = int(orc.bucket_items[:b0].sum()), int(orc.bucket_items[:b1].sum())
    assert np.array_equal(gpu.records, orc.records[lo:hi])
    assert np.array_equal(gpu.bucket_items[b0:b1], orc.bucket_items[b0:b1]) and gpu.bucket_items.sum() == hi - lo


def _pass_bytes(n_items, k):
    """roughly what a pass of n_items holds on the device: two key buffers, census, outputs, side digits, slack.  Only a starting point
    for _build_in_ranges, which looks at the number of passes a limit really gives: no case depends on the figure being exact"""
    key_bytes = max(4 * ((2 * k + 4 + 31) // 32), 12)
    return 2 * (n_items * key_bytes + 4096) + (n_items + 32767) // 32768 * 2048 + 3 * n_items + (8 << 20)


def _build_in_ranges(c, rd, k, n_items, n_reads, other, want, **kw):
    """the first build under a memory limit that takes one of the `want`ed numbers of passes.  The limit for R ranges holds a pass of
    1.25 times a range's share of the items, the table of the counted digits and the planner's eighth of headroom; the 8 MB of slack in
    every pass weigh so much at these sizes that the planner may still settle on another number, hence a few targets in turn"""
    seen = []
    for ranges in (3, 4, 5, 6, 2):
        table = ranges * 256 * 8 * -(-n_reads // 64) * 9 // 8
        c.set_mem_limit(int((_pass_bytes(int(n_items * 1.25 / ranges), k) + table) * 9 / 8 * 1.05) + other)
        g = c.build_sdbg(rd, k, **kw)
        seen.append(g.stats["n_passes"])
        if g.stats["n_passes"] in want:
            return g
    raise AssertionError(f"no memory limit gave {tuple(want)} passes: {seen}")


def _check(monkeypatch, oracle, reads, k, want=range(2, 9), fused="all", min_count=1, mercy=False, bucket_range=None, packed_start=None):
    """oracle == fused build (checked on the device) == plain build, all under one memory limit; returns the fused build's stats"""
    from megagta_amd import api
    packed, start = packed_start if packed_start is not None else readlib.pack_for_build(reads)
    if min_count > 1:
        o = oracle.Stream.build_solid(packed, start, k, min_count, mercy, threads=4).edges()
    else:
        o = oracle.Stream.build(packed, start, k, threads=4).edges()
    kw = dict(min_count=min_count, need_mercy=mercy) if min_count > 1 else {}
    if bucket_range is not None:
        kw["bucket_range"] = bucket_range
    c = api.Context(0)
    try:
        rd = c.upload_reads(packed, start)
        monkeypatch.setenv("MGTA_SORT_FUSED", "2")
        whole = c.build_sdbg(rd, k, **kw)                                   # one pass: nothing counted ahead, nothing fused
        assert whole.stats["n_passes"] == 1 and whole.stats["n_fused_passes"] == 0
        g = _build_in_ranges(c, rd, k, whole.stats["n_items"], start.size - 1, packed.nbytes + start.nbytes + (1 << 16), want, **kw)
        limit_passes = g.stats["n_passes"]
        monkeypatch.setenv("MGTA_SORT_FUSED", "0")
        plain = c.build_sdbg(rd, k, **kw)                                   # (the limit of the fused build still holds)
        assert plain.stats["n_fused_passes"] == 0 and plain.stats["n_passes"] == limit_passes
    finally:
        monkeypatch.delenv("MGTA_SORT_FUSED")
        c.close()
    for b in (g, plain, whole):
        if bucket_range is None:
            _same(b, o)
        else:
            _same_slice(b, o, *bucket_range)
    assert g.stats["n_items"] == plain.stats["n_items"] == whole.stats["n_items"]
    if fused == "all":
        assert g.stats["n_fused_passes"] == g.stats["n_passes"], g.stats
    elif fused == "some":
        assert 1 <= g.stats["n_fused_passes"] <= g.stats["n_passes"], g.stats
    else:                                                                   # the fall-back: some range took the plain route
        assert 0 <= g.stats["n_fused_passes"] < g.stats["n_passes"], g.stats
    # a fused pass launches no scatter for its first digit
    assert g.stats["n_sort_launches"] == plain.stats["n_sort_launches"] - g.stats["n_fused_passes"]
    return g.stats, o


@pytest.fixture(scope="module")
def plain_reads():
    mg = synth.make_metagenome(20_000, 150, (("rplB", 60),), seed=91)
    return synth.pack_reads_for_build(mg.reads)


@pytest.mark.parametrize("bias", ["0", None, "2"])
def test_plain_three_or_four_ranges(monkeypatch, oracle, plain_reads, bias):
    """20 000 reads of 150 bp at k = 44 (W = 3): ~4 M items in 3-4 ranges, two global passes each (side digits in play); the digit the
    writer places by moves with the leading bits a range's keys share (MGTA_SORT_BIAS)"""
    if bias is not None:
        monkeypatch.setenv("MGTA_SORT_BIAS", bias)
    st, _ = _check(monkeypatch, oracle, None, 44, want=(3, 4), packed_start=plain_reads)
    assert st["n_items"] > 3_000_000
    assert st["n_sort_launches"] >= st["n_passes"]                          # P >= 2: a scatter was left to every range


@pytest.mark.parametrize("k,L", [(29, 100), (60, 150), (95, 250), (127, 250)])
def test_key_widths(monkeypatch, oracle, k, L):
    """W = 2, 4, 7, 9 key words (W = 9: no side digits, the tile's bytes do not fit the LDS next to the staged keys)"""
    mg = synth.make_metagenome(12_000, L, (("rplB", 60),), seed=k)
    _check(monkeypatch, oracle, None, k, packed_start=synth.pack_reads_for_build(mg.reads))


@pytest.mark.parametrize("n_reads", [63, 64, 65, 1000])
def test_ragged_reads_and_partial_workgroups(monkeypatch, oracle, n_reads):
    """reads shorter than k + 1, of exactly k + 1, of 150 bases and one far longer than 4096 + k (a read at a time; it also carries
    the items a memory limit needs to split the buckets), in a last workgroup of 63, 64, 1 and 40 reads"""
    k = 44
    rng = np.random.default_rng(n_reads)
    reads = []
    for i in range(n_reads - 1):
        L = (k - 5, k, k + 1, 150, int(rng.integers(k + 1, 200)))[i % 5]
        reads.append(rng.integers(0, 4, L).astype(np.uint8))
    reads.insert(int(rng.integers(0, n_reads - 1)), rng.integers(0, 4, 600_000).astype(np.uint8))
    _check(monkeypatch, oracle, reads, k)


def test_staging_overflow(monkeypatch, oracle):
    """70 reads of ~9 000 bases at k = 31: a workgroup of 64 reads holds several batches of the writer's LDS stage per range"""
    rng = np.random.default_rng(31)
    reads = [rng.integers(0, 4, int(rng.integers(8800, 9200))).astype(np.uint8) for _ in range(70)]
    st, _ = _check(monkeypatch, oracle, reads, 31)
    assert st["n_items"] / st["n_passes"] / 2 > 4 * 8192                    # per range and workgroup: more than four stages of any width


def test_skewed_digits(monkeypatch, oracle):
    """highly redundant reads and a poly-A block: one digit value takes most keys of a row and of a whole pass.  The copies crowd into
    the ranges of their own buckets, so a range's items are not its share of the buckets and some range may get another plan than
    the estimated one and fall back: at least one range must be fused, not every one"""
    k = 44
    rng = np.random.default_rng(7 + k)
    reads = []
    for i in range(40):
        r = rng.integers(0, 4, 120).astype(np.uint8)
        reads += [r.copy() for _ in range(int(rng.integers(2, 400)))]
    for i in range(3000):
        reads.append(rng.integers(0, 4, int(rng.integers(k + 1, 140))).astype(np.uint8))
    reads += [np.zeros(150, np.uint8) for _ in range(300)]
    order = rng.permutation(len(reads))
    _check(monkeypatch, oracle, [reads[i] for i in order], k, fused="some")


def test_min_count_two_with_mercy(monkeypatch, oracle):
    """-m 2 with mercy edges: both scans take the solid runs of stage 1 (a read at a time).  Stage 1 drops what it sees once, unevenly
    over the buckets, so as in the skewed case a range may fall back: at least one must be fused"""
    k = 31
    rng = np.random.default_rng(231)
    genome = rng.integers(0, 4, 60_000).astype(np.uint8)
    reads = []
    for _ in range(9000):
        L = int(rng.integers(k - 2, 200))
        p = int(rng.integers(0, genome.size - L))
        r = genome[p:p + L].copy()
        err = rng.random(L) < 0.01
        r[err] = (r[err] + rng.integers(1, 4, int(err.sum()))) & 3
        if rng.random() < 0.5:
            r = (3 - r[::-1]).astype(np.uint8)
        reads.append(r)
    _check(monkeypatch, oracle, reads, k, min_count=2, mercy=True, fused="some")


def test_bucket_sub_range_under_a_limit(monkeypatch, oracle, plain_reads):
    """the share of one GPU of several, itself split into ranges: biased digits and a scan that starts at the share's first bucket"""
    _check(monkeypatch, oracle, None, 44, bucket_range=(12345, 42346), packed_start=plain_reads)


def test_fall_back_when_the_estimated_plan_is_not_the_real_one(monkeypatch, oracle):
    """reads over the letters A and C only, and a little random sequence: their keys start with A or C (the lowest third of the
    buckets), those of the other strand with G or T (the highest), and the ranges between hold so few that their sort takes fewer
    global passes than their share of the buckets suggested -- those take the plain route, and the stream is the same"""
    k = 44
    rng = np.random.default_rng(3)
    reads = [rng.integers(0, 2, 150).astype(np.uint8) for _ in range(5000)] + [rng.integers(0, 4, 150).astype(np.uint8) for _ in range(40)]
    order = rng.permutation(len(reads))
    st, o = _check(monkeypatch, oracle, [reads[i] for i in order], k, want=(3, 5, 6, 7, 8), fused="fall-back")
    width = -(-65536 // st["n_passes"])
    per_range = [int(o.bucket_items[b:b + width].sum()) for b in range(0, 65536, width)]
    assert max(per_range) > 50 * min(per_range), per_range                  # (edges per range: the sort items follow them)
