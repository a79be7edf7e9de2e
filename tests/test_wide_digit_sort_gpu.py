"""Global sort passes on digits wider than 8 bits (MGTA_SORT_WIDE): 9-bit scatters and censuses, 16-bit side entries from the scatter
and from the fused key writer.  Every case compares the whole stream with the CPU oracle's (the two largest inputs with the same build
under MGTA_SORT_WIDE=0, see there) and reads off stats["n_wide_passes"] / stats["n_sort_launches"] that the wide kernels really ran:
MGTA_SORT_WIDE=2 makes every global pass but the first one of a sort 9 bits wide, so that inputs of a few million keys take them."""
import numpy as np
import pytest

from megagta_amd import readlib, synth

pytestmark = pytest.mark.gpu

TILE, SUB_TILE = 32768, 4096                                                # keys per workgroup and per LDS stage of the radix scatter


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
    """roughly what a pass of n_items holds on the device: two key buffers, census, outputs, side entries of two bytes, slack.  Only a
    starting point for _build_in_ranges, which looks at the number of passes a limit really gives"""
    key_bytes = max(4 * ((2 * k + 4 + 31) // 32), 12)
    return 2 * (n_items * key_bytes + 4096) + (n_items + 32767) // 32768 * 4096 + 4 * n_items + (8 << 20)


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


def _build(packed_start, k, **kw):
    from megagta_amd import api
    c = api.Context(0)
    try:
        return c.build_sdbg(c.upload_reads(*packed_start), k, **kw)
    finally:
        c.close()


@pytest.fixture(scope="module")
def plain_reads():
    mg = synth.make_metagenome(20_000, 150, (("rplB", 60),), seed=91)
    return synth.pack_reads_for_build(mg.reads)


@pytest.fixture(scope="module")
def plain_oracle(oracle, plain_reads):
    return oracle.Stream.build(*plain_reads, 44, threads=4).edges()


def _skewed_reads(k, scale):
    """the input of test_fused_first_pass_gpu.test_skewed_digits (scale = 1): highly redundant reads and a poly-A block"""
    rng = np.random.default_rng(7 + k)
    reads = []
    for i in range(40 * scale):
        r = rng.integers(0, 4, 120).astype(np.uint8)
        reads += [r.copy() for _ in range(int(rng.integers(2, 400)))]
    for i in range(3000):
        reads.append(rng.integers(0, 4, int(rng.integers(k + 1, 140))).astype(np.uint8))
    reads += [np.zeros(150, np.uint8) for _ in range(300)]
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def test_one_wide_pass_whole(monkeypatch, plain_reads, plain_oracle):
    """20 000 x 150 bp, k = 44 (W = 3), ~4 M items in one pass over every bucket: 8 + 9 bits.  The tiled key writer leaves the census of
    the 8-bit pass, whose scatter writes 16-bit side entries; the 9-bit census reads them (checked against the keys: MGTA_SORT_SIDE=2)"""
    monkeypatch.setenv("MGTA_SORT_WIDE", "2")
    monkeypatch.setenv("MGTA_SORT_SIDE", "2")
    g = _build(plain_reads, 44)
    _same(g, plain_oracle)
    st = g.stats
    assert st["n_items"] > 3_000_000 and st["n_passes"] == 1
    assert st["n_sort_launches"] == 2 and st["n_wide_passes"] == 1, st


@pytest.mark.parametrize("bias", ["0", None, "2"])
def test_one_wide_pass_in_ranges(monkeypatch, plain_reads, plain_oracle, bias):
    """the same under a memory limit that gives 3-4 bucket ranges: the fused key writer does every range's 8-bit pass and leaves
    16-bit side entries for the 9-bit one (its output checked on the device: MGTA_SORT_FUSED=2); bias = 2: digits below the leading
    bit a range's keys share"""
    from megagta_amd import api
    monkeypatch.setenv("MGTA_SORT_WIDE", "2")
    monkeypatch.setenv("MGTA_SORT_SIDE", "2")
    monkeypatch.setenv("MGTA_SORT_FUSED", "2")
    if bias is not None:
        monkeypatch.setenv("MGTA_SORT_BIAS", bias)
    packed, start = plain_reads
    c = api.Context(0)
    try:
        rd = c.upload_reads(packed, start)
        whole = c.build_sdbg(rd, 44)
        assert whole.stats["n_passes"] == 1
        g = _build_in_ranges(c, rd, 44, whole.stats["n_items"], start.size - 1, packed.nbytes + start.nbytes + (1 << 16), (3, 4))
    finally:
        c.close()
    _same(g, plain_oracle)
    st = g.stats
    assert st["n_fused_passes"] == st["n_passes"], st                        # every range: the writer placed the keys and wrote the 16-bit entries
    assert st["n_wide_passes"] == st["n_passes"] and st["n_sort_launches"] == st["n_passes"], st   # one scatter left per range, the wide one


def test_default_takes_no_wide_digit_where_none_saves_a_pass(monkeypatch, plain_reads, plain_oracle):
    """MGTA_SORT_WIDE unset: two 8-bit passes, as with MGTA_SORT_WIDE=0 (8 + 9 bits would save nothing)"""
    monkeypatch.delenv("MGTA_SORT_WIDE", raising=False)
    g = _build(plain_reads, 44)
    monkeypatch.setenv("MGTA_SORT_WIDE", "0")
    g0 = _build(plain_reads, 44)
    _same(g, plain_oracle)
    _same(g0, plain_oracle)
    assert g.stats["n_wide_passes"] == 0 and g0.stats["n_wide_passes"] == 0
    assert g.stats["n_sort_launches"] == g0.stats["n_sort_launches"] == 2


def test_bucket_sub_range(monkeypatch, plain_reads, plain_oracle):
    """the buckets [12345, 42346), MGTA_SORT_BIAS=2: one skipped leading bit and a bias under the wide digit"""
    monkeypatch.setenv("MGTA_SORT_WIDE", "2")
    monkeypatch.setenv("MGTA_SORT_BIAS", "2")
    monkeypatch.setenv("MGTA_SORT_SIDE", "2")
    g = _build(plain_reads, 44, bucket_range=(12345, 42346))
    _same_slice(g, plain_oracle, 12345, 42346)
    assert g.stats["n_sort_launches"] == 2 and g.stats["n_wide_passes"] == 1, g.stats


def test_odd_item_count(monkeypatch, plain_reads, plain_oracle):
    """an odd number of keys (a whole build always has an even one): the scalar tail of the 16-bit side census and runs of side entries
    that start at odd offsets.  The first of a few bucket ranges that holds an odd number of items (biased digits: MGTA_SORT_BIAS=2)"""
    from megagta_amd import api
    monkeypatch.setenv("MGTA_SORT_WIDE", "2")
    monkeypatch.setenv("MGTA_SORT_BIAS", "2")
    monkeypatch.setenv("MGTA_SORT_SIDE", "2")
    c = api.Context(0)
    try:
        rd = c.upload_reads(*plain_reads)
        for b1 in range(30000, 30016):
            g = c.build_sdbg(rd, 44, bucket_range=(0, b1))
            _same_slice(g, plain_oracle, 0, b1)
            assert g.stats["n_sort_launches"] == 2 and g.stats["n_wide_passes"] == 1, g.stats
            if g.stats["n_items"] % 2 == 1:
                return
    finally:
        c.close()
    raise AssertionError("no bucket range with an odd number of items")


@pytest.mark.parametrize("last_tile", [TILE - 2, TILE, TILE + 2, SUB_TILE - 2, SUB_TILE, SUB_TILE + 2])
def test_tile_edges(monkeypatch, oracle, last_tile):
    """a sort of 65536 keys or fewer takes a single (8-bit) global pass, so the edges are those of the third tile: two full tiles and a
    last one just below, at and just above a whole tile (then a fourth of two keys) and one 4096-key sub-tile.  A read of length L
    brings 2 (L - k) + 4 items"""
    k = 44
    n = 2 * TILE + last_tile
    rng = np.random.default_rng(n)
    lens, left = [], n
    while left:
        items = min(left, 2 * 106 + 4)                                        # 150 bp
        if 0 < left - items < 6:                                              # the last read needs L >= k + 1: 6 items at least
            items -= 6
        lens.append((items - 4) // 2 + k)
        left -= items
    reads = [rng.integers(0, 4, L).astype(np.uint8) for L in lens]
    ps = readlib.pack_for_build(reads)
    monkeypatch.setenv("MGTA_SORT_WIDE", "2")
    monkeypatch.setenv("MGTA_SORT_SIDE", "2")
    g = _build(ps, k)
    assert g.stats["n_items"] == n
    _same(g, oracle.Stream.build(*ps, k, threads=4).edges())
    assert g.stats["n_sort_launches"] == 2 and g.stats["n_wide_passes"] == 1, g.stats


def test_skew_and_stability(monkeypatch, oracle):
    """redundant reads and a poly-A block: one digit value takes most of a tile, and the many equal keys must keep the order the first
    pass left them in through the stable 9-bit pass"""
    k = 44
    ps = readlib.pack_for_build(_skewed_reads(k, 1))
    monkeypatch.setenv("MGTA_SORT_WIDE", "2")
    monkeypatch.setenv("MGTA_SORT_SIDE", "2")
    g = _build(ps, k)
    _same(g, oracle.Stream.build(*ps, k, threads=4).edges())
    assert g.stats["n_sort_launches"] == 2 and g.stats["n_wide_passes"] == 1, g.stats


def _against_narrow(monkeypatch, ps, k, side):
    """8 + 9 + 9 bits against the same build under MGTA_SORT_WIDE=0.  That route is the code from before the wide digits, which the
    existing tests hold against the oracle; the oracle itself needs far more than a few seconds for 17 M items and more"""
    monkeypatch.setenv("MGTA_SORT_WIDE", "0")
    ref = _build(ps, k)
    assert ref.stats["n_wide_passes"] == 0 and ref.stats["n_sort_launches"] == 3 and ref.stats["n_items"] > 16_800_000, ref.stats
    monkeypatch.setenv("MGTA_SORT_WIDE", "2")
    if side is not None:
        monkeypatch.setenv("MGTA_SORT_SIDE", side)
    g = _build(ps, k)
    _same(g, ref)
    assert g.stats["n_items"] == ref.stats["n_items"]
    assert g.stats["n_sort_launches"] == 3 and g.stats["n_wide_passes"] == 2, g.stats


@pytest.fixture(scope="module")
def many_reads():
    mg = synth.make_metagenome(100_000, 150, (("rplB", 60),), seed=92)
    return synth.pack_reads_for_build(mg.reads)


@pytest.mark.parametrize("side", [None, "2", "0"])
def test_two_wide_passes_back_to_back(monkeypatch, many_reads, side):
    """100 000 x 150 bp, k = 44: more than 16.8 M items, three global passes, 8 + 9 + 9 bits: the census of the third reads the 16-bit
    entries the second (wide) scatter wrote (side = 2: every side census checked against the keys; 0: every census from the keys).
    Compared with the build under MGTA_SORT_WIDE=0, see _against_narrow"""
    _against_narrow(monkeypatch, many_reads, 44, side)


def test_skew_through_two_wide_passes(monkeypatch):
    """the skewed input with fourteen times the redundant reads (more than 16.8 M items): equal keys through two stable wide passes.
    Compared with the build under MGTA_SORT_WIDE=0, see _against_narrow"""
    _against_narrow(monkeypatch, readlib.pack_for_build(_skewed_reads(44, 14)), 44, "2")


def test_two_key_words_take_wide_digits(monkeypatch, oracle):
    """W = 2 (k = 29)"""
    mg = synth.make_metagenome(12_000, 100, (("rplB", 60),), seed=29)
    ps = synth.pack_reads_for_build(mg.reads)
    monkeypatch.setenv("MGTA_SORT_WIDE", "2")
    monkeypatch.setenv("MGTA_SORT_SIDE", "2")
    g = _build(ps, 29)
    _same(g, oracle.Stream.build(*ps, 29, threads=4).edges())
    assert g.stats["words_per_key"] == 2 and g.stats["n_sort_launches"] == 2 and g.stats["n_wide_passes"] == 1, g.stats


def test_four_key_words_keep_narrow_digits(monkeypatch, oracle):
    """W = 4 (k = 60): the wide scatter with its side entries does not fit the LDS next to 4096 keys of four words"""
    mg = synth.make_metagenome(12_000, 150, (("rplB", 60),), seed=60)
    ps = synth.pack_reads_for_build(mg.reads)
    monkeypatch.setenv("MGTA_SORT_WIDE", "2")
    g = _build(ps, 60)
    _same(g, oracle.Stream.build(*ps, 60, threads=4).edges())
    assert g.stats["words_per_key"] == 4 and g.stats["n_sort_launches"] == 2 and g.stats["n_wide_passes"] == 0, g.stats


def test_min_count_two_keeps_narrow_digits(monkeypatch, oracle):
    """-m 2 at k = 60: stage 1 sorts records of W + 2 = 6 words, stage 2 keys of 4: neither takes wide digits"""
    k = 60
    rng = np.random.default_rng(260)
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
    ps = readlib.pack_for_build(reads)
    monkeypatch.setenv("MGTA_SORT_WIDE", "2")
    g = _build(ps, k, min_count=2, need_mercy=True)
    _same(g, oracle.Stream.build_solid(*ps, k, 2, True, threads=4).edges())
    assert g.stats["n_sort_launches"] >= 1 and g.stats["n_wide_passes"] == 0, g.stats
