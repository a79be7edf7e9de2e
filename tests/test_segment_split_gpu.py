"""Segments of equal sorted prefix that no LDS tile holds (longer than BigCfg::kTile keys, or LocalCfg::kTile where a key width has no
big tile): split by the highest digit below the prefix, level by level (segment_split_kernel), the pieces finished in LDS from whichever
key buffer they are in.  Every case compares the whole edge stream with the CPU oracle's and reads off stats["n_split_levels"] that
the route ran, and how deep.

The inputs are some ten thousand reads of k + 4 bases (12 sort items each), so that a sort holds between 65 537 and 16.7 M items and
its global passes sort 16 leading bits: 8 bases.  A key is a window of the reversed read or of its reverse complement (one per start
0 .. 5), so reads whose REVERSED sequence starts with one 8-base motif put one key each into the segment of that motif."""
import numpy as np
import pytest

from megagta_amd import readlib

pytestmark = pytest.mark.gpu

MOTIF = np.array([0, 1, 2, 3, 3, 1, 0, 2], np.uint8)                       # ACGTTCAG: no overlap with a shift of itself
MOTIF16 = np.concatenate([MOTIF, np.array([1, 3, 0, 2, 2, 0, 3, 1], np.uint8)])


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


def _pack(windows, rng):
    """reads whose reversed sequences are `windows` (pack_for_build reverses every read), shuffled"""
    order = rng.permutation(len(windows))
    return readlib.pack_for_build([windows[i][::-1].copy() for i in order])


def _build(ps, k, full_lsd=0, **kw):
    from megagta_amd import api
    c = api.Context(0)
    try:
        if full_lsd:
            c.set_full_lsd(full_lsd)
        return c.build_sdbg(c.upload_reads(*ps), k, **kw)
    finally:
        c.close()


def _tiles(k):
    """LocalCfg::kTile, lds_cap of the key width (sdbg_build.hip)"""
    w = (2 * k + 4 + 31) // 32
    local = 4096 if w <= 4 else 2048
    return local, (2 * local if w <= 8 else local)


def _one_level_windows(k, rng):
    """the motif, then four characters that decide the piece a key falls into when the segment is split: 56 % AAAA (one piece above
    lds_cap: the next level resolves it on the random characters behind), 29 % CAAA (one piece between the two tile sizes, or a
    second oversized one where the key width has no big tile), 7.5 % each G... and T... with random characters (short pieces, packed
    several to a range).  Where the digit right below the prefix is narrower than 8 bits it still starts with the first of the four
    characters, so the classes hold for every key width.  A quarter of the reads is random (the other segments)."""
    local, cap = _tiles(k)
    n = 6 * local                                                            # keys of the motif segment
    L = k + 4
    cls = rng.choice(4, n, p=[0.56, 0.29, 0.075, 0.075])
    counts = np.bincount(cls, minlength=4)
    assert counts[0] > cap and local < counts[1] and (cap == local or counts[1] <= cap) and counts[2] + counts[3] <= local
    out = []
    for c in cls:
        r = rng.integers(0, 4, L).astype(np.uint8)
        r[:8] = MOTIF
        r[8] = c
        if c < 2:
            r[9:12] = 0
        out.append(r)
    out += [rng.integers(0, 4, L).astype(np.uint8) for _ in range(n // 3)]
    return out


def _several_level_windows(k, rng, copies):
    """a 16-base motif: behind 16 sorted bits the two digits below the prefix are the same in every key of the segment (two levels see
    one bin), the third level splits on random characters.  `copies` of every read (equal keys; solid edges for stage 1)"""
    local, cap = _tiles(k)
    L = k + 4
    out = []
    for _ in range(3 * cap // (2 * copies)):
        r = rng.integers(0, 4, L).astype(np.uint8)
        r[:16] = MOTIF16
        out += [r] * copies
    for _ in range(cap // (2 * copies)):
        out += [rng.integers(0, 4, L).astype(np.uint8)] * copies
    return out


@pytest.fixture(scope="module")
def one_level_44(oracle):
    ps = _pack(_one_level_windows(44, np.random.default_rng(44)), np.random.default_rng(1))
    return ps, oracle.Stream.build(*ps, 44, threads=4).edges()


@pytest.fixture(scope="module")
def several_levels_44():
    return _pack(_several_level_windows(44, np.random.default_rng(45), 2), np.random.default_rng(2))


def _check_plain(st, levels):
    assert 65536 < st["n_items"] < 1 << 24 and st["n_sort_launches"] == 2, st   # two 8-bit global passes: 16 sorted bits
    assert st["n_big_segments"] >= 1 and st["n_split_levels"] >= levels, st


def test_one_level(one_level_44):
    """k = 44 (W = 3, tiles of 4096 / 8192 keys): every class of piece; the oversized piece takes a second level"""
    ps, orc = one_level_44
    g = _build(ps, 44)
    _same(g, orc)
    _check_plain(g.stats, 2)
    assert g.stats["n_split_levels"] <= 4, g.stats                           # (the segments of the shifted motif: one or two idle levels)


@pytest.mark.parametrize("k", [21, 79, 127])
def test_key_widths(oracle, k):
    """W = 2; W = 6 (tiles of 2048 / 4096 keys); W = 9 (no big tile: lds_cap is LocalCfg::kTile, no piece goes to segment_lds_kernel)"""
    ps = _pack(_one_level_windows(k, np.random.default_rng(k)), np.random.default_rng(3))
    g = _build(ps, k)
    _same(g, oracle.Stream.build(*ps, k, threads=4).edges())
    assert g.stats["words_per_key"] == (2 * k + 4 + 31) // 32
    _check_plain(g.stats, 2)


def test_several_levels_with_idle_levels(oracle, several_levels_44):
    """two levels that find one bin and move nothing, then the one that splits"""
    ps = several_levels_44
    g = _build(ps, 44)
    _same(g, oracle.Stream.build(*ps, 44, threads=4).edges())
    _check_plain(g.stats, 3)


def test_stage1_payload_and_mercy(oracle, several_levels_44):
    """min_count = 2 with mercy edges on the same input: stage 1 sorts records of W + 2 words whose last bits are a payload no digit
    looks at (equal keys must keep the order the global passes left them in), and the mercy candidates as Key<2>"""
    ps = several_levels_44
    g = _build(ps, 44, min_count=2, need_mercy=True)
    _same(g, oracle.Stream.build_solid(*ps, 44, 2, True, threads=4).edges())
    assert g.stats["n_split_levels"] >= 3, g.stats


@pytest.mark.parametrize("extra", [False, True])
def test_hot_kmer(oracle, extra):
    """more than 8192 identical keys (poly-A, and poly-T on the other strand) in one segment with keys that differ from them only in
    the last character (second lowest digit) or only in the 4-bit digit at position 0 (the $ items of every read, and of shorter
    poly-A reads, which end inside the run).  The run is longer than a tile at every level, is moved by every level that finds a
    second bin and must end in the result buffer.  `extra` adds reads that leave the run at character 12: their keys that start
    with 8 A's differ from the run in the first level's digit and in no other, so exactly one more level moves the run: the
    other buffer parity"""
    k, L = 44, 48
    rng = np.random.default_rng(5)
    wins = [np.zeros(L, np.uint8) for _ in range(3000)]                      # 4 equal solid keys per read and strand: 12 000
    for _ in range(300):                                                     # equal but for the last base
        r = np.zeros(L, np.uint8)
        r[-1] = rng.integers(1, 4)
        wins.append(r)
    wins += [np.zeros(int(rng.integers(k + 1, L)), np.uint8) for _ in range(300)]   # the read ends inside the run
    if extra:
        for _ in range(600):
            r = rng.integers(0, 4, L).astype(np.uint8)
            r[:11] = 0
            r[11] = 1
            wins.append(r)
    wins += [rng.integers(0, 4, L).astype(np.uint8) for _ in range(3000)]
    ps = _pack(wins, rng)
    g = _build(ps, k)
    _same(g, oracle.Stream.build(*ps, k, threads=4).edges())
    st = g.stats
    assert 65536 < st["n_items"] and st["n_sort_launches"] == 2, st
    assert st["n_big_segments"] >= 2 and st["n_split_levels"] == 10, st      # every low digit of k = 44 behind 16 bits: 9 of characters, 1 of flags


def test_whole_array_as_one_segment(oracle):
    """set_full_lsd(1): no global pass, the whole array is one deferred segment and the split is the whole sort"""
    k = 44
    rng = np.random.default_rng(6)
    ps = _pack([rng.integers(0, 4, k + 4).astype(np.uint8) for _ in range(1500)], rng)
    plain = _build(ps, k)
    g = _build(ps, k, full_lsd=1)
    assert g.stats["n_items"] == plain.stats["n_items"] > 8192
    assert g.stats["n_sort_launches"] == 0 and g.stats["n_big_segments"] == 1 and g.stats["n_split_levels"] >= 1, g.stats
    _same(g, plain)
    _same(g, oracle.Stream.build(*ps, k, threads=4).edges())


def test_bucket_sub_range(monkeypatch, one_level_44):
    """the buckets around the motif's, MGTA_SORT_WIDE=2 and MGTA_SORT_BIAS=2: a 9-bit pass and skipped leading bits, so the sorted
    prefix is no multiple of 8 bits and the digit the first level splits on is narrower than 8"""
    ps, orc = one_level_44
    b = int(sum(int(c) << (14 - 2 * i) for i, c in enumerate(MOTIF)))
    b0, b1 = max(0, b - 5000), min(65536, b + 5000)
    monkeypatch.setenv("MGTA_SORT_WIDE", "2")
    monkeypatch.setenv("MGTA_SORT_BIAS", "2")
    g = _build(ps, 44, bucket_range=(b0, b1))
    _same_slice(g, orc, b0, b1)
    st = g.stats
    assert st["n_wide_passes"] >= 1 and st["n_big_segments"] >= 1 and st["n_split_levels"] >= 2, st
