"""The emitter's info byte of every key position, written by the segment-local finish of the sort while the sorted keys are still
in LDS (local_sort_kernel's epilogue, emit_info_range_kernel for every range that kernel did not finish), and compacted by
emit_compact_info_kernel without a second read of the keys (MGTA_EMIT_FUSED).

Every case builds with MGTA_EMIT_FUSED=2 (the run descriptors are also taken from the keys by emit_compact_kernel and compared on
the device: a difference fails the build), compares the whole edge stream with the CPU oracle's, builds once more with
MGTA_EMIT_FUSED=0 for the same md5, and reads off the stats that the route meant ran.

Inputs as in test_segment_split_gpu.py: reads of k + 4 bases (12 sort items each), ten to twenty thousand of them, so that a sort
holds between 65 537 and 16.7 M items and its two global passes sort T = 16 leading bits = the bucket: every tile's first key
starts a bucket.  A key is a window of the reversed read or of its reverse complement.

What the inputs hold, from the generators and the CPU oracle (no GPU; `python tests/test_emit_fused_gpu.py` prints the read counts):
  runs_and_groups   16 001 reads = 192 012 items (192 012 % 64 = 12): 5 333 distinct reads 3 times, one twice; at k = 44 the oracle
                    yields 56 008 records, 47 996 of multiplicity 3 and 8 000 of 6 and more: runs of 3 equal keys almost everywhere
  lsd_tiles         10 800 reads: 6 reads x 300, every one of their 72 keys 300 times (> kMaxRun = 256), next to 9 000 random reads
  one_level (k=44)  32 768 reads; the motif's bucket (7122) holds 24 585 records = a segment of 6 tiles of 4096 behind 16 sorted bits;
                    the generator asserts its pieces: one > 8192, one in (4096, 8192], the short ones <= 4096 together
  several_levels    16 384 reads; 12 288 of them behind a 16-base motif in one segment (> 8192), two idle levels
  hot_read          13 300 reads: one read 10 000 times (12 runs of 10 000 equal keys > 8192: never moved), 300 that differ from it
                    in the last base only, 3 000 random
  one_segment       1 500 reads = 18 000 items > 8192 behind no global pass (set_full_lsd(1)); 5 reads = 60 items < 64
  sub-range         the buckets [2122, 12122) of one_level: 62 125 records; mgta_sort_plan_wide gives T = 19 from 30 k to 200 k items"""
import ctypes as C

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


def _both(monkeypatch, ps, k, check, **kw):
    """the checked build against the oracle (check(gpu stream)), then the old route for the same md5; the checked build's stats"""
    monkeypatch.setenv("MGTA_EMIT_FUSED", "2")
    g = _build(ps, k, **kw)
    check(g)
    monkeypatch.setenv("MGTA_EMIT_FUSED", "0")
    g0 = _build(ps, k, **kw)
    assert g0.md5() == g.md5() and np.array_equal(g0.records, g.records)
    assert g0.stats["n_emit_fused"] == 0, g0.stats
    return g.stats


def _plan_T(n_items, k, b0=0, b1=65536):
    """leading bits the global passes of such a sort order the keys by (mgta_sort_plan_wide: W >= 2)"""
    from megagta_amd import _lib
    n_pass, skip, widths = C.c_int(0), C.c_int(0), (C.c_int * 4)()
    assert _lib.load().mgta_sort_plan_wide(n_items, (2 * k + 4 + 31) // 32, b0, b1, C.byref(n_pass), C.byref(skip), widths) == 0
    return sum(widths[i] for i in range(n_pass.value)) + skip.value


def _tiles(k):
    """LocalCfg::kTile, lds_cap of the key width (sdbg_build.hip)"""
    w = (2 * k + 4 + 31) // 32
    local = 4096 if w <= 4 else 2048
    return local, (2 * local if w <= 8 else local)


def _random_windows(k, rng, n):
    return [rng.integers(0, 4, k + 4).astype(np.uint8) for _ in range(n)]


def _runs_and_groups_windows(k, rng):
    """every read 3 times (equal keys); for 1 000 of them one more read, 3 times, that differs in its last base only: the keys that
    end with that base share their (k-1)-mer and differ in `a` (a group of two runs); 16 001 reads: 192 012 items, no multiple of 64"""
    out = []
    base = _random_windows(k, rng, 4333)
    for r in base:
        out += [r] * 3
    for r in base[:1000]:
        v = r.copy()
        v[-1] = (v[-1] + 1 + rng.integers(0, 3)) & 3
        out += [v] * 3
    out += [rng.integers(0, 4, k + 4).astype(np.uint8)] * 2                 # 12 999 + 3 000 + 2
    return out


def _lsd_tile_windows(k, rng):
    out = []
    for r in _random_windows(k, rng, 6):
        out += [r] * 300
    return out + _random_windows(k, rng, 9000)


def _one_level_windows(k, rng):
    """the motif, then four characters that decide the piece a key falls into when the segment is split: 56 % AAAA (one piece above
    lds_cap), 29 % CAAA (one piece between the two tile sizes), 7.5 % each G... and T... (short pieces); a quarter random reads"""
    local, cap = _tiles(k)
    n = 6 * local
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
    return out + _random_windows(k, rng, n // 3)


def _several_level_windows(k, rng, copies):
    """a 16-base motif: the two digits below the 16 sorted bits are the same in every key of the segment (two levels see one bin)"""
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


def _hot_read_windows(k, rng):
    """one read 10 000 times: each of its 12 keys is a run of 10 000 (> 8192: no level of the split moves it); 300 reads that differ from
    it in the last base only share its segments, so that a level finds a second bin there"""
    hot = rng.integers(0, 4, k + 4).astype(np.uint8)
    out = [hot] * 10000
    for _ in range(300):
        v = hot.copy()
        v[-1] = (v[-1] + 1 + rng.integers(0, 3)) & 3
        out.append(v)
    return out + _random_windows(k, rng, 3000)


def _plain(st):
    assert 65536 < st["n_items"] < 1 << 24 and st["n_sort_launches"] == 2, st   # two 8-bit global passes: T = 16


@pytest.fixture(scope="module")
def one_level_44(oracle):
    ps = _pack(_one_level_windows(44, np.random.default_rng(44)), np.random.default_rng(1))
    return ps, oracle.Stream.build(*ps, 44, threads=4).edges()


@pytest.mark.parametrize("k", [44, 21, 9])
def test_comparison_route(monkeypatch, oracle, k):
    """random reads: every tile is finished by comparison and writes its own info bytes; T = 16, so every tile's first key starts a
    bucket.  k = 9 (W = 1): T = 16 = 2 (k - 1), the last prefix the rule for a tile's first key holds for"""
    rng = np.random.default_rng(100 + k)
    ps = _pack(_random_windows(k, rng, 12000), rng)
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    st = _both(monkeypatch, ps, k, lambda g: _same(g, orc))
    _plain(st)
    if k > 14:
        assert _plan_T(st["n_items"], k) == 16
    assert st["n_emit_fused"] >= 1 and st["n_lsd_tiles"] == 0, st


@pytest.mark.parametrize("k", [44, 21])
def test_runs_and_groups_at_window_and_tile_edges(monkeypatch, oracle, k):
    """runs of 3 and more equal keys and groups of two runs everywhere, so also across the 64-key windows and the tile starts; an item
    count that is no multiple of 64"""
    ps = _pack(_runs_and_groups_windows(k, np.random.default_rng(200 + k)), np.random.default_rng(7))
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    st = _both(monkeypatch, ps, k, lambda g: _same(g, orc))
    _plain(st)
    assert st["n_items"] % 64 != 0 and st["n_emit_fused"] >= 1 and st["n_lsd_tiles"] == 0, st


def test_lsd_tiles(monkeypatch, oracle):
    """runs longer than kMaxRun: their tiles go to local_lsd_kernel and get their info bytes from emit_info_range_kernel"""
    k = 44
    ps = _pack(_lsd_tile_windows(k, np.random.default_rng(300)), np.random.default_rng(8))
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    st = _both(monkeypatch, ps, k, lambda g: _same(g, orc))
    _plain(st)
    assert st["n_emit_fused"] >= 1 and st["n_lsd_tiles"] > 0, st


def test_oversized_one_level(monkeypatch, one_level_44):
    ps, orc = one_level_44
    st = _both(monkeypatch, ps, 44, lambda g: _same(g, orc))
    _plain(st)
    assert st["n_emit_fused"] >= 1 and st["n_big_segments"] >= 1 and st["n_split_levels"] >= 2, st


def test_oversized_several_levels(monkeypatch, oracle):
    k = 44
    ps = _pack(_several_level_windows(k, np.random.default_rng(45), 2), np.random.default_rng(2))
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    st = _both(monkeypatch, ps, k, lambda g: _same(g, orc))
    _plain(st)
    assert st["n_emit_fused"] >= 1 and st["n_big_segments"] >= 1 and st["n_split_levels"] >= 3, st


def test_oversized_hot_read(monkeypatch, oracle):
    """all-equal runs longer than every LDS tile: no level moves them, they stay where the global passes left them"""
    k = 44
    rng = np.random.default_rng(500)
    ps = _pack(_hot_read_windows(k, rng), rng)
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    st = _both(monkeypatch, ps, k, lambda g: _same(g, orc))
    _plain(st)
    assert st["n_emit_fused"] >= 1 and st["n_big_segments"] >= 12 and st["n_split_levels"] >= 1, st


def test_whole_array_as_one_segment(monkeypatch, oracle):
    """set_full_lsd(1): no global pass, T = 0, the whole array is one deferred segment: every info byte from emit_info_range_kernel"""
    k = 44
    rng = np.random.default_rng(6)
    ps = _pack(_random_windows(k, rng, 1500), rng)
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    st = _both(monkeypatch, ps, k, lambda g: _same(g, orc), full_lsd=1)
    assert st["n_items"] > 8192 and st["n_sort_launches"] == 0 and st["n_big_segments"] == 1 and st["n_split_levels"] >= 1, st
    assert st["n_emit_fused"] == 1, st


def test_fewer_than_64_items(monkeypatch, oracle):
    """5 reads: one tile of 60 keys behind no global pass (T = 0 < 16: its first key starts a bucket without a look at a predecessor)"""
    k = 44
    rng = np.random.default_rng(9)
    ps = _pack(_random_windows(k, rng, 5), rng)
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    st = _both(monkeypatch, ps, k, lambda g: _same(g, orc))
    assert st["n_items"] == 60 and st["n_sort_launches"] == 0 and st["n_emit_fused"] == 1 and st["n_big_segments"] == 0, st


def test_bucket_heads_inside_a_tile_and_before_it(monkeypatch, one_level_44):
    """a bucket sub-range with MGTA_SORT_WIDE=2 and MGTA_SORT_BIAS=2: T = 19 (9 + 8 bits below 2 skipped ones), so a segment is an eighth
    of a bucket, most tiles start inside a bucket and take their first key's bucket-head bit from the key before the tile"""
    ps, orc = one_level_44
    b = int(sum(int(c) << (14 - 2 * i) for i, c in enumerate(MOTIF)))
    b0, b1 = max(0, b - 5000), min(65536, b + 5000)
    monkeypatch.setenv("MGTA_SORT_WIDE", "2")
    monkeypatch.setenv("MGTA_SORT_BIAS", "2")
    st = _both(monkeypatch, ps, 44, lambda g: _same_slice(g, orc, b0, b1), bucket_range=(b0, b1))
    assert _plan_T(st["n_items"], 44, b0, b1) == 19
    assert st["n_wide_passes"] >= 1 and st["n_big_segments"] >= 1 and st["n_emit_fused"] >= 1, st


@pytest.mark.parametrize("k,full_lsd,fused", [(44, 1, True), (44, 2, True), (79, 0, True), (127, 0, True)])
def test_other_routes_and_key_widths(monkeypatch, oracle, k, full_lsd, fused):
    """set_full_lsd(1): the emitter numbers its tiles by ticket; set_full_lsd(2): no finish by comparison, every tile through
    local_lsd_kernel.  k = 79, 127 (W = 5, 8; tiles of 2048 keys): T = 16 <= 2 (k - 1), so the route runs at these widths too"""
    rng = np.random.default_rng(700 + k + full_lsd)
    ps = _pack(_random_windows(k, rng, 10000), rng)
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    st = _both(monkeypatch, ps, k, lambda g: _same(g, orc), full_lsd=full_lsd)
    assert (st["n_emit_fused"] >= 1) == fused, st
    if full_lsd == 2:
        assert st["n_lsd_tiles"] > 0, st


def test_stage1_build(monkeypatch, oracle):
    """min_count = 2: stage 1 sorts masked records and emits nothing (no info bytes asked for), stage 2 takes the route"""
    k = 44
    ps = _pack(_several_level_windows(k, np.random.default_rng(45), 2), np.random.default_rng(2))
    orc = oracle.Stream.build_solid(*ps, k, 2, False, threads=4).edges()
    st = _both(monkeypatch, ps, k, lambda g: _same(g, orc), min_count=2)
    assert st["n_emit_fused"] >= 1, st


def test_fallback_prefix_longer_than_the_k_minus_1_mer(monkeypatch, oracle):
    """k = 9 (W = 1), a bucket sub-range with MGTA_SORT_BIAS=2: 16 sorted bits below 3 skipped ones, T = 19 > 16 = 2 (k - 1).  Two keys of one
    (k-1)-mer can then lie in two segments, the rule for a tile's first key does not hold and the emitter reads the keys as before"""
    k = 9
    rng = np.random.default_rng(900)
    ps = _pack(_random_windows(k, rng, 60000), rng)
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    b0, b1 = 20000, 28000                                                   # (8000 << 16) - 1 < 2^29: three leading zero bits
    monkeypatch.setenv("MGTA_SORT_BIAS", "2")
    st = _both(monkeypatch, ps, k, lambda g: _same_slice(g, orc, b0, b1), bucket_range=(b0, b1))
    assert st["n_sort_launches"] == 2 and st["n_emit_fused"] == 0, st


if __name__ == "__main__":                                                   # what the inputs hold (CPU only; see the module docstring)
    for name, fn, k in (("runs_and_groups", _runs_and_groups_windows, 44), ("lsd_tiles", _lsd_tile_windows, 44), ("one_level", _one_level_windows, 44),
                        ("hot_read", _hot_read_windows, 44)):
        wins = fn(k, np.random.default_rng(1))
        uniq, cnt = np.unique(np.stack([w[:k + 4] for w in wins]), axis=0, return_counts=True)
        print(f"{name}: {len(wins)} reads = {12 * len(wins)} items ({12 * len(wins) % 64} mod 64), {len(uniq)} distinct, copies min {cnt.min()} max {cnt.max()}")
