"""emit_decide_write_kernel (MGTA_EMIT_CHAIN): every run decided and its record written by one kernel behind two chained scans.

Every case builds with MGTA_EMIT_CHAIN=2: the three-step route (emit_decide_kernel, three scans, emit_write_kernel) runs next to the
one kernel, and the records, the large counts, the tip words, the bucket boundaries and the three totals are compared on the device;
any difference fails the build with MGTA_EINTERNAL.  The stream that comes back is the one kernel's, and it is compared with the CPU
oracle's as well.

A workgroup of the kernel takes 8 rounds of 1024 runs (kChainRounds x kDecideTile = kChainTile = 8192).  A run is a distinct sort
item.  How the inputs reach the sizes and places they are after:

  run counts        reads of k + 1 .. k + 4 random bases give 6, 8, 10, 12 sort items, all distinct; at k = 21 (k + 1 even) a read that
                    is one palindromic 22-mer gives 3 (its reverse complement is itself), so every run count is reachable.  The build's
                    n_items is asserted, and that every record has multiplicity 1: then the number of runs is n_items.
  long runs         a read of k + 1 A's, N times: the poly-A keys are the smallest of all and the poly-T keys of the other strand the
                    largest, so runs of N keys are the first runs of the first tile and the last runs of the last one.
  groups            every read with all four last bases and all four first bases: at least a sixth of the records carry the mark of
                    a run in front of them in their (k-1)-mer group (w >= 5, from the CPU oracle), so the run at a round's or a
                    workgroup's start lies inside a group with that chance at least.  430 000 records hold more than 50 workgroup
                    starts and 400 round starts: the chance that none of the 50 lies inside a group is below (5/6)^50 = 1e-4 (fixed
                    seed: the input is the same every time).  The first run of the first tile is a bucket head; with 132 tiles and
                    a twelfth of the runs being tips, some tile starts with one.  These places are reached by density, not by
                    construction: the order of the keys is the sort's business.
"""
import numpy as np
import pytest

from megagta_amd import readlib

pytestmark = pytest.mark.gpu

ROUND, TILE = 1024, 8192                                                     # kDecideTile, kChainTile (sdbg_build.hip)


def _build(ps, k, full_lsd=0, **kw):
    from megagta_amd import api
    c = api.Context(0)
    try:
        if full_lsd:
            c.set_full_lsd(full_lsd)
        return c.build_sdbg(c.upload_reads(*ps), k, **kw)
    finally:
        c.close()


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


def _checked(monkeypatch, ps, k, **kw):
    monkeypatch.setenv("MGTA_EMIT_CHAIN", "2")
    return _build(ps, k, **kw)


def _reads_with_items(k, n_items, rng):
    """random reads, shuffled, whose sort items number exactly n_items (see the module docstring)"""
    reads = []
    if n_items & 1:
        assert (k + 1) % 2 == 0 and n_items >= 3
        half = rng.integers(0, 4, (k + 1) // 2).astype(np.uint8)
        reads.append(np.concatenate([half, (3 - half)[::-1]]))               # a palindromic (k+1)-mer: 3 items
        n_items -= 3
    n12, rem = divmod(n_items, 12)
    if rem in (2, 4):                                                         # 12 + 2 = 6 + 8, 12 + 4 = 6 + 10
        assert n12 >= 1
        n12 -= 1
        extra = (k + 1, k + 2) if rem == 2 else (k + 1, k + 3)
    else:
        extra = {0: (), 6: (k + 1,), 8: (k + 2,), 10: (k + 3,)}[rem]
    for length in (k + 4,) * n12 + extra:
        reads.append(rng.integers(0, 4, length).astype(np.uint8))
    return readlib.pack_for_build([reads[i] for i in rng.permutation(len(reads))])


def _group_reads(k, n_base, rng):
    """n_base random reads of k + 4 bases, each with every last base and every first base (7 reads): keys that differ in `a` or in `b` only"""
    out = []
    for _ in range(n_base):
        r = rng.integers(0, 4, k + 4).astype(np.uint8)
        for c in range(4):
            v = r.copy(); v[-1] = c; out.append(v)
        for c in range(4):
            if c != r[0]:
                v = r.copy(); v[0] = c; out.append(v)
    return readlib.pack_for_build([out[i] for i in rng.permutation(len(out))])


@pytest.mark.parametrize("n_runs", [1, ROUND - 1, ROUND, ROUND + 1, TILE - 1, TILE, TILE + 1])
def test_run_counts_at_round_and_workgroup_edges(monkeypatch, oracle, n_runs):
    """one round, one round +- 1, one workgroup (round x rounds) +- 1 runs at k = 21 (W = 2; k + 1 even: tips of 2 words, the palindrome's
    sentinel slots dropped before the emitter); n_runs = 1: single buckets of a build of 60 items"""
    k = 21
    rng = np.random.default_rng(1000 + n_runs)
    if n_runs == 1:
        return _single_run_and_empty_range(monkeypatch, oracle, k, rng)
    ps = _reads_with_items(k, n_runs, rng)
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    g = _checked(monkeypatch, ps, k)
    _same(g, orc)
    assert g.stats["n_items"] == n_runs, g.stats
    assert g.records.size and np.all(g.records >> 8 == 1)                    # no two equal keys: as many runs as items


def _single_run_and_empty_range(monkeypatch, oracle, k, rng):
    """a bucket range that holds one record, and one that holds no key at all"""
    ps = _reads_with_items(k, 60, rng)
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    single = 0
    for b in np.flatnonzero(orc.bucket_items == 1)[:12]:                     # (a suppressed run may share a bucket with the record)
        g = _checked(monkeypatch, ps, k, bucket_range=(int(b), int(b) + 1))
        _same_slice(g, orc, int(b), int(b) + 1)
        assert g.records.size == 1 and g.stats["n_items"] >= 1, g.stats
        single += g.stats["n_items"] == 1
    assert single >= 1
    empty = int(np.flatnonzero(orc.bucket_items == 0)[0])
    g = _checked(monkeypatch, ps, k, bucket_range=(empty, empty + 1))
    assert g.records.size == 0 and g.tips.size == 0 and g.large.size == 0


@pytest.mark.parametrize("k", [44, 21])
def test_groups_across_rounds_and_workgroups(monkeypatch, oracle, k):
    """groups of four runs almost everywhere (W = 3 and W = 2): walks that cross a round's and a workgroup's first run, in LDS and,
    where they leave the halo, in device memory; the three-step route alone gives the same stream"""
    ps = _group_reads(k, 12000, np.random.default_rng(2000 + k))
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    g = _checked(monkeypatch, ps, k)
    _same(g, orc)
    assert g.records.size > 50 * TILE and np.mean((g.records & 15) >= 5) > 0.16, g.stats
    monkeypatch.setenv("MGTA_EMIT_CHAIN", "0")
    g0 = _build(ps, k)
    assert g0.md5() == g.md5() and np.array_equal(g0.records, g.records)


@pytest.mark.parametrize("copies", [254, 255, 65536 + 3])
def test_long_runs_first_and_last(monkeypatch, oracle, copies):
    """runs of 254 (the last count a record holds), 255 (the first large one) and more than 65535 keys (capped) as the first runs of
    the first tile and the last runs of the last one, next to 3 000 random reads"""
    k = 44
    rng = np.random.default_rng(3000 + copies)
    reads = [np.zeros(k + 1, np.uint8)] * copies + [rng.integers(0, 4, k + 4).astype(np.uint8) for _ in range(3000)]
    ps = readlib.pack_for_build([reads[i] for i in rng.permutation(len(reads))])
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    g = _checked(monkeypatch, ps, k)
    _same(g, orc)
    want = min(copies, 65535)
    if copies > 254:
        assert g.large.size >= 2 and g.large[0] == want and g.large[-1] == want, g.large
        assert g.records[0] >> 8 == 255 and g.records[-1] >> 8 == 255
    else:
        assert g.large.size == 0 and g.records[0] >> 8 == 254 and g.records[-1] >> 8 == 254


def test_look_back_past_two_windows(monkeypatch, oracle):
    """132 workgroups: a look-back that has to walk past two full windows of 64 predecessors finds its way"""
    k = 44
    rng = np.random.default_rng(4000)
    ps = readlib.pack_for_build([rng.integers(0, 4, k + 4).astype(np.uint8) for _ in range(90200)])
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    g = _checked(monkeypatch, ps, k)
    _same(g, orc)
    assert g.stats["n_items"] > 131 * TILE and np.all(g.records >> 8 == 1), g.stats


def test_tiles_numbered_by_ticket(monkeypatch, oracle):
    """set_full_lsd(1): both chained kernels of the emitter number their tiles by ticket (the route the host repeats a launch with
    when a look-back ever waits in vain)"""
    k = 44
    rng = np.random.default_rng(5000)
    ps = readlib.pack_for_build([rng.integers(0, 4, k + 4).astype(np.uint8) for _ in range(6000)])
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    g = _checked(monkeypatch, ps, k, full_lsd=1)
    _same(g, orc)
    assert g.stats["n_items"] > 8 * TILE, g.stats


@pytest.mark.parametrize("k", [44, 21])
def test_two_bucket_ranges(monkeypatch, oracle, k):
    """the buckets in two builds: the second one's bucket boundaries are written relative to a non-zero first bucket"""
    ps = _group_reads(k, 300, np.random.default_rng(6000 + k))
    orc = oracle.Stream.build(*ps, k, threads=4).edges()
    cut = int(np.searchsorted(np.cumsum(orc.bucket_items), orc.bucket_items.sum() // 2))
    for b0, b1 in ((0, cut), (cut, 65536)):
        g = _checked(monkeypatch, ps, k, bucket_range=(b0, b1))
        _same_slice(g, orc, b0, b1)
        assert g.records.size > 0
