"""mgta_rows_pairs / mgta_rows_cluster on the device against `restate`, the contract of include/megagta_hip.h written out in Python: the
pair counts as two loops over bytes, the kept rule with Python floats (IEEE doubles), the linkage as the naive loop with
fractions.Fraction.  Every comparison is exact: the pair list element for element, cluster / rep / rep_diff / rep_overlap for every row.
The jars of the reference (`Clustering.jar`) are not available; the rule is this project's own."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from megagta_amd import align as al
from megagta_amd import cluster as cl
from megagta_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
GAP = 45                                                                  # '-'


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------
def pair_counts(a: bytes, b: bytes):
    n_overlap = n_diff = 0
    for x, y in zip(a, b):
        if x != GAP and y != GAP:
            n_overlap += 1
            if x != y:
                n_diff += 1
    return n_diff, n_overlap


def is_kept(n_diff, n_overlap, min_overlap, cutoff):
    return n_overlap >= min_overlap and float(n_diff) <= cutoff * float(n_overlap)


def restate_pairs(rows, min_overlap, cutoff):
    out = []
    for i in range(len(rows)):
        for j in range(i + 1, len(rows)):
            d, o = pair_counts(rows[i], rows[j])
            if is_kept(d, o, min_overlap, cutoff):
                out.append((i, j, d, o))
    return out


def restate_link(rows, lens, pairs):
    """the naive loop of the contract over the kept pairs -> (cluster, rep, rep_diff, rep_overlap) per row"""
    n = len(rows)
    kept = {(i, j): (d, o) for i, j, d, o in pairs}
    n_res = [sum(1 for x in r if x != GAP) for r in rows]
    clusters = [[i] for i in range(n) if n_res[i] > 0]                    # each sorted, the list sorted by lowest member
    while True:
        best = None
        for x in range(len(clusters)):
            for y in range(x + 1, len(clusters)):
                A, B = clusters[x], clusters[y]                           # min(A) < min(B)
                dist = None
                for i in A:
                    for j in B:
                        p = kept.get((min(i, j), max(i, j)))
                        if p is None:
                            break
                        f = Fraction(p[0], p[1])
                        dist = f if dist is None or f > dist else dist
                    else:
                        continue
                    break
                else:
                    key = (dist, A[0], B[0])
                    if best is None or key < best[0]:
                        best = (key, x, y)
        if best is None:
            break
        _, x, y = best
        clusters[x] = sorted(clusters[x] + clusters[y])
        del clusters[y]
    cluster, rep, rd, ro = [-1] * n, [-1] * n, [0] * n, [0] * n
    for number, members in enumerate(clusters):
        r = max(members, key=lambda i: (lens[i], -i))
        for i in members:
            cluster[i], rep[i] = number, r
            rd[i], ro[i] = (0, n_res[i]) if i == r else kept[(min(i, r), max(i, r))]
    return cluster, rep, rd, ro


def restate(rows, lens, min_overlap, cutoff):
    pairs = restate_pairs(rows, min_overlap, cutoff)
    return pairs, restate_link(rows, lens, pairs)


def pair_list(res):
    p = res["pairs"]
    return list(zip(p["i"].tolist(), p["j"].tolist(), p["n_diff"].tolist(), p["n_overlap"].tolist()))


def assert_is(ctx, rows, lens, min_overlap, cutoff, want=None, what=""):
    pairs, (cluster, rep, rd, ro) = want if want is not None else restate(rows, lens, min_overlap, cutoff)
    got = ctx.row_pairs(rows, min_overlap, cutoff)
    assert pair_list(got) == pairs, what
    assert got["stats"]["n_pairs_kept"] == len(pairs) and got["stats"]["n_rows"] == len(rows)
    res = ctx.cluster(rows, lens, min_overlap, cutoff)
    assert res["cluster"].tolist() == cluster, what
    assert res["rep"].tolist() == rep, what
    assert res["rep_diff"].tolist() == rd and res["rep_overlap"].tolist() == ro, what
    st = res["stats"]
    sizes = np.bincount(np.array([c for c in cluster if c >= 0], dtype=np.int64)) if any(c >= 0 for c in cluster) else np.zeros(0, dtype=np.int64)
    assert st["n_rows"] == len(rows) and st["n_pairs_kept"] == len(pairs) and st["n_unaligned"] == cluster.count(-1)
    assert st["n_clusters"] == sizes.size and st["n_singletons"] == int((sizes == 1).sum()) and st["largest_cluster"] == (int(sizes.max()) if sizes.size else 0)
    return res


def random_rows(n, M, seed):
    """rows over a 4-letter alphabet near three templates, `-` runs at both ends and inside, now and then a row of `-` only: many
    pairs kept and many apart at min_overlap = max(1, M // 4), cutoff 0.1"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACDE", dtype=np.uint8)
    templates = letters[rng.integers(0, 4, (3, M))]
    rows = []
    for i in range(n):
        r = templates[rng.integers(0, 3)].copy()
        hit = rng.random(M) < 0.04
        r[hit] = letters[rng.integers(0, 4, int(hit.sum()))]
        r[:int(rng.integers(0, M // 3 + 1))] = GAP
        tail = int(rng.integers(0, M // 3 + 1))
        if tail:
            r[M - tail:] = GAP
        if M >= 5 and rng.random() < 0.5:
            at = int(rng.integers(0, M))
            r[at:at + int(rng.integers(1, M // 5 + 1))] = GAP
        if rng.random() < 0.03:
            r[:] = GAP
        rows.append(r.tobytes())
    lens = [int(x) for x in rng.integers(1, 4, n)]                        # few values: the representative is often decided by the index
    return rows, lens


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


# ---- 1. tile and word edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 63, 64, 65, 257])
def test_tile_and_word_edges(ctx, n, M):
    rows, lens = random_rows(n, M, seed=1000 * n + M)
    min_overlap, cutoff = max(1, M // 4), 0.1
    want = restate(rows, lens, min_overlap, cutoff)
    tiles = {}
    try:
        for tile in (0, 1, 7):
            ctx.set_cluster_tile(tile)
            res = assert_is(ctx, rows, lens, min_overlap, cutoff, want, what=f"tile {tile}")
            tiles[tile] = res["stats"]["n_tiles"]
    finally:
        ctx.set_cluster_tile(0)
    blocks = lambda r: -(-n // r)
    assert tiles == {0: 1, 1: n * (n + 1) // 2, 7: blocks(7) * (blocks(7) + 1) // 2}
    if n >= 63 and M >= 5:
        assert 0 < len(want[0]) < n * (n - 1) // 2                        # some kept, some apart


def test_long_rows(ctx):
    rows, lens = random_rows(40, 1200, seed=5)
    want = restate(rows, lens, 300, 0.1)
    assert len(want[0]) > 0
    try:
        for tile in (0, 7):
            ctx.set_cluster_tile(tile)
            assert_is(ctx, rows, lens, 300, 0.1, want)
    finally:
        ctx.set_cluster_tile(0)


# ---- 2. the boundaries of the kept rule ----------------------------------------------------------------------------------------------
def test_kept_rule_boundaries(ctx):
    # n_overlap at min_overlap and one below it
    rows = [b"AAAA----", b"AAAAAA--"]
    assert pair_list(ctx.row_pairs(rows, 4, 0.0)) == [(0, 1, 0, 4)]
    assert pair_list(ctx.row_pairs(rows, 5, 0.0)) == []
    # n_diff exactly at the cut-off and one above it: 2/4 and 3/4 at 0.5
    rows = [b"AAAA", b"AACC", b"ACCC"]
    assert pair_list(ctx.row_pairs(rows, 1, 0.5)) == [(0, 1, 2, 4), (1, 2, 1, 4)] == restate_pairs(rows, 1, 0.5)
    # 1/100 and 2/100 at 0.01 (0.01 * 100.0 is 1.0 in fp64)
    rows = [b"A" * 100, b"A" * 99 + b"C", b"A" * 98 + b"CC"]
    assert pair_list(ctx.row_pairs(rows, 25, 0.01)) == [(0, 1, 1, 100), (1, 2, 1, 100)] == restate_pairs(rows, 25, 0.01)
    # 1/99 at 0.01 is beyond it
    rows = [b"A" * 99 + b"-", b"A" * 98 + b"C-"]
    assert pair_list(ctx.row_pairs(rows, 25, 0.01)) == [] == restate_pairs(rows, 25, 0.01)
    # cut-off 0: identical where they overlap; cut-off 1: whatever overlaps enough
    rows = [b"ACDE-", b"ACDEA", b"CDEAC", b"----A"]
    for cutoff in (0.0, 1.0):
        assert_is(ctx, rows, [4, 5, 5, 1], 1, cutoff)
    assert pair_list(ctx.row_pairs(rows, 1, 0.0)) == [(0, 1, 0, 4), (1, 3, 0, 1)]
    assert pair_list(ctx.row_pairs(rows, 1, 1.0)) == [(0, 1, 0, 4), (0, 2, 4, 4), (1, 2, 5, 5), (1, 3, 0, 1), (2, 3, 1, 1)]


# ---- 3. bytes ------------------------------------------------------------------------------------------------------------------------
def test_bytes(ctx):
    # values >= 128 are residues like any other; lower case differs from upper case; 0 is a residue too
    rows = [bytes([200, 201, 255, 128]), bytes([200, 201, 255, 129]), b"acde", b"ACDE", b"acdE", bytes([0, 0, 0, 0]), bytes([0, 0, GAP, 0])]
    lens = [4] * 7
    assert_is(ctx, rows, lens, 1, 0.25)
    got = pair_list(ctx.row_pairs(rows, 1, 0.25))
    assert (0, 1, 1, 4) in got and (2, 4, 1, 4) in got and (5, 6, 0, 3) in got and not [p for p in got if p[:2] in ((2, 3), (3, 4))]
    # a row of `-` only: unaligned, no pairs, cluster -1
    rows = [b"ACDE", b"----", b"ACDE"]
    res = assert_is(ctx, rows, [4, 0, 4], 1, 0.0)
    assert res["cluster"].tolist() == [0, -1, 0] and res["rep"].tolist() == [0, -1, 0] and res["rep_overlap"].tolist() == [4, 0, 4]
    assert res["stats"]["n_unaligned"] == 1 and res["stats"]["n_components"] == 1
    # disjoint residue columns: apart, two singletons
    res = assert_is(ctx, [b"AC--", b"--AC"], [2, 2], 1, 1.0)
    assert res["cluster"].tolist() == [0, 1] and res["stats"]["n_pairs_kept"] == 0 and res["stats"]["n_singletons"] == 2


# ---- 4. compaction -------------------------------------------------------------------------------------------------------------------
def test_compaction_everything_and_nothing(ctx):
    n, M = 300, 37
    rows = [b"ACDEFGHIKLMNPQRSTVWY-ACDEFGHIKLMNPQRS"] * n
    lens = [36] * n
    lens[123] = lens[211] = 40
    got = ctx.row_pairs(rows, 25, 0.01)
    assert len(got["pairs"]) == 44850
    assert pair_list(got) == [(i, j, 0, 36) for i in range(n) for j in range(i + 1, n)]
    res = ctx.cluster(rows, lens, 25, 0.01)
    assert (res["cluster"] == 0).all() and (res["rep"] == 123).all() and (res["rep_diff"] == 0).all() and (res["rep_overlap"] == 36).all()
    st = res["stats"]
    assert (st["n_clusters"], st["n_singletons"], st["largest_cluster"], st["n_components"], st["n_pairs_kept"]) == (1, 0, 300, 1, 44850)
    # nothing kept: any two rows differ in one column of two at least
    rows = [bytes([48 + i // 20, 100 + i % 20]) for i in range(n)]
    got = ctx.row_pairs(rows, 1, 0.01)
    assert len(got["pairs"]) == 0 and got["stats"]["n_pairs_kept"] == 0
    res = ctx.cluster(rows, [2] * n, 1, 0.01)
    assert res["cluster"].tolist() == list(range(n)) and res["rep"].tolist() == list(range(n)) and (res["rep_overlap"] == 2).all()
    assert (res["stats"]["n_clusters"], res["stats"]["n_singletons"], res["stats"]["n_components"]) == (300, 300, 300)


# ---- 5. linkage ----------------------------------------------------------------------------------------------------------------------
def test_linkage_chain_is_not_single_linkage(ctx):
    # A-B and B-C kept, A-C apart because it is beyond the cut-off: {A, B} and {C} by the tie rule
    rows = [b"AAAAAAAAAA", b"AAAAAAAAAC", b"AAAAAAAACC"]
    res = assert_is(ctx, rows, [10] * 3, 1, 0.1)
    assert pair_list(ctx.row_pairs(rows, 1, 0.1)) == [(0, 1, 1, 10), (1, 2, 1, 10)] and res["cluster"].tolist() == [0, 0, 1]
    # ... and because it is below min_overlap
    rows = [b"AAAA----", b"AAAAAAAA", b"----AAAA"]
    res = assert_is(ctx, rows, [4, 8, 4], 2, 0.0)
    assert pair_list(ctx.row_pairs(rows, 2, 0.0)) == [(0, 1, 0, 4), (1, 2, 0, 4)] and res["cluster"].tolist() == [0, 0, 1]
    assert res["rep"].tolist() == [1, 1, 2] and res["stats"]["n_components"] == 1


def test_linkage_ties(ctx):
    # equal distances: the lower min(A) ...
    rows = [b"AAAAAAAAAA", b"AAAAAAAACC", b"AAAAAAAAAC"]
    assert assert_is(ctx, rows, [10] * 3, 1, 0.1)["cluster"].tolist() == [0, 1, 0]
    # ... then the lower min(B)
    rows = [b"AAAAAAAAAC", b"AAAAAAAAAA", b"AAAAAAAACC"]
    assert assert_is(ctx, rows, [10] * 3, 1, 0.1)["cluster"].tolist() == [0, 0, 1]
    # 2/100 and 1/50 are one distance: the tie rule decides, whichever row comes first
    p, y, x = b"A" * 100, b"A" * 98 + b"CC", b"-" * 50 + b"A" * 49 + b"D"
    assert pair_counts(p, y) == (2, 100) and pair_counts(p, x) == (1, 50) and pair_counts(x, y) == (2, 50)
    assert assert_is(ctx, [p, y, x], [100, 100, 50], 25, 0.03)["cluster"].tolist() == [0, 0, 1]
    assert assert_is(ctx, [p, x, y], [100, 50, 100], 25, 0.03)["cluster"].tolist() == [0, 0, 1]


def test_linkage_orders_close_fractions_exactly(ctx):
    """600/60001 and 599/59901 differ by 1 / (60001 * 59901), 2.8e-8 of their value: their fp32 quotients are one number, so a compare
    in single precision would call it a tie and merge rows 0 and 1 by the tie rule.  (Two different fractions of 16-bit counts always
    have different fp64 quotients; what the contract asks for is the exact order, by cross-multiplication.)"""
    M = 60001
    assert np.float32(600) / np.float32(60001) == np.float32(599) / np.float32(59901) and Fraction(599, 59901) < Fraction(600, 60001)
    p = b"A" * M
    x = b"C" * 600 + b"A" * (M - 600)
    y = b"-" * 100 + b"A" * (59901 - 599) + b"D" * 599
    assert pair_counts(p, x) == (600, 60001) and pair_counts(p, y) == (599, 59901) and pair_counts(x, y) == (1099, 59901)
    res = assert_is(ctx, [p, x, y], [M, M, 59901], 25, 0.015)
    assert res["cluster"].tolist() == [0, 1, 0]


def test_linkage_of_one_component(ctx):
    rng = np.random.default_rng(77)
    M, n = 60, 40
    base = np.frombuffer(b"ACDE", dtype=np.uint8)[rng.integers(0, 4, M)]
    rows = []
    for i in range(n):
        r = base.copy()
        hit = rng.choice(M, int(rng.integers(0, 5)), replace=False)
        r[hit] = np.frombuffer(b"FGHI", dtype=np.uint8)[rng.integers(0, 4, hit.size)]
        rows.append(r.tobytes())
    lens = [int(x) for x in rng.integers(50, 70, n)]
    want = restate(rows, lens, 25, 0.07)                                  # up to 4 differences of 60 are kept: some pairs, not all
    assert 0 < len(want[0]) < n * (n - 1) // 2
    res = assert_is(ctx, rows, lens, 25, 0.07, want)
    assert res["stats"]["n_components"] == 1 and 1 < res["stats"]["n_clusters"] < n


# ---- 6. guards -----------------------------------------------------------------------------------------------------------------------
def test_guards(ctx):
    import ctypes as C
    L = ctx._L
    rows = np.frombuffer(b"ACDE" b"ACDC", dtype=np.uint8).copy()
    wide = np.full(2 * 65536, 65, dtype=np.uint8)
    lens = np.array([4, 4], dtype=np.int64)
    cluster, rep = np.full(2, 77, dtype=np.int32), np.full(2, 77, dtype=np.int64)
    rd, ro = np.full(2, 77, dtype=np.uint16), np.full(2, 77, dtype=np.uint16)
    pairs = np.full(4 * 3, 77, dtype=np.int32)
    cnt = C.c_int64(77)
    outs = (cluster.ctypes.data, rep.ctypes.data, rd.ctypes.data, ro.ctypes.data)

    def both(rows_p, n, M, min_overlap, cutoff, word):
        assert L.mgta_rows_pairs(ctx.h, rows_p, n, M, min_overlap, cutoff, pairs.ctypes.data, 4, C.byref(cnt), None) == -1 and word in L.mgta_last_error()
        assert L.mgta_rows_cluster(ctx.h, rows_p, lens.ctypes.data, n, M, min_overlap, cutoff, *outs, None) == -1 and word in L.mgta_last_error()

    both(rows.ctypes.data, 2, 4, 0, 0.5, b"min_overlap")
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        both(rows.ctypes.data, 2, 4, 1, bad, b"cutoff")
    both(wide.ctypes.data, 2, 65536, 1, 0.5, b"65536")
    both(rows.ctypes.data, 2, 0, 1, 0.5, b"M = 0")
    both(None, 2, 4, 1, 0.5, b"rows")
    both(rows.ctypes.data, -1, 4, 1, 0.5, b"n = -1")
    assert L.mgta_rows_pairs(None, rows.ctypes.data, 2, 4, 1, 0.5, pairs.ctypes.data, 4, C.byref(cnt), None) == -1 and b"ctx" in L.mgta_last_error()
    assert L.mgta_rows_pairs(ctx.h, rows.ctypes.data, 2, 4, 1, 0.5, None, 4, C.byref(cnt), None) == -1 and b"pairs" in L.mgta_last_error()
    assert L.mgta_rows_pairs(ctx.h, rows.ctypes.data, 2, 4, 1, 0.5, pairs.ctypes.data, 4, None, None) == -1 and b"n_pairs" in L.mgta_last_error()
    assert L.mgta_rows_pairs(ctx.h, rows.ctypes.data, 2, 4, 1, 0.5, pairs.ctypes.data, -1, C.byref(cnt), None) == -1 and b"cap" in L.mgta_last_error()
    assert L.mgta_rows_cluster(None, rows.ctypes.data, lens.ctypes.data, 2, 4, 1, 0.5, *outs, None) == -1 and b"ctx" in L.mgta_last_error()
    assert L.mgta_rows_cluster(ctx.h, rows.ctypes.data, None, 2, 4, 1, 0.5, *outs, None) == -1 and b"lens" in L.mgta_last_error()
    for i in range(4):
        o = list(outs)
        o[i] = None
        assert L.mgta_rows_cluster(ctx.h, rows.ctypes.data, lens.ctypes.data, 2, 4, 1, 0.5, *o, None) == -1 and b"must not be NULL" in L.mgta_last_error()
    for bad in (-1, 32769):
        assert L.mgta_ctx_set_cluster_tile(ctx.h, bad) == -1 and b"rows_per_tile" in L.mgta_last_error()
    assert L.mgta_ctx_set_cluster_tile(None, 7) == -1 and b"ctx" in L.mgta_last_error()
    # nothing was written by the refused calls
    assert (cluster == 77).all() and (rep == 77).all() and (rd == 77).all() and (ro == 77).all() and (pairs == 77).all() and cnt.value == 77
    # the same arguments with everything in place: a valid call; a buffer too small holds nothing and learns the count
    assert L.mgta_rows_pairs(ctx.h, rows.ctypes.data, 2, 4, 1, 0.5, pairs.ctypes.data, 4, C.byref(cnt), None) == 0
    assert cnt.value == 1 and pairs[:3].tolist() == [0, 1, 1 | 4 << 16] and (pairs[3:] == 77).all()
    three = np.frombuffer(b"ACDE" * 3, dtype=np.uint8).copy()
    pairs[:] = 77
    assert L.mgta_rows_pairs(ctx.h, three.ctypes.data, 3, 4, 1, 0.5, pairs.ctypes.data, 2, C.byref(cnt), None) == 0
    assert cnt.value == 3 and (pairs == 77).all()
    assert L.mgta_rows_cluster(ctx.h, rows.ctypes.data, lens.ctypes.data, 2, 4, 1, 0.5, *outs, None) == 0
    assert cluster.tolist() == [0, 0] and rep.tolist() == [0, 0] and rd.tolist() == [0, 1] and ro.tolist() == [4, 4]
    assert L.mgta_rows_cluster(ctx.h, None, None, 0, 4, 1, 0.5, None, None, None, None, None) == 0
    assert L.mgta_rows_pairs(ctx.h, None, 0, 4, 1, 0.5, None, 0, C.byref(cnt), None) == 0 and cnt.value == 0


# ---- 7. files: one process per call and the worker -----------------------------------------------------------------------------------
def a2m_case(seed):
    """A2M lines with inserted (lower-case) residues, over the rows of random_rows"""
    rows, _ = random_rows(90, 70, seed)
    rng = np.random.default_rng(seed)
    lines = []
    for r in rows:
        s = r.decode()
        if rng.random() < 0.3 and s.strip("-"):
            at = int(rng.integers(1, len(s)))
            s = s[:at] + "kv"[:int(rng.integers(1, 3))] + s[at:]
        lines.append(s)
    headers = [f"c{j} len={j}" if j % 3 else f"c{j}" for j in range(len(lines))]
    nucl = [(f"c{j} x", "ACGT"[j % 4] * (3 + j % 5)) for j in range(len(lines))]
    return headers, lines, nucl


def test_one_shot_and_worker_write_the_same_files(ctx, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    cases = [a2m_case(4), a2m_case(5)]
    for i, (headers, lines, nucl) in enumerate(cases):
        open(tmp_path / f"a{i}.fa", "w").write("".join(f">{h}\n{s}\n" for h, s in zip(headers, lines)))
        open(tmp_path / f"n{i}.fa", "w").write("".join(f">{h}\n{s}\n" for h, s in nucl))
        subprocess.run([BIN, "cluster", str(tmp_path / f"a{i}.fa"), str(tmp_path / f"one{i}"), "0.1", "17", str(tmp_path / f"n{i}.fa"), str(tmp_path / f"one{i}n")],
                       check=True, capture_output=True, timeout=120)
    req = "".join(f"cluster\t{tmp_path}/a{i}.fa\t{tmp_path}/w{i}\t0.1\t17\t{tmp_path}/n{i}.fa\t{tmp_path}/w{i}n\n" for i in range(2)) + "quit\n"
    r = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0", "DONE", "0"], r.stderr[-2000:]
    for i, (headers, lines, nucl) in enumerate(cases):
        rows, lens = cl.rows_and_lens(lines)
        assert lens.tolist() == [len(x.replace("-", "")) for x in lines]
        res = ctx.cluster(rows, lens, 17, 0.1)
        assert res["stats"]["n_unaligned"] > 0 and 1 < res["stats"]["n_clusters"] < len(lines) - res["stats"]["n_unaligned"]
        cl.write_cluster(str(tmp_path / f"py{i}"), headers, lines, res, nucl, str(tmp_path / f"py{i}n"))
        for tail in ("_clust.txt", "_rep_seqs.fasta", "n_rep_seqs.fasta"):
            text = open(f"{tmp_path}/py{i}{tail}").read()
            assert open(f"{tmp_path}/one{i}{tail}").read() == open(f"{tmp_path}/w{i}{tail}").read() == text and len(text) > 0, (i, tail)
        back = cl.read_clust(f"{tmp_path}/one{i}_clust.txt")
        for f in ("cluster", "rep", "rep_diff", "rep_overlap"):
            assert np.array_equal(back[f], res[f]), f
        assert back["lens"].tolist() == lens.tolist() and back["names"] == [al.record_name(h) for h in headers]
        reps = al.parse_aligned_fasta(open(f"{tmp_path}/one{i}_rep_seqs.fasta").read())
        assert reps == [(h, x.replace("-", "").upper()) for j, (h, x) in enumerate(zip(headers, lines)) if res["rep"][j] == j]
    # without the nucleotide pair: the two protein files alone
    subprocess.run([BIN, "cluster", str(tmp_path / "a1.fa"), str(tmp_path / "solo"), "0.1", "17"], check=True, capture_output=True, timeout=120)
    assert open(tmp_path / "solo_clust.txt").read() == open(tmp_path / "one1_clust.txt").read()
    assert open(tmp_path / "solo_rep_seqs.fasta").read() == open(tmp_path / "one1_rep_seqs.fasta").read()
    assert not os.path.exists(tmp_path / "solon_rep_seqs.fasta")
    # a nucleotide file with one name changed, or one record short; a row of another width; a cut-off outside [0, 1]: the step fails and
    # leaves nothing
    text = open(tmp_path / "n1.fa").read()
    for j, bad in enumerate((text.replace(">c7 x\n", ">c7b x\n"), text[:text.rindex(">")])):
        assert bad != text
        open(tmp_path / "bad.fa", "w").write(bad)
        r = subprocess.run([BIN, "cluster", str(tmp_path / "a1.fa"), str(tmp_path / f"bad{j}"), "0.1", "17", str(tmp_path / "bad.fa"), str(tmp_path / f"bad{j}n")],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "cluster" in r.stderr
        assert [f for f in os.listdir(tmp_path) if f.startswith(f"bad{j}")] == []
    open(tmp_path / "narrow.fa", "w").write(">c0\nACDE\n>c1\nACkvDE\n>c2\nACD\n")
    r = subprocess.run([BIN, "cluster", str(tmp_path / "narrow.fa"), str(tmp_path / "bad2"), "0.1", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "record 2" in r.stderr and "columns" in r.stderr
    r = subprocess.run([BIN, "cluster", str(tmp_path / "a1.fa"), str(tmp_path / "bad3"), "1.5", "17"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cutoff" in r.stderr
    assert [f for f in os.listdir(tmp_path) if f.startswith("bad2") or f.startswith("bad3")] == []


# ---- 8. driver end to end ------------------------------------------------------------------------------------------------------------
def test_driver_cluster_end_to_end(golden_dir, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    mg = synth.make_metagenome(6000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)    # the sample of test_driver_align_end_to_end
    synth.write_fasta(mg.reads, str(tmp_path / "reads.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "45", "-t", "4", "--min-contig-len", "150",
                        "-o", str(out), "--derep", "--align", "--cluster"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
    d = out / "contigs" / "rplB"
    table = cl.read_clust(str(d / "prot_merged_rmdup_clust.txt"))
    aligned = al.read_aligned_fasta(str(d / "prot_merged_rmdup_aligned.fasta"))
    prot_reps = al.read_aligned_fasta(str(d / "prot_merged_rmdup_rep_seqs.fasta"))
    nucl_reps = al.read_aligned_fasta(str(d / "nucl_merged_rmdup_rep_seqs.fasta"))
    n = len(aligned)
    assert n > 0 and table["names"] == [al.record_name(h) for h, _ in aligned]
    rows, lens = cl.rows_and_lens([x for _, x in aligned])
    assert table["lens"].tolist() == lens.tolist()
    # every record's counts against its representative, recomputed from the rows, satisfy the kept rule at the defaults (0.01, 25)
    n_reps = 0
    for i in range(n):
        row = rows[i].encode("latin-1")
        if table["status"][i] == 2:
            assert not row.strip(b"-")
            continue
        rep = int(table["rep"][i])
        assert table["cluster"][rep] == table["cluster"][i] and table["status"][rep] == 0 and lens[rep] >= lens[i]
        if rep == i:
            n_reps += 1
            assert (int(table["rep_diff"][i]), int(table["rep_overlap"][i])) == (0, len(row) - row.count(b"-"))
        else:
            got = pair_counts(row, rows[rep].encode("latin-1"))
            assert got == (int(table["rep_diff"][i]), int(table["rep_overlap"][i])) and is_kept(*got, 25, 0.01)
    clusters = table["cluster"][table["status"] != 2]
    assert n_reps == len(set(clusters.tolist())) == len(prot_reps) == len(nucl_reps) and sorted(set(clusters.tolist())) == list(range(n_reps))
    rep_headers = [h for i, (h, _) in enumerate(aligned) if table["status"][i] == 0]
    assert [h for h, _ in prot_reps] == rep_headers
    assert [al.record_name(h) for h, _ in nucl_reps] == [al.record_name(h) for h in rep_headers]
    assert [s for _, s in prot_reps] == [x.replace("-", "").upper() for i, (_, x) in enumerate(aligned) if table["status"][i] == 0]
    # the checkpoints: six of a run without flags, then derep, align, cluster (one gene each)
    assert open(out / "tmp" / "cp.txt").read().splitlines() == [f"{i}\tdone" for i in range(6 + 3)]
    log = open(out / "log").read()
    assert log.count("Clustering the aligned contigs") == 1 and log.index("Aligning the contigs") < log.index("Clustering the aligned contigs")
