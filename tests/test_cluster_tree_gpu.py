"""mgta_pairs_tree / mgta_tree_cut / mgta_rows_clusters on the device against `restate_tree`, the contract of include/megagta_hip.h
written out in Python: the naive sequential loop with fractions.Fraction (always merge the smallest (distance, lower name, higher name)
among the pairs of clusters whose cross pairs are all kept), every merge recorded as (fraction, a, b), the list then sorted and put in
lowest terms.  Every comparison is exact.  The clusters at a cut-off are compared with the existing route, Context.cluster at that
cut-off, row for row."""
import functools
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from megagta_amd import align as al
from megagta_amd import cluster as cl
from megagta_amd import synth
from tests.test_cluster_gpu import GAP, a2m_case, is_kept, pair_counts, random_rows, restate_link, restate_pairs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------
def restate_tree(pairs):
    """the sequential rule over the kept pairs (i, j, n_diff, n_overlap) -> [(a, b, n_diff, n_overlap)], the fractions in lowest terms (0 as
    0 / 1), sorted by (fraction, a, b).  dist holds the pairs of clusters (named by their lowest rows) whose cross pairs are all kept."""
    dist = {(i, j): Fraction(d, o) for i, j, d, o in pairs}
    merges = []
    while dist:
        f, a, b = min((f, a, b) for (a, b), f in dist.items())
        merges.append((f, a, b))
        new = {k: g for k, g in dist.items() if a not in k and b not in k}
        for x in {x for k in dist for x in k} - {a, b}:
            ka, kb = (min(a, x), max(a, x)), (min(b, x), max(b, x))
            if ka in dist and kb in dist:                                 # linked to both halves: to the union, at the larger distance
                new[ka] = max(dist[ka], dist[kb])
        dist = new
    return [(a, b, f.numerator, f.denominator) for f, a, b in sorted(merges)]


def merge_list(m):
    return list(zip(m["a"].tolist(), m["b"].tolist(), m["n_diff"].tolist(), m["n_overlap"].tolist()))


def residues(n, pairs, unaligned=()):
    return [0 if i in unaligned else 100 for i in range(n)]


def tree_of(ctx, n, pairs, unaligned=()):
    res = ctx.pairs_tree(pairs, residues(n, pairs, unaligned))
    st = res["stats"]
    assert st["n_rows"] == n and st["n_pairs"] == len(pairs) and st["n_merges"] == len(res["merges"])
    return merge_list(res["merges"]), st


def assert_tree(ctx, n, pairs, unaligned=(), what=""):
    got, st = tree_of(ctx, n, pairs, unaligned)
    assert got == restate_tree(pairs), what
    assert (st["n_rounds"] == 0) == (len(got) == 0) and st["n_rounds"] <= max(0, n - 1)
    return got, st


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


# ---- 1. hand-made pair lists ---------------------------------------------------------------------------------------------------------
def test_tree_of_hand_made_pairs(ctx):
    assert assert_tree(ctx, 1, [])[0] == []
    assert assert_tree(ctx, 2, [(0, 1, 3, 100)])[0] == [(0, 1, 3, 100)]
    assert assert_tree(ctx, 2, [])[0] == []
    # a chain x - y - z where only neighbours are kept: y goes with the closer one, the other stays (single linkage would take all three)
    assert assert_tree(ctx, 3, [(0, 1, 2, 100), (1, 2, 1, 100)])[0] == [(1, 2, 1, 100)]
    # close fractions: 599 / 59901 < 600 / 60001, the cross products differ by 1 (equal as fp32, and the lower pair has the larger one)
    assert Fraction(599, 59901) < Fraction(600, 60001) and 600 * 59901 - 599 * 60001 == 1
    assert assert_tree(ctx, 4, [(0, 1, 600, 60001), (2, 3, 599, 59901)])[0] == [(2, 3, 599, 59901), (0, 1, 600, 60001)]
    # equal fractions with different denominators: lowest terms, the order by the names; 0 is 0 / 1
    assert assert_tree(ctx, 6, [(0, 1, 2, 100), (2, 3, 1, 50), (4, 5, 0, 77)])[0] == [(4, 5, 0, 1), (0, 1, 1, 50), (2, 3, 1, 50)]
    # the distance of a union is the largest cross fraction, also when a smaller denominator attains it
    assert assert_tree(ctx, 3, [(0, 1, 0, 90), (0, 2, 2, 100), (1, 2, 3, 150)])[0] == [(0, 1, 0, 1), (0, 2, 1, 50)]
    # rows without residues between the others
    assert assert_tree(ctx, 5, [(1, 3, 1, 100)], unaligned=(0, 2))[0] == [(1, 3, 1, 100)]


# ---- 2. two merges in one round ------------------------------------------------------------------------------------------------------
def test_two_merges_in_one_round(ctx):
    a, b, c, d, e = range(5)
    close = [(a, b, 0, 100), (c, d, 0, 100)]                               # mutual pairs of the first round
    # b - d apart: the two unions are not linked, whatever the other three say
    got, st = assert_tree(ctx, 4, sorted(close + [(a, c, 1, 100), (a, d, 1, 100), (b, c, 1, 100)]))
    assert got == [(a, b, 0, 1), (c, d, 0, 1)] and st["n_rounds"] == 1
    # all four kept: the unions merge at the largest of the four
    got, st = assert_tree(ctx, 4, sorted(close + [(a, c, 1, 100), (a, d, 3, 100), (b, c, 1, 50), (b, d, 1, 100)]))
    assert got == [(a, b, 0, 1), (c, d, 0, 1), (a, c, 3, 100)] and st["n_rounds"] == 2
    # e is linked to c and not to d: after the round it is linked to nothing
    got, st = assert_tree(ctx, 5, sorted(close + [(c, e, 1, 100)]))
    assert got == [(a, b, 0, 1), (c, d, 0, 1)] and st["n_rounds"] == 1
    # e linked to both halves of one union and to one of the other
    got, _ = assert_tree(ctx, 5, sorted(close + [(c, e, 1, 100), (d, e, 2, 100), (a, e, 1, 100)]))
    assert got == [(a, b, 0, 1), (c, d, 0, 1), (c, e, 1, 50)]


# ---- 3. ties -------------------------------------------------------------------------------------------------------------------------
def test_cliques_at_one_distance(ctx):
    n = 70                                                                # more than one wave of names
    zero = [(i, j, 0, 64) for i in range(n) for j in range(i + 1, n)]
    got, st = assert_tree(ctx, n, zero)
    assert got == [(0, j, 0, 1) for j in range(1, n)] and 1 <= st["n_rounds"] <= n - 1
    # beside it a clique at 2 / 100 whose pairs are written in three ways, and no link between the two
    m = 9
    ways = [(2, 100), (1, 50), (4, 200)]
    both = zero + [(n + i, n + j) + ways[(i + j) % 3] for i in range(m) for j in range(i + 1, m)]
    got, st = assert_tree(ctx, n + m, both)
    assert got == [(0, j, 0, 1) for j in range(1, n)] + [(n, n + j, 1, 50) for j in range(1, m)] and 1 <= st["n_rounds"] <= n + m - 1
    assert st["n_lists_rewritten"] >= n - 1 and st["n_entries_visited"] >= 2 * len(both)


# ---- 4. list-length edges ------------------------------------------------------------------------------------------------------------
def star(k):
    """row 0 with k neighbours at distinct distances, the neighbours apart from each other, and a row without any pair"""
    return k + 2, [(0, j, j, 400) for j in range(1, k + 1)]


@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 300])
def test_a_list_of_k_entries(ctx, k):
    n, pairs = star(k)
    got, st = assert_tree(ctx, n, pairs)
    assert got == ([(0, 1, 1, 400)] if k else []) and st["n_rounds"] == (1 if k else 0)
    # the same list on the last row: every entry points down
    pairs = [(j, n - 1, j + 1, 400) for j in range(k)]
    assert assert_tree(ctx, n, pairs)[0] == ([(0, n - 1, 1, 400)] if k else [])


ROWS = {(n, M): random_rows(n, M, 1000 + n) for n, M in ((63, 40), (64, 57), (65, 64), (129, 80), (300, 120))}
CUTS = [0.0, 0.01, 0.03, 0.05, 0.1]
SMALL = 129                                                               # up to here the Python restatement of the tree is quick enough


@functools.lru_cache(maxsize=None)
def want_pairs(n, M):
    return restate_pairs(ROWS[(n, M)][0], M // 4, 0.1)


@functools.lru_cache(maxsize=None)
def want_tree(n, M):
    return restate_tree(want_pairs(n, M))


def test_the_inputs_have_rows_without_residues():
    assert sum(not r.strip(b"-") for rows, _ in ROWS.values() for r in rows) >= 3


@pytest.mark.parametrize("n,M", sorted(ROWS))
def test_random_rows(ctx, n, M):
    rows, lens = ROWS[(n, M)]
    got = ctx.row_pairs(rows, M // 4, 0.1)["pairs"]
    pairs = list(zip(got["i"].tolist(), got["j"].tolist(), got["n_diff"].tolist(), got["n_overlap"].tolist()))
    assert pairs == want_pairs(n, M) and len(pairs) > n
    n_res = [len(r) - r.count(b"-") for r in rows]
    res = ctx.pairs_tree(got, n_res)
    if n <= SMALL:
        assert merge_list(res["merges"]) == want_tree(n, M)
    assert 1 <= res["stats"]["n_rounds"] <= n - 1
    again = ctx.pairs_tree(got, n_res)                                    # nothing depends on the order the device worked in
    assert merge_list(again["merges"]) == merge_list(res["merges"])
    for f in ("n_rounds", "n_entries_visited", "n_lists_rewritten", "n_merges"):
        assert again["stats"][f] == res["stats"][f], f


# ---- 5. cuts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,M", sorted(ROWS))
def test_cuts_equal_the_existing_route(ctx, n, M):
    from megagta_amd import api
    rows, lens = ROWS[(n, M)]
    res = ctx.clusters(rows, lens, M // 4, CUTS)
    st = res["stats"]
    assert st["n_cut_fallbacks"] == 0 and st["n_rows"] == n and st["n_merges"] == len(res["merges"])
    assert res["cluster"].shape == (len(CUTS), n)
    n_res = [len(r) - r.count(b"-") for r in rows]
    all_pairs = want_pairs(n, M)
    if n <= SMALL:
        assert merge_list(res["merges"]) == want_tree(n, M)
    for k, c in enumerate(CUTS):
        want = ctx.cluster(rows, lens, M // 4, c)
        for f in ("cluster", "rep", "rep_diff", "rep_overlap"):
            assert res[f][k].tolist() == want[f].tolist(), (c, f)
        kept = [p for p in all_pairs if is_kept(p[2], p[3], M // 4, c)]
        if n <= 65:
            cluster, rep, rd, ro = restate_link(rows, lens, kept)
            assert (res["cluster"][k].tolist(), res["rep"][k].tolist(), res["rep_diff"][k].tolist(), res["rep_overlap"][k].tolist()) == (cluster, rep, rd, ro), c
        one = api.tree_cut(all_pairs, res["merges"], n_res, lens, c)      # the cut alone gives the same, and so does the host linkage on the kept pairs
        two = api.link_pairs(kept, n_res, lens)
        for f in ("cluster", "rep", "rep_diff", "rep_overlap"):
            assert one[f].tolist() == two[f].tolist() == want[f].tolist(), (c, f)
        assert one["stats"]["n_cut_fallbacks"] == 0
    last = ctx.cluster(rows, lens, M // 4, CUTS[-1])["stats"]
    for f in ("n_unaligned", "n_clusters", "n_singletons", "largest_cluster"):
        assert st[f] == last[f], f
    assert st["n_merges"] == n - st["n_unaligned"] - st["n_clusters"]     # aligned rows - clusters at D


def test_three_thousand_rows(ctx):
    from megagta_amd import api
    n, M = 3000, 120
    rows, lens = random_rows(n, M, 77)
    n_res = [len(r) - r.count(b"-") for r in rows]
    cuts = [0.02, 0.05, 0.1]
    res = ctx.clusters(rows, lens, M // 4, cuts)
    assert res["stats"]["n_cut_fallbacks"] == 0 and res["stats"]["n_pairs"] > 100 * n
    pairs = ctx.row_pairs(rows, M // 4, 0.1)["pairs"]
    assert len(pairs) == res["stats"]["n_pairs"]
    for k, c in enumerate(cuts):
        kept = pairs[pairs["n_diff"].astype(np.float64) <= c * pairs["n_overlap"].astype(np.float64)]
        want = api.link_pairs(kept, n_res, lens)
        for f in ("cluster", "rep", "rep_diff", "rep_overlap"):
            assert np.array_equal(res[f][k], want[f]), (c, f)
    m = res["merges"]
    assert len(m) == n - res["stats"]["n_unaligned"] - res["stats"]["n_clusters"] and (m["a"] < m["b"]).all() and len(set(m["b"].tolist())) == len(m)
    assert (np.gcd(m["n_diff"].astype(np.int64), m["n_overlap"].astype(np.int64)) == 1).all()
    keys = [(Fraction(int(d), int(o)), int(a), int(b)) for a, b, d, o in merge_list(m)]
    assert keys == sorted(keys)
    assert 1 <= res["stats"]["n_rounds"] <= n - 1


# ---- 6. the anomaly: one rounded product decides equal fractions differently ----------------------------------------------------------
def anomaly_rows():
    """four rows of 110 columns in one would-be cluster: rows 0 and 1 overlap in 110 columns and differ in 15; rows 2 and 3 hold 22
    columns, row 2 equal to rows 0 and 1 there, row 3 different in 3 of them from all three"""
    M = 110
    r0 = bytearray(b"A" * M)
    r1 = bytearray(b"A" * M)
    for k in range(15):
        r1[30 + k] = ord("C")                                            # 15 / 110 against row 0
    r2 = bytearray(b"-" * M)
    r2[:22] = b"A" * 22                                                  # 0 / 22 against rows 0 and 1
    r3 = bytearray(b"-" * M)
    r3[:22] = b"A" * 19 + b"CCC"                                         # 3 / 22 against rows 0, 1 and 2
    return [bytes(r0), bytes(r1), bytes(r2), bytes(r3)], [4, 3, 2, 1]


def test_the_cut_does_not_assume_a_monotone_kept_rule(ctx):
    from megagta_amd import _lib, api
    rows, lens = anomaly_rows()
    c = float(Fraction(3, 22))
    assert Fraction(3, 22) == Fraction(15, 110) and is_kept(3, 22, 22, c) and not is_kept(15, 110, 22, c)
    assert pair_counts(rows[0], rows[1]) == (15, 110) and pair_counts(rows[2], rows[3]) == (3, 22) and pair_counts(rows[0], rows[3]) == (3, 22)
    res = ctx.clusters(rows, lens, 22, [0.2, c, 0.0])
    assert res["stats"]["n_cut_fallbacks"] >= 1
    for k, cut in enumerate([0.2, c, 0.0]):
        want = ctx.cluster(rows, lens, 22, cut)
        for f in ("cluster", "rep", "rep_diff", "rep_overlap"):
            assert res[f][k].tolist() == want[f].tolist(), (cut, f)
        pairs = restate_pairs(rows, 22, cut)
        assert (res["cluster"][k].tolist(), res["rep"][k].tolist(), res["rep_diff"][k].tolist(), res["rep_overlap"][k].tolist()) == restate_link(rows, lens, pairs)
    assert res["cluster"][0].tolist() == [0, 0, 0, 0] and res["cluster"][1].tolist() != res["cluster"][0].tolist()
    # the cut alone, on the pairs at D = 0.2
    at_d = ctx.row_pairs(rows, 22, 0.2)["pairs"]
    one = api.tree_cut(at_d, res["merges"], [110, 110, 22, 22], lens, c)
    assert one["stats"]["n_cut_fallbacks"] == 1 and one["cluster"].tolist() == res["cluster"][1].tolist()
    # a cut-off outside [0, 1] is refused
    with pytest.raises(_lib.MegaGtaError, match="cutoff"):
        ctx.clusters(rows, lens, 22, [0.2, 1.5])
    with pytest.raises(_lib.MegaGtaError, match="cutoff"):
        api.tree_cut(at_d, res["merges"], [110, 110, 22, 22], lens, 1.5)


# ---- 7. guards -----------------------------------------------------------------------------------------------------------------------
def test_guards(ctx):
    import ctypes as C
    from megagta_amd import _lib, api
    L = ctx._L
    n_res = np.array([4, 4, 4], dtype=np.int32)
    merges = np.full(3 * 3, 77, dtype=np.int32)
    cnt = C.c_int64(77)

    def refused(pairs, n, word, nr=n_res, ctx_h=ctx.h, cap=3, out=merges.ctypes.data, count=C.byref(cnt)):
        p = np.array(pairs, dtype=api.ROW_PAIR) if pairs is not None else None
        rc = L.mgta_pairs_tree(ctx_h, p.ctypes.data if p is not None and p.size else None, 0 if p is None else p.size, None if nr is None else nr.ctypes.data, n, out, cap, count,
                               None)
        assert rc == -1 and word in L.mgta_last_error(), (pairs, L.mgta_last_error())

    good = [(0, 1, 1, 4), (0, 2, 1, 4)]
    refused(good, 3, b"ctx", ctx_h=None)
    refused(good, -1, b"n = -1")
    refused(good, 3, b"n_residues", nr=None)
    refused(good, 3, b"cap", cap=-1)
    refused(good, 3, b"merges", out=None)
    refused(good, 3, b"n_merges", count=None)
    refused([(0, 3, 1, 4)], 3, b"pair 0")                                 # j outside
    refused([(1, 1, 1, 4)], 3, b"pair 0")                                 # i = j
    refused([(-1, 1, 1, 4)], 3, b"pair 0")
    refused([(0, 1, 1, 0)], 3, b"pair 0")                                 # n_overlap = 0
    refused([(0, 1, 5, 4)], 3, b"pair 0")                                 # n_diff > n_overlap
    refused([(0, 2, 1, 4), (0, 1, 1, 4)], 3, b"ascend")
    refused([(0, 1, 1, 4), (0, 1, 1, 4)], 3, b"ascend")
    refused(good, 3, b"pair 1", nr=np.array([4, 4, 0], dtype=np.int32))   # a row of a pair without residues
    refused(good, 3, b"n_residues[1]", nr=np.array([4, 65536, 4], dtype=np.int32))
    assert L.mgta_pairs_tree(ctx.h, None, 2, n_res.ctypes.data, 3, merges.ctypes.data, 3, C.byref(cnt), None) == -1 and b"pairs" in L.mgta_last_error()
    assert (merges == 77).all() and cnt.value == 77                      # nothing was written by the refused calls
    # a buffer too small holds nothing and learns the count; one that fits holds the list
    p = np.array(good + [(1, 2, 0, 4)], dtype=api.ROW_PAIR)
    st = _lib.TreeStats()
    assert L.mgta_pairs_tree(ctx.h, p.ctypes.data, 3, n_res.ctypes.data, 3, merges.ctypes.data, 1, C.byref(cnt), C.byref(st)) == 0
    assert cnt.value == 2 and (merges == 77).all() and st.n_merges == 2
    assert L.mgta_pairs_tree(ctx.h, p.ctypes.data, 3, n_res.ctypes.data, 3, None, 0, C.byref(cnt), None) == 0 and cnt.value == 2
    assert L.mgta_pairs_tree(ctx.h, p.ctypes.data, 3, n_res.ctypes.data, 3, merges.ctypes.data, 3, C.byref(cnt), None) == 0
    assert cnt.value == 2 and merges[:6].tolist() == [1, 2, 0 | 1 << 16, 0, 1, 1 | 4 << 16] and (merges[6:] == 77).all()
    # n = 0
    assert L.mgta_pairs_tree(ctx.h, None, 0, None, 0, None, 0, C.byref(cnt), C.byref(st)) == 0 and cnt.value == 0
    assert all(v == 0 for v in st.as_dict().values())
    tenth, nan = np.array([0.1]), np.array([float("nan")])
    assert L.mgta_rows_clusters(ctx.h, None, None, 0, 4, 1, tenth.ctypes.data, 1, None, None, None, None, None, None, C.byref(st)) == 0
    assert all(v == 0 for v in st.as_dict().values())
    # mgta_rows_clusters: the guards of mgta_rows_cluster, and the list of cut-offs
    rows = np.frombuffer(b"ACDE" b"ACDC", dtype=np.uint8).copy()
    lens = np.array([4, 4], dtype=np.int64)
    cluster, rep = np.full(2, 77, dtype=np.int32), np.full(2, 77, dtype=np.int64)
    rd, ro = np.full(2, 77, dtype=np.uint16), np.full(2, 77, dtype=np.uint16)
    outs = (cluster.ctypes.data, rep.ctypes.data, rd.ctypes.data, ro.ctypes.data)
    half = np.array([0.5])
    for args, word in (((None, rows.ctypes.data, lens.ctypes.data, 2, 4, 1, half.ctypes.data, 1), b"ctx"), ((ctx.h, None, lens.ctypes.data, 2, 4, 1, half.ctypes.data, 1), b"rows"),
                       ((ctx.h, rows.ctypes.data, None, 2, 4, 1, half.ctypes.data, 1), b"lens"), ((ctx.h, rows.ctypes.data, lens.ctypes.data, 2, 0, 1, half.ctypes.data, 1), b"M = 0"),
                       ((ctx.h, rows.ctypes.data, lens.ctypes.data, 2, 4, 0, half.ctypes.data, 1), b"min_overlap"),
                       ((ctx.h, rows.ctypes.data, lens.ctypes.data, 2, 4, 1, half.ctypes.data, 0), b"n_cutoffs"), ((ctx.h, rows.ctypes.data, lens.ctypes.data, 2, 4, 1, None, 1), b"cutoffs"),
                       ((ctx.h, rows.ctypes.data, lens.ctypes.data, 2, 4, 1, nan.ctypes.data, 1), b"cutoff")):
        assert L.mgta_rows_clusters(*args, *outs, None, None, None) == -1 and word in L.mgta_last_error(), word
    assert (cluster == 77).all() and (rep == 77).all() and (rd == 77).all() and (ro == 77).all()
    assert L.mgta_rows_clusters(ctx.h, rows.ctypes.data, lens.ctypes.data, 2, 4, 1, half.ctypes.data, 1, *outs, None, None, None) == 0
    assert cluster.tolist() == [0, 0] and rep.tolist() == [0, 0] and rd.tolist() == [0, 1] and ro.tolist() == [4, 4]


# ---- 8. files: one process per call, the worker, the driver --------------------------------------------------------------------------
def test_one_shot_and_worker_write_the_same_files(ctx, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    headers, lines, nucl = a2m_case(4)
    open(tmp_path / "a.fa", "w").write("".join(f">{h}\n{s}\n" for h, s in zip(headers, lines)))
    open(tmp_path / "n.fa", "w").write("".join(f">{h}\n{s}\n" for h, s in nucl))
    tags = ["0.03", "0.1", "0", ".05"]
    subprocess.run([BIN, "clustertree", str(tmp_path / "a.fa"), str(tmp_path / "one"), ",".join(tags), "17", str(tmp_path / "n.fa"), str(tmp_path / "onen")], check=True,
                   capture_output=True, timeout=120)
    req = f"clustertree\t{tmp_path}/a.fa\t{tmp_path}/w\t{','.join(tags)}\t17\t{tmp_path}/n.fa\t{tmp_path}/wn\nquit\n"
    r = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0"], r.stderr[-2000:]
    rows, lens = cl.rows_and_lens(lines)
    res = ctx.clusters(rows, lens, 17, [float(t) for t in tags])
    cl.write_cluster_tree(str(tmp_path / "py"), headers, lines, tags, res, nucl, str(tmp_path / "pyn"))
    for tag in tags:
        subprocess.run([BIN, "cluster", str(tmp_path / "a.fa"), str(tmp_path / f"c{tag}"), tag, "17", str(tmp_path / "n.fa"), str(tmp_path / f"c{tag}n")], check=True,
                       capture_output=True, timeout=120)
        for tail, ctail in ((f"_d{tag}_clust.txt", "_clust.txt"), (f"_d{tag}_rep_seqs.fasta", "_rep_seqs.fasta"), (f"n_d{tag}_rep_seqs.fasta", "n_rep_seqs.fasta")):
            text = open(f"{tmp_path}/c{tag}{ctail}").read()
            assert open(f"{tmp_path}/one{tail}").read() == open(f"{tmp_path}/w{tail}").read() == open(f"{tmp_path}/py{tail}").read() == text and len(text) > 0, tail
    assert len({open(f"{tmp_path}/one_d{tag}_clust.txt").read() for tag in tags}) > 1
    tree = open(tmp_path / "one_tree.txt").read()
    assert tree == open(tmp_path / "w_tree.txt").read() == open(tmp_path / "py_tree.txt").read() and tree.count("\n") == 1 + len(res["merges"]) > 1
    back = cl.read_tree(str(tmp_path / "one_tree.txt"))
    names = [al.record_name(h) for h in headers]
    assert back["merges"] == merge_list(res["merges"]) and all(names[i] == name for i, name in back["names"].items())
    assert cl.tree_text(names, back["merges"]) == tree and "." not in "".join(x.split("\t", 4)[4] for x in tree.splitlines()[1:])
    # bad items, the same number twice, a cut-off above 1: the step fails and leaves nothing
    for j, (bad, word) in enumerate((("0.03,0.030", "same number"), ("0.03,1e-2", "1e-2"), ("0.03,,0.1", "''"), ("1.5", "1.5"), ("0.03,-0.1", "-0.1"), (".", "'.'"))):
        r = subprocess.run([BIN, "clustertree", str(tmp_path / "a.fa"), str(tmp_path / f"bad{j}"), bad, "17"], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "clustertree" in r.stderr and word in r.stderr, (bad, r.stderr)
    assert [f for f in os.listdir(tmp_path) if f.startswith("bad")] == []
    # without the nucleotide pair
    subprocess.run([BIN, "clustertree", str(tmp_path / "a.fa"), str(tmp_path / "solo"), "0.1", "17"], check=True, capture_output=True, timeout=120)
    assert open(tmp_path / "solo_d0.1_clust.txt").read() == open(tmp_path / "one_d0.1_clust.txt").read() and open(tmp_path / "solo_tree.txt").read() == tree
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("solo")) == ["solo_d0.1_clust.txt", "solo_d0.1_rep_seqs.fasta", "solo_tree.txt"]


def test_driver_cluster_dists_end_to_end(golden_dir, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    from megagta_amd import samplecov, taxonabund
    mg = synth.make_metagenome(6000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)    # the sample of test_driver_cluster_end_to_end
    synth.write_fasta(mg.reads, str(tmp_path / "reads.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "45", "-t", "4", "--min-contig-len", "150", "--derep",
            "--align", "--cluster", "--taxon-abund", "--sample-abund"]
    for out, extra in ((tmp_path / "plain", []), (tmp_path / "out", ["--cluster-dists", "0.03,0.05"])):
        r = subprocess.run(base + ["-o", str(out)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
    out = tmp_path / "out"
    plain, tree = tmp_path / "plain" / "contigs" / "rplB", out / "contigs" / "rplB"
    before = sorted(os.listdir(plain))
    new = ["prot_merged_rmdup_tree.txt"] + [f"{kind}_merged_rmdup_d{tag}{tail}" for tag in ("0.03", "0.05") for kind, tail in (
        ("prot", "_clust.txt"), ("prot", "_rep_seqs.fasta"), ("nucl", "_rep_seqs.fasta"), ("prot", "_otu_abund.txt"), ("prot", "_otu_samples.txt"),
        ("prot", "_otu_samples_ppm.txt"))]
    assert sorted(os.listdir(tree)) == sorted(before + new)
    for f in before:                                                      # every file of the run without the flag, byte for byte
        assert open(tree / f, "rb").read() == open(plain / f, "rb").read(), f
    cp_plain = open(tmp_path / "plain" / "tmp" / "cp.txt").read().splitlines()
    cp_tree = open(out / "tmp" / "cp.txt").read().splitlines()
    assert cp_tree == cp_plain + [f"{len(cp_plain)}\tdone"]               # one checkpoint per gene, at the end
    log = open(out / "log").read()
    assert log.count("Clustering the aligned contigs of rplB at 2 cut-offs") == 1 and log.index("per library") < log.index("at 2 cut-offs")
    assert "cut-offs" not in open(tmp_path / "plain" / "log").read()
    for tag in ("0.03", "0.05"):                                          # each is what `megagta cluster` writes at that cut-off
        subprocess.run([BIN, "cluster", str(tree / "prot_merged_rmdup_aligned.fasta"), str(tmp_path / f"c{tag}"), tag, "25", str(tree / "nucl_merged_rmdup.fasta"),
                        str(tmp_path / f"c{tag}n")], check=True, capture_output=True, timeout=120)
        for mine, theirs in ((f"prot_merged_rmdup_d{tag}_clust.txt", f"c{tag}_clust.txt"), (f"prot_merged_rmdup_d{tag}_rep_seqs.fasta", f"c{tag}_rep_seqs.fasta"),
                             (f"nucl_merged_rmdup_d{tag}_rep_seqs.fasta", f"c{tag}n_rep_seqs.fasta")):
            assert open(tree / mine, "rb").read() == open(tmp_path / theirs, "rb").read(), mine
    # the clusters get coarser with the cut-off, and every table sums to the mass of the primary one
    counts = [len(set(cl.read_clust(str(tree / f"prot_merged_rmdup{t}_clust.txt"))["cluster"].tolist())) for t in ("", "_d0.03", "_d0.05")]
    assert counts[0] >= counts[1] >= counts[2] >= 1
    total = sum(r["mass"] for r in taxonabund.read_otu(str(tree / "prot_merged_rmdup_otu_abund.txt")))
    per_lib = [sum(col) for col in zip(*(r["mass"] for r in samplecov.read_otu_samples(str(tree / "prot_merged_rmdup_otu_samples.txt"))["rows"]))]
    assert total > 0
    for tag in ("0.03", "0.05"):
        assert sum(r["mass"] for r in taxonabund.read_otu(str(tree / f"prot_merged_rmdup_d{tag}_otu_abund.txt"))) == total
        assert [sum(col) for col in zip(*(r["mass"] for r in samplecov.read_otu_samples(str(tree / f"prot_merged_rmdup_d{tag}_otu_samples.txt"))["rows"]))] == per_lib
        back = cl.read_clust(str(tree / f"prot_merged_rmdup_d{tag}_clust.txt"))
        assert back["names"] == cl.read_clust(str(tree / "prot_merged_rmdup_clust.txt"))["names"]
