"""The linkage of the clustering step on its own (mgta_pairs_link: host only, no device) against the naive loop of the contract with
fractions.Fraction, the yardstick of tests/test_cluster_gpu.py, and the exact order of fractions of 16-bit counts."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np

from megagta_amd import _lib, api
from tests.test_cluster_gpu import GAP, random_rows, restate_link, restate_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def link(rows, lens, pairs):
    n_res = [sum(1 for x in r if x != GAP) for r in rows]
    return api.link_pairs(pairs, n_res, lens)


def assert_is(res, want):
    cluster, rep, rd, ro = want
    assert res["cluster"].tolist() == cluster and res["rep"].tolist() == rep
    assert res["rep_diff"].tolist() == rd and res["rep_overlap"].tolist() == ro
    sizes = np.bincount(np.array([c for c in cluster if c >= 0] or [0], dtype=np.int64)) if any(c >= 0 for c in cluster) else np.zeros(0, dtype=np.int64)
    st = res["stats"]
    assert (st["n_rows"], st["n_unaligned"], st["n_clusters"]) == (len(cluster), cluster.count(-1), sizes.size)
    assert st["n_singletons"] == int((sizes == 1).sum()) and st["largest_cluster"] == (int(sizes.max()) if sizes.size else 0)


def test_symbol_is_declared():
    assert "mgta_pairs_link" in _lib.SYMBOLS and _lib.load().mgta_pairs_link
    assert re.search(r"\bmgta_pairs_link\s*\(", open(os.path.join(ROOT, "include", "megagta_hip.h")).read())


def test_linkage_equals_the_naive_loop():
    for n, M, min_overlap, cutoff, seed in ((40, 60, 15, 0.1, 1), (65, 64, 16, 0.1, 2), (129, 33, 8, 0.12, 3), (50, 5, 1, 0.0, 4), (30, 40, 10, 1.0, 5)):
        rows, lens = random_rows(n, M, seed)
        pairs = restate_pairs(rows, min_overlap, cutoff)
        assert pairs
        res = link(rows, lens, pairs)
        assert_is(res, restate_link(rows, lens, pairs))
        assert res["stats"]["n_pairs_kept"] == len(pairs) and res["stats"]["n_link_pops"] >= len(pairs)
    # no pairs at all, and no rows
    assert_is(link([b"AC", b"--", b"CA"], [2, 0, 2], []), ([0, -1, 1], [0, -1, 2], [0, 0, 0], [2, 0, 2]))
    assert api.link_pairs([], [], [])["cluster"].size == 0


def test_order_of_fractions_is_exact():
    """rows 0, 1, 2 with the kept pairs (0, 1) at d1 / o1 and (0, 2) at d2 / o2, rows 1 and 2 apart: row 0 merges with row 2 exactly when
    d2 / o2 < d1 / o1 as rationals (a tie goes to the lower row).  Two different fractions of counts below 65536 are at least 2^-32
    apart, so their fp64 quotients differ too; their fp32 quotients often do not, which is where a careless compare would go wrong."""
    rng = np.random.default_rng(11)
    cases, fp32_ties = [], 0
    for _ in range(3000):
        o1 = int(rng.integers(1, 65536))
        d1 = int(rng.integers(0, o1 + 1))
        o2 = int(rng.integers(1, 65536)) if rng.random() < 0.3 else int(np.clip(o1 + rng.integers(-200, 201), 1, 65535))
        d2 = int(np.clip(round(d1 * o2 / o1) + int(rng.integers(-1, 2)), 0, o2))
        cases.append((d1, o1, d2, o2))
    while len(cases) < 3500:                                              # neighbours: d1 * o2 - d2 * o1 = 1, the closest two fractions can be
        o1 = int(rng.integers(40000, 65536))
        d1 = int(rng.integers(1000, o1))
        if np.gcd(d1, o1) != 1:
            continue
        o2 = pow(d1, -1, o1)
        cases.append((d1, o1, (d1 * o2 - 1) // o1, o2) if rng.random() < 0.5 else ((d1 * o2 - 1) // o1, o2, d1, o1))
    cases += [(1, 50, 2, 100), (2, 100, 1, 50), (600, 60001, 599, 59901), (599, 59901, 600, 60001), (0, 1, 0, 65535), (65535, 65535, 1, 1), (65534, 65535, 65533, 65534)]
    for d1, o1, d2, o2 in cases:
        f1, f2 = Fraction(d1, o1), Fraction(d2, o2)
        fp32_ties += f1 != f2 and np.float32(d1) / np.float32(o1) == np.float32(d2) / np.float32(o2)
        res = api.link_pairs([(0, 1, d1, o1), (0, 2, d2, o2)], [65535] * 3, [1, 1, 1])
        assert res["cluster"].tolist() == ([0, 1, 0] if f2 < f1 else [0, 0, 1]), (d1, o1, d2, o2)
    assert fp32_ties > 100                                                # the sample does hold what single precision cannot tell apart


def test_guards():
    L = _lib.load()
    pairs = np.array([(0, 1, 1, 4), (1, 2, 0, 4)], dtype=api.ROW_PAIR)
    n_res, lens = np.array([4, 4, 4], dtype=np.int32), np.array([4, 4, 4], dtype=np.int64)
    cluster, rep = np.full(3, 77, dtype=np.int32), np.full(3, 77, dtype=np.int64)
    rd, ro = np.full(3, 77, dtype=np.uint16), np.full(3, 77, dtype=np.uint16)
    outs = (cluster.ctypes.data, rep.ctypes.data, rd.ctypes.data, ro.ctypes.data)

    def refused(p, n_pairs, nr, ln, n, o, word):
        assert L.mgta_pairs_link(p, n_pairs, nr, ln, n, *o, None) == -1 and word in L.mgta_last_error(), word

    good = (pairs.ctypes.data, 2, n_res.ctypes.data, lens.ctypes.data, 3)
    refused(None, 2, *good[2:], outs, b"pairs")
    refused(good[0], -1, *good[2:], outs, b"n_pairs")
    refused(good[0], 2, None, good[3], 3, outs, b"n_residues")
    refused(good[0], 2, good[2], None, 3, outs, b"lens")
    refused(good[0], 2, good[2], good[3], -1, outs, b"n = -1")
    for i in range(4):
        o = list(outs)
        o[i] = None
        refused(*good, o, b"must not be NULL")
    for bad, word in (([(1, 1, 0, 4)], b"pair 0"), ([(1, 0, 0, 4)], b"pair 0"), ([(0, 3, 0, 4)], b"pair 0"), ([(0, 1, 0, 0)], b"pair 0"), ([(0, 1, 5, 4)], b"pair 0"),
                      ([(-1, 1, 0, 4)], b"pair 0"), ([(0, 2, 0, 4), (0, 1, 0, 4)], b"ascend"), ([(0, 1, 0, 4), (0, 1, 0, 4)], b"ascend")):
        p = np.array(bad, dtype=api.ROW_PAIR)
        refused(p.ctypes.data, len(bad), good[2], good[3], 3, outs, word)
    empty = np.array([4, 0, 4], dtype=np.int32)
    refused(good[0], 2, empty.ctypes.data, good[3], 3, outs, b"residues")                           # a pair of a row without residues
    wide = np.array([4, 65536, 4], dtype=np.int32)
    refused(good[0], 2, wide.ctypes.data, good[3], 3, outs, b"n_residues[1]")
    assert (cluster == 77).all() and (rep == 77).all() and (rd == 77).all() and (ro == 77).all()    # nothing was written by the refused calls
    st = _lib.ClusterStats()
    assert L.mgta_pairs_link(*good, *outs, C.byref(st)) == 0
    assert cluster.tolist() == [0, 1, 1] and rep.tolist() == [0, 1, 1] and rd.tolist() == [0, 0, 0] and ro.tolist() == [4, 4, 4]
    assert (st.n_clusters, st.n_components, st.n_pairs_kept) == (2, 1, 2)
    assert L.mgta_pairs_link(None, 0, None, None, 0, None, None, None, None, None) == 0
