"""The host side of the merge tree, no device: mgta_tree_cut on merges made by the Python restatement of the contract
(tests/test_cluster_tree_gpu.py restate_tree) against the restatement's direct run on the pairs kept at the cut-off, the route through
the host linkage included; its guards; the writers and readers of the files; the driver's flag."""
import ctypes as C
import os
import random
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from megagta_amd import _lib, api
from megagta_amd import cluster as cl
from tests import helpers as H
from tests.test_cluster_gpu import GAP, is_kept, restate_link
from tests.test_cluster_host import _fresh_driver
from tests.test_cluster_tree_gpu import restate_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")


def rows_of(n, unaligned=()):
    """rows that only say which records have residues (restate_link reads nothing else of them): 100 columns, or none"""
    return [bytes([GAP]) * 100 if i in unaligned else b"A" * 100 for i in range(n)]


def assert_cut(n, pairs, lens, cutoff, unaligned=(), fallback=None):
    """the cut of the restated tree == the restated linkage of the pairs kept at the cut-off == mgta_pairs_link on them"""
    rows = rows_of(n, unaligned)
    n_res = [0 if i in unaligned else 100 for i in range(n)]
    kept = [p for p in pairs if is_kept(p[2], p[3], 1, cutoff)]
    want = restate_link(rows, lens, kept)
    got = api.tree_cut(pairs, restate_tree(pairs), n_res, lens, cutoff)
    assert (got["cluster"].tolist(), got["rep"].tolist(), got["rep_diff"].tolist(), got["rep_overlap"].tolist()) == want, (pairs, cutoff)
    link = api.link_pairs(kept, n_res, lens)
    for f in ("cluster", "rep", "rep_diff", "rep_overlap"):
        assert got[f].tolist() == link[f].tolist(), f
    st = got["stats"]
    assert st["n_rows"] == n and st["n_pairs"] == len(pairs) and st["n_unaligned"] == len(unaligned)
    for f in ("n_clusters", "n_singletons", "largest_cluster"):
        assert st[f] == link["stats"][f], f
    if fallback is not None:
        assert st["n_cut_fallbacks"] == fallback
    return got


def test_cut_is_the_direct_run_on_random_pair_lists():
    rng = random.Random(7)
    fallbacks = 0
    for _ in range(150):
        n = rng.randint(2, 12)
        density = rng.uniform(0.3, 1.0)
        unaligned = tuple(i for i in range(n) if rng.random() < 0.1)
        pairs = [(i, j, rng.choice([0, 1, 2, 3]), rng.choice([50, 100, 200])) for i in range(n) for j in range(i + 1, n)
                 if i not in unaligned and j not in unaligned and rng.random() < density]                   # ties and equal fractions everywhere
        lens = [rng.randint(1, 3) for _ in range(n)]
        for c in (0.0, 0.01, 0.02, 0.03, 0.06):
            fallbacks += assert_cut(n, pairs, lens, c, unaligned)["stats"]["n_cut_fallbacks"]
    assert fallbacks == 0                                                 # these cut-offs decide equal fractions alike


def test_cut_of_hand_made_lists():
    assert_cut(1, [], [5], 0.5, fallback=0)
    assert_cut(3, [], [5, 5, 5], 0.5, unaligned=(1,), fallback=0)
    pairs = [(0, 1, 1, 100), (0, 2, 3, 100), (1, 2, 2, 100), (2, 3, 0, 100)]
    for c, want in ((0.0, [0, 1, 2, 2]), (0.01, [0, 0, 1, 1]), (0.03, [0, 0, 1, 1]), (1.0, [0, 0, 1, 1])):
        assert assert_cut(4, pairs, [1, 2, 3, 4], c, fallback=0)["cluster"].tolist() == want
    # nothing kept at the cut-off, everything kept
    assert assert_cut(3, [(0, 1, 1, 100), (1, 2, 1, 100)], [1, 1, 1], 0.001, fallback=0)["cluster"].tolist() == [0, 1, 2]
    assert assert_cut(3, [(0, 1, 1, 100), (0, 2, 1, 100), (1, 2, 1, 100)], [1, 1, 9], 0.01, fallback=0)["rep"].tolist() == [2, 2, 2]


def test_cut_where_the_kept_rule_splits_equal_fractions():
    c = float(Fraction(3, 22))
    assert is_kept(3, 22, 1, c) and not is_kept(15, 110, 1, c)
    pairs = [(0, 1, 15, 110), (0, 2, 0, 22), (0, 3, 3, 22), (1, 2, 0, 22), (1, 3, 3, 22), (2, 3, 3, 22)]
    got = assert_cut(4, pairs, [4, 3, 2, 1], c, fallback=1)
    assert got["cluster"].tolist() == [0, 1, 0, 0]                       # the prefix of the tree up to 3 / 22 would put all four together
    assert assert_cut(4, pairs, [4, 3, 2, 1], 0.2, fallback=0)["cluster"].tolist() == [0, 0, 0, 0]
    assert assert_cut(4, pairs, [4, 3, 2, 1], 0.0, fallback=0)["cluster"].tolist() == [0, 1, 0, 2]
    c = 0.09999999999999999
    assert not is_kept(1, 10, 1, c) and is_kept(5, 50, 1, c)
    pairs = [(0, 1, 5, 50), (0, 2, 1, 10), (1, 2, 5, 50)]
    assert assert_cut(3, pairs, [1, 1, 1], c, fallback=1)["cluster"].tolist() == [0, 0, 1]


def test_guards():
    L = _lib.load()
    pairs = np.array([(0, 1, 1, 4), (0, 2, 1, 4), (1, 2, 0, 4)], dtype=api.ROW_PAIR)
    merges = np.array([(1, 2, 0, 1), (0, 1, 1, 4)], dtype=api.TREE_MERGE)
    n_res, lens = np.array([4, 4, 4], dtype=np.int32), np.array([1, 1, 1], dtype=np.int64)
    cluster, rep = np.full(3, 77, dtype=np.int32), np.full(3, 77, dtype=np.int64)
    rd, ro = np.full(3, 77, dtype=np.uint16), np.full(3, 77, dtype=np.uint16)
    outs = [cluster.ctypes.data, rep.ctypes.data, rd.ctypes.data, ro.ctypes.data]

    def refused(word, p=pairs, n_pairs=3, m=merges, n_merges=2, nr=n_res, ln=lens, n=3, cutoff=0.5, o=outs):
        rc = L.mgta_tree_cut(None if p is None else p.ctypes.data, n_pairs, None if m is None else m.ctypes.data, n_merges, None if nr is None else nr.ctypes.data,
                             None if ln is None else ln.ctypes.data, n, cutoff, *o, None)
        assert rc == -1 and word in L.mgta_last_error(), L.mgta_last_error()

    refused(b"n = -1", n=-1)
    refused(b"n_pairs", n_pairs=-1)
    refused(b"pairs", p=None)
    refused(b"n_residues", nr=None)
    refused(b"lens", ln=None)
    for i in range(4):
        refused(b"must not be NULL", o=outs[:i] + [None] + outs[i + 1:])
    for bad in (-0.1, 1.5, float("nan")):
        refused(b"cutoff", cutoff=bad)
    refused(b"pair 1", p=np.array([(0, 1, 1, 4), (0, 3, 1, 4), (1, 2, 0, 4)], dtype=api.ROW_PAIR))
    refused(b"ascend", p=np.array([(0, 2, 1, 4), (0, 1, 1, 4), (1, 2, 0, 4)], dtype=api.ROW_PAIR))
    refused(b"n_residues[0]", nr=np.array([-1, 4, 4], dtype=np.int32))
    refused(b"n_merges", n_merges=3)
    refused(b"n_merges", n_merges=-1)
    refused(b"merges", m=None)
    refused(b"merge 0", m=np.array([(2, 1, 0, 1), (0, 1, 1, 4)], dtype=api.TREE_MERGE))          # a >= b
    refused(b"merge 1", m=np.array([(1, 2, 0, 1), (0, 3, 1, 4)], dtype=api.TREE_MERGE))          # b outside
    refused(b"merge 1", m=np.array([(1, 2, 0, 1), (0, 2, 1, 4)], dtype=api.TREE_MERGE))          # 2 merged twice
    refused(b"merge 0", m=np.array([(1, 2, 0, 0), (0, 1, 1, 4)], dtype=api.TREE_MERGE))          # n_overlap = 0
    refused(b"merge 1", m=np.array([(0, 1, 1, 4), (1, 2, 0, 1)], dtype=api.TREE_MERGE))          # not ascending by the fraction
    assert (cluster == 77).all() and (rep == 77).all() and (rd == 77).all() and (ro == 77).all()
    st = _lib.TreeStats()
    assert L.mgta_tree_cut(pairs.ctypes.data, 3, merges.ctypes.data, 2, n_res.ctypes.data, lens.ctypes.data, 3, 0.0, *outs, C.byref(st)) == 0
    assert cluster.tolist() == [0, 1, 1] and rep.tolist() == [0, 1, 1] and rd.tolist() == [0, 0, 0] and ro.tolist() == [4, 4, 4]
    assert (st.n_rows, st.n_pairs, st.n_merges, st.n_clusters, st.n_singletons, st.largest_cluster, st.n_cut_fallbacks) == (3, 3, 2, 2, 1, 2, 0)
    assert L.mgta_tree_cut(None, 0, None, 0, None, None, 0, 0.5, None, None, None, None, C.byref(st)) == 0 and all(v == 0 for v in st.as_dict().values())


def test_new_symbols_are_declared():
    new = {"mgta_pairs_tree", "mgta_tree_cut", "mgta_rows_clusters"}
    assert new <= set(_lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    for name in new:
        assert f"int {name}(" in hdr
    # the structures of _lib are those of the header, field for field
    fields = H.header_fields("mgta_tree_stats", hdr)
    assert fields == [n for n, _ in _lib.TreeStats._fields_]
    assert C.sizeof(_lib.TreeStats) == 8 * len(fields) and api.TREE_MERGE.itemsize == 12 and api.TREE_MERGE.names == ("a", "b", "n_diff", "n_overlap")


def test_tree_text_round_trip(tmp_path):
    names = ["c0", "c1", "c2", "c3"]
    merges = np.array([(1, 2, 0, 1), (0, 1, 1, 50)], dtype=api.TREE_MERGE)
    text = cl.tree_text(names, merges)
    assert text == "#a_row\tb_row\ta\tb\tn_diff\tn_overlap\n1\t2\tc1\tc2\t0\t1\n0\t1\tc0\tc1\t1\t50\n"
    assert cl.tree_text(names, [(1, 2, 0, 1), (0, 1, 1, 50)]) == text
    back = cl.parse_tree(text)
    assert back["merges"] == [(1, 2, 0, 1), (0, 1, 1, 50)] and back["names"] == {0: "c0", 1: "c1", 2: "c2"}
    assert cl.tree_text(names, back["merges"]) == text
    assert cl.parse_tree(cl.TREE_HEADER) == dict(merges=[], names={})
    for bad in ("", text.replace("#a_row", "#row"), text + "1\t2\tc1\n", text + "3\t2\tc3\tc2\t0\t1\n", text + "2\t3\tc2\tc3\t2\t1\n", text + "2\t3\tother\tc3\t0\t1\n",
                text + "2\t3\tc2\tc3\t0.5\t1\n"):
        with pytest.raises(ValueError, match="tree table"):
            cl.parse_tree(bad)
    # the files of write_cluster_tree: per tag those of write_cluster, and the tree
    headers = ["c0 x", "c1", "c2", "c3"]
    lines = ["AC-", "ACD", "-CD", "---"]
    one = dict(cluster=np.array([0, 0, 1, -1]), rep=np.array([1, 1, 2, -1]), rep_diff=np.array([0, 0, 0, 0]), rep_overlap=np.array([2, 3, 2, 0]))
    two = dict(cluster=np.array([0, 0, 0, -1]), rep=np.array([1, 1, 1, -1]), rep_diff=np.array([0, 0, 0, 0]), rep_overlap=np.array([2, 3, 2, 0]))
    result = {f: np.stack([one[f], two[f]]) for f in one}
    result["merges"] = np.array([(0, 1, 0, 1), (0, 2, 0, 1)], dtype=api.TREE_MERGE)
    nucl = [(h, "ACGT") for h in headers]
    cl.write_cluster_tree(str(tmp_path / "p"), headers, lines, ["0", "0.10"], result, nucl, str(tmp_path / "n"))
    for tag, res in (("0", one), ("0.10", two)):
        cl.write_cluster(str(tmp_path / "q"), headers, lines, res, nucl, str(tmp_path / "qn"))
        for mine, theirs in ((f"p_d{tag}_clust.txt", "q_clust.txt"), (f"p_d{tag}_rep_seqs.fasta", "q_rep_seqs.fasta"), (f"n_d{tag}_rep_seqs.fasta", "qn_rep_seqs.fasta")):
            assert open(tmp_path / mine).read() == open(tmp_path / theirs).read() != ""
    assert cl.read_tree(str(tmp_path / "p_tree.txt"))["merges"] == [(0, 1, 0, 1), (0, 2, 0, 1)]
    with pytest.raises(ValueError, match="one tag"):
        cl.write_cluster_tree(str(tmp_path / "r"), headers, lines, ["0"], result)


def test_cutoff_lists():
    assert cl.parse_cutoff_list("0.03,0.05") == (["0.03", "0.05"], [0.03, 0.05])
    assert cl.parse_cutoff_list("0,.5,0.10") == (["0", ".5", "0.10"], [0.0, 0.5, 0.1])
    for bad, word in (("0.03,0.030", "same number"), ("0.1,1e-1", "1e-1"), ("0.1,", "''"), ("", "''"), ("1.5", "1.5"), ("-0.1", "-0.1"), (".", "'.'"), ("0.1.2", "0.1.2"),
                      ("0.1, 0.2", "' 0.2'")):
        with pytest.raises(ValueError, match=word.replace(".", r"\.")):
            cl.parse_cutoff_list(bad)


def test_cli_prints_the_usage_line():
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    for args in (["clustertree"], ["clustertree", "a", "b", "0.01", "25", "c"]):
        r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage: megagta clustertree <aligned.fasta> <out_prefix> <c1,c2,...> <min_overlap> [<nucl.fasta> <nucl_out_prefix>]" in r.stderr
    r = subprocess.run([BIN, "nosuchstep"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "clustertree" in r.stderr
    # the list is read before any file and before the device
    for bad, word in (("0.03,0.030", "same number"), ("0.03,x", "'x'"), ("2", "'2'")):
        r = subprocess.run([BIN, "clustertree", "/nonexistent/a.fa", "/nonexistent/out", bad, "25"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "[ERROR] clustertree" in r.stderr and word in r.stderr


def test_driver_usage_errors(tmp_path):
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "genes.txt"), "-o", str(tmp_path / "out")]
    r = subprocess.run(base + ["--align", "--cluster-dists", "0.03"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--cluster-dists needs --cluster" in r.stderr
    for bad, word in (("0.03,0.030", "same number"), ("0.03,abc", "'abc'"), ("0.03,1.5", "'1.5'"), ("", "''")):
        r = subprocess.run(base + ["--align", "--cluster", "--cluster-dists", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--cluster-dists" in r.stderr and word in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out")


def test_the_step_of_the_flag_comes_last(tmp_path, monkeypatch):
    """--cluster-dists runs `megagta clustertree` per gene behind every other step, --sample-abund's included, with one checkpoint per
    gene; without the flag the steps and the checkpoints are what they were"""
    def run(dists):
        calls = []
        drv = _fresh_driver(tmp_path, monkeypatch, calls)
        drv.opt.derep = drv.opt.align = drv.opt.cluster = drv.opt.nearest = True
        drv.opt.cluster_min_overlap = 40
        drv.opt.cluster_dists = dists
        if os.path.exists(drv.opt.temp_dir + "cp.txt"):
            os.remove(drv.opt.temp_dir + "cp.txt")
        drv.search_contigs(44)
        drv.after_search(44)
        return drv, calls, open(drv.opt.temp_dir + "cp.txt").read()

    drv, before, cp_before = run(None)
    assert "--cluster-dists" in drv.USAGE and drv.opt.cluster_dists is None
    drv, calls, cp = run("0.03,.05")
    assert calls[:len(before)] == before and [c[1] for c in calls[len(before):]] == ["clustertree"] * 2
    d = drv.opt.out_dir + "contigs/"
    assert calls[len(before):] == [[drv.opt.bin, "clustertree", d + g + "/prot_merged_rmdup_aligned.fasta", d + g + "/prot_merged_rmdup", "0.03,.05", "40",
                                    d + g + "/nucl_merged_rmdup.fasta", d + g + "/nucl_merged_rmdup"] for g in ("rplB", "nirK")]
    n = cp_before.count("\n")
    assert cp.startswith(cp_before) and cp == cp_before + f"{n}\tdone\n{n + 1}\tdone\n"
    # the option comes back from opts.txt
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    with open(drv.opt.out_dir + "opts.txt", "w") as fh:
        fh.write("\n".join(["-r", "reads.fa", "-g", "genes.txt", "--align", "--cluster", "--cluster-dists", "0.03,0.05"]) + "\n")
    drv.parse_opt(["--continue", "-o", str(tmp_path)])
    assert drv.opt.continue_mode and drv.opt.cluster_dists == "0.03,0.05" and drv.cluster_cutoff_tags(drv.opt.cluster_dists) == ["0.03", "0.05"]
