"""Host side of the clustering step, no device: the files (writers and readers), the new symbols, the CLI's usage line, the driver's
`--cluster` options, where the step's checkpoints go and what it is handed."""
import ctypes
import importlib
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from megagta_amd import _lib, api
from megagta_amd import cluster as cl
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")


def sample():
    """five records on a model of 6 columns: a representative, a member with an inserted residue, an unaligned record, a singleton, a
    member in lower-case columns"""
    headers = ["c0 len=5", "c1", "c2 x y", "c3 ", "c4"]
    lines = ["-KVLMA", "MKqVLM-", "------", "---MKV", "-KVlmLM-"]
    result = dict(cluster=np.array([0, 0, -1, 1, 0], dtype=np.int32), rep=np.array([1, 1, -1, 3, 1], dtype=np.int64),
                  rep_diff=np.array([0, 0, 0, 0, 1], dtype=np.uint16), rep_overlap=np.array([4, 5, 0, 3, 4], dtype=np.uint16))
    nucl = [("c0 n", "AAA"), ("c1 n", "CCC"), ("c2", "GGG"), ("c3 n", "TTT"), ("c4", "ACG")]
    return headers, lines, result, nucl


def test_rows_and_lens():
    _, lines, _, _ = sample()
    rows, lens = cl.rows_and_lens(lines)
    assert rows == ["-KVLMA", "MKVLM-", "------", "---MKV", "-KVLM-"] and lens.tolist() == [5, 6, 0, 3, 6]
    with pytest.raises(ValueError, match="record 1 has 4 columns"):
        cl.rows_and_lens(["-KVLMA", "MKqVL"])
    assert cl.unaligned_text("-KVlmLM-") == "KVLMLM" and cl.unaligned_text("--\xe9a-") == "\xe9A"      # ASCII letters only


def test_files_round_trip(tmp_path):
    headers, lines, result, nucl = sample()
    prefix, nprefix = str(tmp_path / "prot_merged"), str(tmp_path / "nucl_merged")
    cl.write_cluster(prefix, headers, lines, result, nucl, nprefix)
    assert open(prefix + "_clust.txt").read() == ("#contig\tstatus\tcluster\trep\tlen\tn_diff\tn_overlap\n"
                                                  "c0\tmember\t0\tc1\t5\t0\t4\n"
                                                  "c1\trep\t0\tc1\t6\t0\t5\n"
                                                  "c2\tunaligned\t-\t-\t0\t0\t0\n"
                                                  "c3\trep\t1\tc3\t3\t0\t3\n"
                                                  "c4\tmember\t0\tc1\t6\t1\t4\n")
    assert open(prefix + "_rep_seqs.fasta").read() == ">c1\nMKQVLM\n>c3 \nMKV\n"                      # header lines as they stood
    assert open(nprefix + "_rep_seqs.fasta").read() == ">c1 n\nCCC\n>c3 n\nTTT\n"
    back = cl.read_clust(prefix + "_clust.txt")
    assert back["names"] == ["c0", "c1", "c2", "c3", "c4"] and back["status"].tolist() == [1, 0, 2, 0, 1] and back["lens"].tolist() == [5, 6, 0, 3, 6]
    for f in ("cluster", "rep", "rep_diff", "rep_overlap"):
        assert np.array_equal(back[f], result[f]) and back[f].dtype == result[f].dtype, f
    assert cl.parse_clust(cl.CLUST_HEADER)["names"] == []
    # without the nucleotide pair: two files
    cl.write_cluster(str(tmp_path / "solo"), headers, lines, result)
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("solo")) == ["solo_clust.txt", "solo_rep_seqs.fasta"]
    # nucleotide records under other names, or one short: an error and no files
    for j, bad in enumerate((nucl[:4], nucl[:3] + [("c9", "TTT")] + nucl[4:])):
        with pytest.raises(ValueError, match="names"):
            cl.write_cluster(str(tmp_path / f"bad{j}"), headers, lines, result, bad, str(tmp_path / f"bad{j}n"))
        assert [f for f in os.listdir(tmp_path) if f.startswith(f"bad{j}")] == []
    H = cl.CLUST_HEADER
    for bad in ("", "c0\trep\t0\tc0\t5\t0\t4\n", H + "c0\tgone\t0\tc0\t5\t0\t4\n", H + "c0\trep\t0\tc0\t5\t0\n", H + "c0\trep\t-\t-\t5\t0\t4\n",
                H + "c0\tunaligned\t0\tc0\t0\t0\t0\n", H + "c0\tmember\t0\tc7\t5\t0\t4\n", H + "c0\trep\t0\tc1\t5\t0\t4\nc1\trep\t1\tc1\t5\t0\t4\n",
                H + "c0\trep\tx\tc0\t5\t0\t4\n", H + "c0\trep\t0\tc0\t5\t-1\t4\n"):
        with pytest.raises(ValueError):
            cl.parse_clust(bad)


def test_new_symbols_are_declared():
    new = {"mgta_rows_pairs", "mgta_rows_cluster", "mgta_ctx_set_cluster_tile"}
    assert new <= set(_lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    for struct, mirror in (("mgta_cluster_stats", _lib.ClusterStats), ("mgta_row_pair", _lib.RowPair)):
        fields = [n for n, _ in mirror._fields_]
        names = H.header_fields(struct, hdr)
        assert names == fields, struct                                    # the ctypes mirror has the header's order
    assert [n for n, _ in _lib.RowPair._fields_] == list(api.ROW_PAIR.names)
    assert ctypes.sizeof(_lib.RowPair) == api.ROW_PAIR.itemsize == 12
    for n in ("n_rows", "n_unaligned", "n_pairs_kept", "n_clusters", "n_singletons", "largest_cluster", "n_components", "ms_pairs", "ms_link"):
        assert n in [f for f, _ in _lib.ClusterStats._fields_]
    lib = _lib.load()                                                     # the library has them (dlopen needs no device)
    assert lib.mgta_rows_pairs and lib.mgta_rows_cluster and lib.mgta_ctx_set_cluster_tile
    for m in ("row_pairs", "cluster", "set_cluster_tile"):
        assert callable(getattr(api.Context, m))


def test_cli_prints_the_usage_line():
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    r = subprocess.run([BIN, "cluster"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage: megagta cluster <aligned.fasta> <out_prefix> <dist_cutoff> <min_overlap> [<nucl.fasta> <nucl_out_prefix>]" in r.stderr
    r = subprocess.run([BIN, "cluster", "a", "b", "0.01", "25", "c"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage: megagta cluster" in r.stderr
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and re.search(r"^\s+cluster\s", r.stderr, re.M)
    r = subprocess.run([BIN, "nosuchstep"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and re.search(r"is not built here \([^)]*\bcluster\b", r.stderr)


def _fresh_driver(tmp_path, monkeypatch, calls):
    from megagta_amd import megagta as drv
    drv = importlib.reload(drv)
    monkeypatch.setattr(drv, "run_step", lambda cmd, what, stdin_path=None, stdout_path=None: calls.append(cmd))
    drv.opt.out_dir = str(tmp_path) + "/"
    drv.opt.temp_dir = drv.opt.out_dir + "tmp/"
    os.makedirs(drv.opt.temp_dir, exist_ok=True)
    drv.opt.lib = drv.opt.temp_dir + "reads.lib"
    drv.opt.gene_info = {"rplB": ("f_rplB.hmm", "r", "a"), "nirK": ("f_nirK.hmm", "r", "a")}
    return drv


def test_driver_accepts_the_options(tmp_path, monkeypatch):
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    assert drv.opt.cluster is False and drv.opt.cluster_dist == 0.01 and drv.opt.cluster_min_overlap == 25
    out = str(tmp_path / "new_out")
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--align", "--cluster"])
    assert drv.opt.cluster is True and drv.opt.align is True and drv.opt.derep is False and (drv.opt.cluster_dist, drv.opt.cluster_min_overlap) == (0.01, 25)
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--align", "--cluster", "--cluster-dist", "0.03", "--cluster-min-overlap", "40"])
    assert drv.opt.cluster is True and (drv.opt.cluster_dist, drv.opt.cluster_min_overlap) == (0.03, 40)
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--align"])
    assert drv.opt.cluster is False and drv.opt.align is True
    for word in ("--cluster ", "--cluster-dist", "--cluster-min-overlap"):
        assert word in drv.USAGE
    # what a finished run wrote into opts.txt brings the options back
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    with open(drv.opt.out_dir + "opts.txt", "w") as fh:
        fh.write("\n".join(["-r", "reads.fa", "-g", "genes.txt", "--align", "--cluster", "--cluster-dist", "0.02"]) + "\n")
    drv.parse_opt(["--continue", "-o", str(tmp_path)])
    assert drv.opt.continue_mode and drv.opt.cluster is True and drv.opt.cluster_dist == 0.02 and drv.opt.cluster_min_overlap == 25


def test_cluster_without_align_is_a_usage_error(tmp_path):
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "genes.txt"), "-o", str(tmp_path / "out")]
    r = subprocess.run(base + ["--cluster"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--cluster needs --align" in r.stderr
    assert not os.path.exists(tmp_path / "out")
    for extra, word in ((["--cluster-dist", "1.5"], "--cluster-dist"), (["--cluster-min-overlap", "0"], "--cluster-min-overlap")):
        r = subprocess.run(base + ["--align", "--cluster"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr


OTHERS = ("coverage", "match_reads", "derep")


@pytest.mark.parametrize("others", list(itertools.product([False, True], repeat=3)), ids=lambda o: "".join("cmd"[i] if x else "-" for i, x in enumerate(o)))
def test_checkpoints_of_the_flag_come_last(tmp_path, monkeypatch, others):
    """the steps of --cluster run behind every step of a run without the flag, behind those of --coverage, --match-reads and --derep and
    behind --align's; one checkpoint per gene; with --derep the files carry _rmdup; without the flag the checkpoint list is unchanged"""
    def set_flags(drv, cluster):
        drv.opt.align, drv.opt.cluster = True, cluster
        drv.opt.coverage, drv.opt.match_reads, drv.opt.derep = others

    calls = []
    drv = _fresh_driver(tmp_path, monkeypatch, calls)
    set_flags(drv, False)
    drv.search_contigs(44)
    drv.after_search(44)
    before = [c[1] for c in calls]
    extra = [s for s, on in zip(("coverage", "matchreads", "derep"), others) if on for _ in range(2)] + ["align"] * 2
    assert before == ["search", "filterbylen", "translate", "filterbylen", "translate"] + extra
    cp_before = open(drv.opt.temp_dir + "cp.txt").read()
    assert cp_before == "".join(f"{i}\tdone\n" for i in range(len(before)))                         # without the flag: what it was
    os.remove(drv.opt.temp_dir + "cp.txt")
    calls.clear()
    drv = _fresh_driver(tmp_path, monkeypatch, calls)
    set_flags(drv, True)
    drv.opt.cluster_dist, drv.opt.cluster_min_overlap = 0.03, 40
    drv.search_contigs(44)
    drv.after_search(44)
    assert [c[1] for c in calls] == before + ["cluster"] * 2
    d = drv.opt.out_dir + "contigs/"
    stem = "_merged_rmdup" if others[2] else "_merged"
    assert calls[-2:] == [[drv.opt.bin, "cluster", d + g + "/prot" + stem + "_aligned.fasta", d + g + "/prot" + stem, "0.03", "40", d + g + "/nucl" + stem + ".fasta",
                           d + g + "/nucl" + stem] for g in ("rplB", "nirK")]
    assert calls[-3][1] == "align" and calls[-3][4] + "_aligned.fasta" == calls[-1][2]             # it reads what --align wrote
    cp = open(drv.opt.temp_dir + "cp.txt").read()
    assert cp.startswith(cp_before) and cp == "".join(f"{i}\tdone\n" for i in range(len(before) + 2))
    # continuing a finished run: nothing runs, every checkpoint is passed.  A search step that is skipped counts one checkpoint (its
    # filters' are written inside it), so past it the flag's two steps are number after + 1 and after + 2
    after = len(before) - 5
    for last_cp, want in ((len(before) + 1, []), (after + 2, []), (after + 1, ["cluster"]), (after, ["cluster"] * 2)):
        calls.clear()
        drv = _fresh_driver(tmp_path, monkeypatch, calls)
        set_flags(drv, True)
        drv.opt.continue_mode, drv.opt.last_cp = True, last_cp
        drv.search_contigs(44)
        drv.after_search(44)
        assert [c[1] for c in calls] == want and drv.cp == 1 + after + 2
