"""Host side of the nearest-reference step, no device: the files (writers and readers), reference reading, the scoring parsers, the new
symbols, the CLI's usage line, the driver's `--nearest` options, where the step's checkpoints go and what it is handed."""
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
from megagta_amd import nearest as nr
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")


def sample():
    """four contigs against three references: two contigs on reference 2, an unaligned one, one on reference 0; reference 1 has none"""
    headers, seqs = ["c0 len=5", "c1", "c2 x y", "c3 "], ["MKVLA", "MKVL", "", "KVLMAQ"]
    ref_names, ref_seqs = ["r0", "r1", "r2"], ["KVLMAQW", "WWWW", "AMKVLAA"]
    recs = np.array([(0, 2, 25, 2, 6, 5, 5, 0, 0), (0, 2, 11, 2, 6, 4, 3, 0, 1), (1, -1, 0, 0, 0, 0, 0, 0, 0), (0, 0, 17, 1, 6, 5, 5, 1, 0)], dtype=nr.REC)
    return headers, seqs, ref_names, ref_seqs, dict(recs=recs)


def test_files_round_trip(tmp_path):
    headers, seqs, ref_names, ref_seqs, result = sample()
    prefix = str(tmp_path / "prot_merged")
    nr.write_nearest(prefix, headers, seqs, ref_names, ref_seqs, result)
    assert open(prefix + "_nearest.txt").read() == (
        "#contig\tstatus\tref\tscore\tidentity\tlen\tref_len\tref_from\tref_to\tmatch\tident\tinsert\tdelete\n"
        "c0\taligned\tr2\t25\t1.0000\t5\t7\t2\t6\t5\t5\t0\t0\n"
        "c1\taligned\tr2\t11\t0.6000\t4\t7\t2\t6\t4\t3\t0\t1\n"
        "c2\tunaligned\t-\t0\t0.0000\t0\t0\t0\t0\t0\t0\t0\t0\n"
        "c3\taligned\tr0\t17\t0.8333\t6\t7\t1\t6\t5\t5\t1\t0\n")
    assert open(prefix + "_nearest_refs.txt").read() == ("#ref\tref_len\tcontigs\tmean_identity\n"
                                                         "r0\t7\t1\t0.8333\n"
                                                         "r1\t4\t0\t0.0000\n"
                                                         "r2\t7\t2\t0.8000\n")
    back = nr.read_nearest(prefix + "_nearest.txt")
    assert back["names"] == ["c0", "c1", "c2", "c3"] and back["ref_names"] == ["r2", "r2", None, "r0"]
    assert back["lens"].tolist() == [5, 4, 0, 6] and back["ref_lens"].tolist() == [7, 7, 0, 7] and back["identity"].tolist() == [1.0, 0.6, 0.0, 0.8333]
    first = nr.ref_index(ref_names)
    for f in nr.REC.names:
        want = result["recs"][f]
        got = back["recs"][f] if f != "ref" else np.array([-1 if x is None else first[x] for x in back["ref_names"]], dtype=np.int32)
        assert np.array_equal(got, want) and got.dtype == want.dtype, f
    refs = nr.read_refs_table(prefix + "_nearest_refs.txt")
    assert refs["names"] == ref_names and refs["ref_lens"].tolist() == [7, 4, 7] and refs["contigs"].tolist() == [1, 0, 2]
    assert refs["mean_identity"].tolist() == [0.8333, 0.0, 0.8]
    assert nr.parse_nearest(nr.NEAREST_HEADER)["names"] == [] and nr.parse_refs_table(nr.REFS_HEADER)["names"] == []
    H = nr.NEAREST_HEADER
    good = "c0\taligned\tr2\t25\t1.0000\t5\t7\t2\t6\t5\t5\t0\t0\n"
    assert nr.parse_nearest(H + good)["names"] == ["c0"]
    for bad in ("", good, H + good.replace("aligned", "gone"), H + good[:-3] + "\n", H + good.replace("\tr2\t", "\t-\t"),
                H + "c2\tunaligned\tr0\t0\t0.0000\t0\t0\t0\t0\t0\t0\t0\t0\n", H + "c2\tunaligned\t-\t3\t0.0000\t0\t0\t0\t0\t0\t0\t0\t0\n",
                H + good.replace("1.0000", "1.5000"), H + good.replace("\t25\t", "\tx\t"), H + good.replace("\t7\t", "\t-7\t")):
        with pytest.raises(ValueError):
            nr.parse_nearest(bad)
    for bad in ("", "r0\t7\t1\t0.5\n", nr.REFS_HEADER + "r0\t7\t1\n", nr.REFS_HEADER + "r0\t7\t0\t0.5000\n", nr.REFS_HEADER + "r0\t7\tx\t0.5000\n"):
        with pytest.raises(ValueError):
            nr.parse_refs_table(bad)


def test_identity_formatting_and_the_refs_summary():
    def rec(m, idn, ins, dele, ref=0):
        return np.array([(0, ref, 1, 1, 1, m, idn, ins, dele)], dtype=nr.REC)[0]

    assert nr.identity(rec(3, 2, 0, 0)) == 2 / 3 and nr.identity(rec(3, 3, 1, 2)) == 0.5
    assert nr.identity(np.array([(1, -1, 0, 0, 0, 0, 0, 0, 0)], dtype=nr.REC)[0]) == 0.0
    recs = np.array([(0, 1, 7, 1, 3, 3, 2, 0, 0), (0, 1, 7, 1, 3, 3, 3, 0, 0), (0, 1, 7, 1, 3, 8, 1, 0, 0), (1, -1, 0, 0, 0, 0, 0, 0, 0)], dtype=nr.REC)
    text = nr.nearest_text(["a", "b", "c", "d"], [3, 3, 8, 2], ["r0", "r1"], [5, 9], recs)
    assert [line.split("\t")[4] for line in text.splitlines()[1:]] == ["0.6667", "1.0000", "0.1250", "0.0000"]
    # the mean of the identities, summed in input order and divided once: (2/3 + 1 + 1/8) / 3
    assert nr.refs_text(["r0", "r1"], [5, 9], recs) == nr.REFS_HEADER + "r0\t5\t0\t0.0000\nr1\t9\t3\t%.4f\n" % ((2 / 3 + 1.0 + 0.125) / 3)


def test_reference_reading(tmp_path):
    text = ">r0 first one\nmk-V.l*\nAQ 1\n\n>r1\n---\n>\nACD\n>r3\tx\n  wy  \n"
    names, seqs = nr.parse_refs("junk before the first header\n" + text)
    assert names == ["r0", "r1", "", "r3"] and seqs == ["MKVLAQ", "", "ACD", "WY"]
    (tmp_path / "ref.faa").write_text(text, encoding="latin-1")
    assert nr.read_refs(str(tmp_path / "ref.faa")) == (names, seqs)
    assert nr.parse_refs(">r\nA\xe9\xc5B\n") == (["r"], ["AB"])                  # ASCII letters only
    assert [nr.residue_class(b) for b in (65, 97, 90, 122, 64, 91, 96, 123, 42, 45, 0, 193, 225)] == [1, 1, 26, 26, 0, 0, 0, 0, 0, 0, 0, 0, 0]


MATRIX = """# a hand-written matrix
   A  C  G  *
A  4 -1 -2 -7   # trailing comment
C -1  5 -3 -7
G -2 -3  6 -7

* -7 -7 -7  1
"""


def test_matrix_parser(tmp_path):
    sub = nr.parse_matrix(MATRIX)
    assert sub.dtype == np.int8 and sub.shape == (27, 27)
    A, Cc, G = 1, 3, 7
    assert [sub[A, A], sub[A, Cc], sub[A, G], sub[Cc, A], sub[Cc, Cc], sub[Cc, G], sub[G, A], sub[G, Cc], sub[G, G]] == [4, -1, -2, -1, 5, -3, -2, -3, 6]
    assert sub[0, 0] == 1 and sub[0, A] == -7 and sub[G, 0] == -7                  # the `*` row and column fill class 0
    rest = [c for c in range(1, 27) if c not in (A, Cc, G)]
    assert (sub[rest, :] == -7).all() and (sub[:, rest] == -7).all()                # absent letters: the file's lowest value
    # lower-case letters name the same classes; without `*` class 0 takes the lowest value too
    low = nr.parse_matrix("a c\na 2 -1\nc -1 3\n")
    assert low[1, 1] == 2 and low[3, 3] == 3 and low[1, 3] == -1 and low[0, 0] == -1 and low[26, 1] == -1
    for bad in ("", "# only a comment\n", MATRIX.replace(" 5 ", " 128 "), MATRIX.replace("-7   #", "-129 #"), MATRIX.replace("C -1  5 -3 -7", "C -1  5 -3"),
                MATRIX.replace("C -1  5 -3 -7", "C -1  5 -3 -7 0"), MATRIX.replace("G -2 -3  6 -7\n", ""), MATRIX.replace("G -2", "C -2"),
                MATRIX.replace("G -2", "T -2"), MATRIX.replace(" 6 ", " x "), "A AA\nA 1 1\nAA 1 1\n", "A a\nA 1 1\na 1 1\n", "A A\nA 1 1\n"):
        with pytest.raises(ValueError):
            nr.parse_matrix(bad)
    (tmp_path / "m.txt").write_text(MATRIX)
    assert np.array_equal(nr.parse_scoring(str(tmp_path / "m.txt")), sub)
    mm = nr.parse_scoring("5,-4")
    assert mm[0, 0] == -4 and all(mm[a, a] == 5 for a in range(1, 27)) and mm[1, 2] == -4 and mm[0, 5] == -4 and mm.dtype == np.int8
    assert np.array_equal(mm, nr.match_mismatch(5, -4))
    for bad in ("5", "5,-4,1", "200,1", "1,-129", "a,b", str(tmp_path / "nosuch.txt")):
        with pytest.raises((ValueError, OSError)):
            nr.parse_scoring(bad)


def test_new_symbols_are_declared():
    new = {"mgta_seqs_nearest", "mgta_ctx_set_nearest_batch"}
    assert new <= set(_lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    for struct, mirror in (("mgta_nearest_stats", _lib.NearestStats), ("mgta_nearest_rec", _lib.NearestRec)):
        fields = [n for n, _ in mirror._fields_]
        names = H.header_fields(struct, hdr)
        assert names == fields, struct                                    # the ctypes mirror has the header's order
    assert [n for n, _ in _lib.NearestRec._fields_] == list(api.NEAREST_REC.names) == list(nr.REC.names)
    assert ctypes.sizeof(_lib.NearestRec) == api.NEAREST_REC.itemsize == nr.REC.itemsize == 36
    for n in ("n_seqs", "n_refs", "n_pairs", "n_unaligned", "n_cells", "n_trace_cells", "n_batches", "ms_score", "ms_trace", "blocks_per_cu", "lds_bytes"):
        assert n in [f for f, _ in _lib.NearestStats._fields_]
    lib = _lib.load()                                                     # the library has them (dlopen needs no device)
    assert lib.mgta_seqs_nearest and lib.mgta_ctx_set_nearest_batch
    for m in ("nearest", "set_nearest_batch"):
        assert callable(getattr(api.Context, m))
    mk = open(os.path.join(ROOT, "megagta_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bnearest\.hip\b", mk, re.M)


def test_guards_need_no_device():
    """the argument checks come before any device work: a NULL context and a setter's bad value are refused as such"""
    lib = _lib.load()
    assert lib.mgta_seqs_nearest(None, None, None, 0, None, None, 0, None, 10, 1, None, None, None, None, None) == -1 and b"ctx" in lib.mgta_last_error()
    assert lib.mgta_ctx_set_nearest_batch(None, 7) == -1 and b"ctx" in lib.mgta_last_error()


def test_cli_prints_the_usage_line():
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    r = subprocess.run([BIN, "nearest"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage: megagta nearest <ref.faa> <prot.fasta> <out_prefix> <gap_open> <gap_extend> <scoring>" in r.stderr
    r = subprocess.run([BIN, "nearest", "a", "b", "c", "10", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage: megagta nearest" in r.stderr
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and re.search(r"^\s+nearest\s", r.stderr, re.M)
    r = subprocess.run([BIN, "nosuchstep"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and re.search(r"is not built here \([^)]*\bnearest\b", r.stderr)


def test_cli_refuses_bad_parameters_before_any_device_work(tmp_path):
    """gap parameters and scoring are checked before a context is made: the step fails, names what is wrong and writes nothing"""
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    (tmp_path / "ref.faa").write_text(">r0\nMKVLA\n")
    (tmp_path / "p.fa").write_text(">c0\nMKVLA\n")
    (tmp_path / "bad.txt").write_text(MATRIX.replace(" 5 ", " 128 "))
    (tmp_path / "ragged.txt").write_text(MATRIX.replace("C -1  5 -3 -7", "C -1  5 -3"))
    base = [BIN, "nearest", str(tmp_path / "ref.faa"), str(tmp_path / "p.fa"), str(tmp_path / "out")]
    for tail, word in ((["1", "2", "5,-4"], "gap_extend"), (["1025", "1", "5,-4"], "gap_open"), (["10", "-1", "5,-4"], "gap_extend"), (["x", "1", "5,-4"], "gap_open"),
                       (["10", "1", "500,-4"], "int8"), (["10", "1", "5"], "scoring"), (["10", "1", str(tmp_path / "bad.txt")], "int8"),
                       (["10", "1", str(tmp_path / "ragged.txt")], "bad row C"), (["10", "1", str(tmp_path / "nosuch.txt")], "scoring")):
        r = subprocess.run(base + tail, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "nearest" in r.stderr and word in r.stderr, (tail, r.stderr)
    assert sorted(os.listdir(tmp_path)) == ["bad.txt", "p.fa", "ragged.txt", "ref.faa"]


def _fresh_driver(tmp_path, monkeypatch, calls):
    from megagta_amd import megagta as drv
    drv = importlib.reload(drv)
    monkeypatch.setattr(drv, "run_step", lambda cmd, what, stdin_path=None, stdout_path=None: calls.append(cmd))
    drv.opt.out_dir = str(tmp_path) + "/"
    drv.opt.temp_dir = drv.opt.out_dir + "tmp/"
    os.makedirs(drv.opt.temp_dir, exist_ok=True)
    drv.opt.lib = drv.opt.temp_dir + "reads.lib"
    drv.opt.gene_info = {"rplB": ("f_rplB.hmm", "r_rplB.hmm", "rplB.faa"), "nirK": ("f_nirK.hmm", "r_nirK.hmm", "nirK.faa")}
    return drv


def test_driver_accepts_the_options(tmp_path, monkeypatch):
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    assert drv.opt.nearest is False and (drv.opt.nearest_scoring, drv.opt.nearest_gap_open, drv.opt.nearest_gap_extend) == ("5,-4", 10, 1)
    out = str(tmp_path / "new_out")
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--nearest"])
    assert drv.opt.nearest is True and drv.opt.cluster is False and (drv.opt.nearest_scoring, drv.opt.nearest_gap_open, drv.opt.nearest_gap_extend) == ("5,-4", 10, 1)
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--nearest", "--nearest-scoring", "m.txt", "--nearest-gap-open", "11", "--nearest-gap-extend", "2"])
    assert drv.opt.nearest is True and (drv.opt.nearest_scoring, drv.opt.nearest_gap_open, drv.opt.nearest_gap_extend) == ("m.txt", 11, 2)
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--align"])
    assert drv.opt.nearest is False
    for word in ("--nearest ", "--nearest-scoring", "--nearest-gap-open", "--nearest-gap-extend"):
        assert word in drv.USAGE
    # what a finished run wrote into opts.txt brings the options back
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    with open(drv.opt.out_dir + "opts.txt", "w") as fh:
        fh.write("\n".join(["-r", "reads.fa", "-g", "genes.txt", "--nearest", "--nearest-gap-open", "12"]) + "\n")
    drv.parse_opt(["--continue", "-o", str(tmp_path)])
    assert drv.opt.continue_mode and drv.opt.nearest is True and drv.opt.nearest_gap_open == 12 and drv.opt.nearest_gap_extend == 1


def test_gap_options_out_of_range_are_a_usage_error(tmp_path):
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "genes.txt"), "-o", str(tmp_path / "out"), "--nearest"]
    for extra in (["--nearest-gap-open", "1025"], ["--nearest-gap-extend", "11"], ["--nearest-gap-extend", "-1"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--nearest-gap-open" in r.stderr, extra
    assert not os.path.exists(tmp_path / "out")


OTHERS = ("coverage", "match_reads", "derep", "align", "cluster")
COMBOS = [o for o in itertools.product([False, True], repeat=5) if o[3] or not o[4]]       # --cluster needs --align


@pytest.mark.parametrize("others", COMBOS, ids=lambda o: "".join("cmdax"[i] if x else "-" for i, x in enumerate(o)))
def test_checkpoints_of_the_flag_come_last(tmp_path, monkeypatch, others):
    """the steps of --nearest run behind every step of a run without the flag, for every combination of the other flags; one checkpoint
    per gene; the input is the representatives with --cluster, what --derep kept with --derep; without the flag the checkpoint list is
    unchanged"""
    def set_flags(drv, nearest):
        drv.opt.coverage, drv.opt.match_reads, drv.opt.derep, drv.opt.align, drv.opt.cluster = others
        drv.opt.nearest = nearest

    calls = []
    drv = _fresh_driver(tmp_path, monkeypatch, calls)
    set_flags(drv, False)
    drv.search_contigs(44)
    drv.after_search(44)
    before = [c[1] for c in calls]
    extra = [s for s, on in zip(("coverage", "matchreads", "derep", "align", "cluster"), others) if on for _ in range(2)]
    assert before == ["search", "filterbylen", "translate", "filterbylen", "translate"] + extra
    cp_before = open(drv.opt.temp_dir + "cp.txt").read()
    assert cp_before == "".join(f"{i}\tdone\n" for i in range(len(before)))                         # without the flag: what it was
    os.remove(drv.opt.temp_dir + "cp.txt")
    calls.clear()
    drv = _fresh_driver(tmp_path, monkeypatch, calls)
    set_flags(drv, True)
    drv.opt.nearest_scoring, drv.opt.nearest_gap_open, drv.opt.nearest_gap_extend = "3,-2", 7, 2
    drv.search_contigs(44)
    drv.after_search(44)
    assert [c[1] for c in calls] == before + ["nearest"] * 2
    d = drv.opt.out_dir + "contigs/"
    stem = "/prot_merged" + ("_rmdup" if others[2] else "") + ("_rep_seqs" if others[4] else "")
    assert calls[-2:] == [[drv.opt.bin, "nearest", g + ".faa", d + g + stem + ".fasta", d + g + stem, "7", "2", "3,-2"] for g in ("rplB", "nirK")]
    if others[4]:
        assert calls[-3][1] == "cluster" and calls[-3][3] + "_rep_seqs.fasta" == calls[-1][3]      # it reads what --cluster wrote
    elif others[2]:
        derep = [c for c in calls if c[1] == "derep"][-1]
        assert derep[3] + "_rmdup.fasta" == calls[-1][3]                                            # ... or what --derep kept
    cp = open(drv.opt.temp_dir + "cp.txt").read()
    assert cp.startswith(cp_before) and cp == "".join(f"{i}\tdone\n" for i in range(len(before) + 2))
    # continuing a finished run: nothing runs, every checkpoint is passed.  A search step that is skipped counts one checkpoint (its
    # filters' are written inside it), so past it the flag's two steps are number after + 1 and after + 2
    after = len(before) - 5
    for last_cp, want in ((len(before) + 1, []), (after + 2, []), (after + 1, ["nearest"]), (after, ["nearest"] * 2)):
        calls.clear()
        drv = _fresh_driver(tmp_path, monkeypatch, calls)
        set_flags(drv, True)
        drv.opt.continue_mode, drv.opt.last_cp = True, last_cp
        drv.search_contigs(44)
        drv.after_search(44)
        assert [c[1] for c in calls] == want and drv.cp == 1 + after + 2
