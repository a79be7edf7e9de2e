"""Host side of the alignment to the model, no device: the two files (writers and readers), the A2M line rebuilt from (cols, path,
sequence), the new symbols, the CLI's usage line, the driver's `--align` flag, where its checkpoints go and what the step is handed."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from megagta_amd import _lib
from megagta_amd import align as al
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
NEG_INF = float("-inf")


def sample():
    """four records on a model of 6 columns: a plain fragment, one with an insert and a delete, an unaligned one, one in upper case"""
    headers = ["c0 len=3", "c1", "c2 x y", "c3 "]
    seqs = ["kvl", "mkqvaa", "", "MKV"]
    recs = np.array([(-1.25, 0, 2, 4, 3, 0, 0), (3.00004, 0, 1, 6, 5, 1, 1), (NEG_INF, 1, 0, 0, 0, 0, 0), (7.5, 0, 4, 6, 3, 0, 0)], dtype=al.REC)
    cols = np.frombuffer(b"-KVL--" b"MK-VAA" b"------" b"---MKV", dtype=np.uint8).reshape(4, 6)
    paths = ["MMM", "MMIDMMM", "", "MMM"]
    return headers, seqs, dict(recs=recs, cols=cols, paths=paths)


def test_a2m_line_from_cols_path_and_sequence():
    headers, seqs, res = sample()
    lines = [al.a2m_line(res["cols"][i], res["paths"][i], seqs[i]) for i in range(4)]
    assert lines == ["-KVL--", "MKq-VAA", "------", "---MKV"]
    # the line without its inserted residues is the row of cols; its residues in order are the sequence
    for i, line in enumerate(lines):
        assert al.a2m_columns(line).encode() == res["cols"][i].tobytes()
        assert "".join(c for c in line if c != "-").lower() == seqs[i].lower()
    # model_from given or found: the same line; bytes in, the same out; an inserted upper-case residue comes out in lower case
    assert al.a2m_line(res["cols"][1], "MMIDMMM", b"mkqvaa", 1) == "MKq-VAA"
    assert al.a2m_line(np.frombuffer(b"MK-VAA", dtype=np.uint8), "MMIDMMM", "MKQVAA") == "MKq-VAA"
    assert al.a2m_line(np.frombuffer(b"-X*-", dtype=np.uint8), "MIM", "x**", 2) == "-X**-"
    for bad_path, seq in (("MMM", "kv"), ("MM", "kvl"), ("MXM", "kvl"), ("MMMMMMM", "kvlkvlk")):
        with pytest.raises((ValueError, IndexError)):
            al.a2m_line(res["cols"][0], bad_path, seq)


def test_files_round_trip(tmp_path):
    headers, seqs, res = sample()
    prefix = str(tmp_path / "prot_merged")
    al.write_align(prefix, headers, seqs, res)
    fasta = open(prefix + "_aligned.fasta").read()
    assert fasta == ">c0 len=3\n-KVL--\n>c1\nMKq-VAA\n>c2 x y\n------\n>c3 \n---MKV\n"            # header lines as they stood
    assert al.read_aligned_fasta(prefix + "_aligned.fasta") == [("c0 len=3", "-KVL--"), ("c1", "MKq-VAA"), ("c2 x y", "------"), ("c3 ", "---MKV")]
    table = open(prefix + "_aligned.txt").read()
    assert table == ("#contig\tlen\tstatus\tscore\tmodel_from\tmodel_to\tmatch\tinsert\tdelete\n"
                     "c0\t3\taligned\t-1.2500\t2\t4\t3\t0\t0\n"
                     "c1\t6\taligned\t3.0000\t1\t6\t5\t1\t1\n"
                     "c2\t0\tunaligned\t-inf\t0\t0\t0\t0\t0\n"
                     "c3\t3\taligned\t7.5000\t4\t6\t3\t0\t0\n")
    back = al.read_table(prefix + "_aligned.txt")
    assert back["names"] == ["c0", "c1", "c2", "c3"] and back["lens"].tolist() == [3, 6, 0, 3]
    assert back["recs"].dtype == al.REC
    for f in ("status", "model_from", "model_to", "n_match", "n_insert", "n_delete"):
        assert np.array_equal(back["recs"][f], res["recs"][f]), f
    assert np.allclose(back["recs"]["score"][[0, 1, 3]], res["recs"]["score"][[0, 1, 3]], rtol=0, atol=5e-5) and back["recs"]["score"][2] == NEG_INF
    assert al.parse_table(al.TABLE_HEADER)["names"] == []
    for bad in ("", "c0\t3\taligned\t1.0\t1\t1\t1\t0\t0\n", al.TABLE_HEADER + "c0\t3\tgone\t1.0\t1\t1\t1\t0\t0\n", al.TABLE_HEADER + "c0\t3\taligned\t1.0\t1\t1\t1\t0\n",
                al.TABLE_HEADER + "c0\t3\taligned\t-inf\t1\t1\t1\t0\t0\n", al.TABLE_HEADER + "c0\t3\tunaligned\t1.0\t0\t0\t0\t0\t0\n",
                al.TABLE_HEADER + "c0\tx\taligned\t1.0\t1\t1\t1\t0\t0\n"):
        with pytest.raises(ValueError):
            al.parse_table(bad)
    with pytest.raises(ValueError):
        al.parse_aligned_fasta(">c0\nKVL\n>c1\n")


def test_new_symbols_are_declared():
    assert {"mgta_seqs_align", "mgta_ctx_set_align_batch"} <= set(_lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    assert re.search(r"\bmgta_seqs_align\s*\(", hdr) and re.search(r"\bmgta_ctx_set_align_batch\s*\(", hdr)
    for struct, mirror in (("mgta_align_stats", _lib.AlignStats), ("mgta_align_rec", _lib.AlignRec)):
        fields = [n for n, _ in mirror._fields_]
        names = H.header_fields(struct, hdr)
        assert names == fields, struct                                    # the ctypes mirror has the header's order
    assert [n for n, _ in _lib.AlignRec._fields_] == list(al.REC.names)
    import ctypes
    assert ctypes.sizeof(_lib.AlignRec) == al.REC.itemsize == 32
    for n in ("n_seqs", "n_aligned", "n_unaligned", "n_cells", "n_batches", "ms_fill", "ms_trace"):
        assert n in [f for f, _ in _lib.AlignStats._fields_]
    lib = _lib.load()                                                     # the library has them (dlopen needs no device)
    assert lib.mgta_seqs_align and lib.mgta_ctx_set_align_batch


def test_cli_prints_the_usage_line():
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    r = subprocess.run([BIN, "align"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage: megagta align <model.hmm> <prot.fasta> <out_prefix>" in r.stderr
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and re.search(r"^\s+align\s", r.stderr, re.M)
    r = subprocess.run([BIN, "nosuchstep"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and re.search(r"is not built here \([^)]*\balign\b", r.stderr)


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


def test_driver_accepts_the_flag(tmp_path, monkeypatch):
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    assert drv.opt.align is False
    out = str(tmp_path / "new_out")
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--align"])
    assert drv.opt.align is True and drv.opt.derep is False and drv.opt.coverage is False and drv.opt.match_reads is False
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--derep"])
    assert drv.opt.align is False and drv.opt.derep is True
    assert "--align" in drv.USAGE


@pytest.mark.parametrize("others", [False, True])
def test_checkpoints_of_the_flag_come_last(tmp_path, monkeypatch, others):
    """the steps of --align run behind every step of a run without the flag and behind those of --coverage, --match-reads and --derep;
    one checkpoint per gene; with --derep the input is what it kept"""
    calls = []
    drv = _fresh_driver(tmp_path, monkeypatch, calls)
    drv.search_contigs(44)
    drv.after_search(44)                                                  # without the flags: nothing more
    plain = [c[1] for c in calls]
    assert plain == ["search", "filterbylen", "translate", "filterbylen", "translate"]
    cp_plain = open(drv.opt.temp_dir + "cp.txt").read()
    assert cp_plain == "".join(f"{i}\tdone\n" for i in range(5))
    os.remove(drv.opt.temp_dir + "cp.txt")
    calls.clear()
    drv = _fresh_driver(tmp_path, monkeypatch, calls)
    drv.opt.align, drv.opt.coverage, drv.opt.match_reads, drv.opt.derep = True, others, others, others
    drv.search_contigs(44)
    drv.after_search(44)
    extra = (["coverage"] * 2 + ["matchreads"] * 2 + ["derep"] * 2 if others else []) + ["align"] * 2
    assert [c[1] for c in calls] == plain + extra
    d = drv.opt.out_dir + "contigs/"
    stem = "/prot_merged_rmdup" if others else "/prot_merged"
    assert calls[-2:] == [[drv.opt.bin, "align", f"f_{g}.hmm", d + g + stem + ".fasta", d + g + stem] for g in ("rplB", "nirK")]
    cp = open(drv.opt.temp_dir + "cp.txt").read()
    assert cp.startswith(cp_plain) and cp == "".join(f"{i}\tdone\n" for i in range(5 + len(extra)))
    # continuing a finished run: nothing runs, every checkpoint is passed
    calls.clear()
    drv = _fresh_driver(tmp_path, monkeypatch, calls)
    drv.opt.align, drv.opt.coverage, drv.opt.match_reads, drv.opt.derep = True, others, others, others
    drv.opt.continue_mode, drv.opt.last_cp = True, 4 + len(extra)
    drv.search_contigs(44)
    drv.after_search(44)
    assert calls == [] and drv.cp == 1 + len(extra)
