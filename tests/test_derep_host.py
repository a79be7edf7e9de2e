"""Host side of de-replication, no device: the map file and the kept-records FASTA (writers and reader), the new symbols, the driver's
`--derep` flag, where its checkpoints go and what the step is handed."""
import importlib
import os
import re

import numpy as np
import pytest

from megagta_amd import _lib
from megagta_amd import derep as dr
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sample():
    headers = ["c0 len=5", "c1", "c2 x y", "c3", "c4 ", "c5"]
    seqs = ["mkvla", "kvl", "mkvla", "", "qqq", "kvl"]
    res = dict(status=np.array([0, 2, 1, 2, 0, 1], dtype=np.uint8), rep=np.array([0, -1, 0, -1, 4, 1], dtype=np.int64),
               copies=np.array([2, 2, 0, 1, 1, 0], dtype=np.uint32))
    return headers, seqs, res


def test_map_text_round_trip():
    headers, seqs, res = sample()
    names = [dr.record_name(h) for h in headers]
    assert names == ["c0", "c1", "c2", "c3", "c4", "c5"]
    text = dr.map_text(names, res["status"], res["rep"], res["copies"])
    assert text == "c0\tkept\tc0\t2\nc1\tcontained\t-\t2\nc2\tduplicate\tc0\t0\nc3\tcontained\t-\t1\nc4\tkept\tc4\t1\nc5\tduplicate\tc1\t0\n"
    back = dr.parse_map(text)
    assert back["names"] == names
    for f, t in (("status", np.uint8), ("rep", np.int64), ("copies", np.uint32)):
        assert back[f].dtype == t and np.array_equal(back[f], res[f]), f
    assert dr.parse_map("")["names"] == [] and dr.parse_map("")["status"].size == 0
    for bad in ("c0\tkept\tc0\n", "c0\tgone\tc0\t1\n", "c0\tkept\t-\t1\n", "c0\tcontained\tc0\t1\n", "c0\tduplicate\tzz\t0\n", "c0\tkept\tc0\t-1\n"):
        with pytest.raises(ValueError):
            dr.parse_map(bad)


def test_files_round_trip(tmp_path):
    headers, seqs, res = sample()
    prefix = str(tmp_path / "prot_merged")
    dr.write_derep(prefix, headers, seqs, res)
    assert open(prefix + "_rmdup.fasta").read() == ">c0 len=5\nmkvla\n>c4 \nqqq\n"        # header lines as they stood
    back = dr.read_map(prefix + "_rmdup_map.txt")
    assert np.array_equal(back["status"], res["status"]) and np.array_equal(back["rep"], res["rep"]) and np.array_equal(back["copies"], res["copies"])
    assert dr.rmdup_fasta_text(headers, seqs, np.ones(6, dtype=np.uint8)) == ""


def test_new_symbols_are_declared():
    assert {"mgta_seqs_derep", "mgta_ctx_set_derep_hash_bits"} <= set(_lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    assert re.search(r"\bmgta_seqs_derep\s*\(", hdr) and re.search(r"\bmgta_ctx_set_derep_hash_bits\s*\(", hdr)
    fields = [n for n, _ in _lib.DerepStats._fields_]
    assert fields == ["n_seqs", "n_letters", "n_first", "n_duplicates", "n_contained", "n_kept", "n_windows", "anchor_len", "n_compares",
                      "ms_dups", "ms_table", "ms_verify"]
    assert H.header_fields("mgta_derep_stats", hdr) == fields                        # the ctypes mirror has the header's order


def _fresh_driver(tmp_path, monkeypatch, calls):
    from megagta_amd import megagta as drv
    drv = importlib.reload(drv)
    monkeypatch.setattr(drv, "run_step", lambda cmd, what, stdin_path=None, stdout_path=None: calls.append(cmd[1]))
    drv.opt.out_dir = str(tmp_path) + "/"
    drv.opt.temp_dir = drv.opt.out_dir + "tmp/"
    os.makedirs(drv.opt.temp_dir, exist_ok=True)
    drv.opt.lib = drv.opt.temp_dir + "reads.lib"
    drv.opt.gene_info = {"rplB": ("f", "r", "a"), "nirK": ("f", "r", "a")}
    return drv


def test_driver_accepts_the_flag(tmp_path, monkeypatch):
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    assert drv.opt.derep is False
    out = str(tmp_path / "new_out")
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--derep"])
    assert drv.opt.derep is True and drv.opt.coverage is False and drv.opt.match_reads is False
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--coverage", "--derep", "--match-reads"])
    assert drv.opt.derep is True and drv.opt.coverage is True and drv.opt.match_reads is True
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out])
    assert drv.opt.derep is False
    assert "--derep" in drv.USAGE


@pytest.mark.parametrize("others", [False, True])
def test_checkpoints_of_the_flag_come_last(tmp_path, monkeypatch, others):
    """the steps of --derep run behind every step of a run without the flag, and behind those of --coverage and --match-reads; one
    checkpoint per gene"""
    calls = []
    drv = _fresh_driver(tmp_path, monkeypatch, calls)
    drv.search_contigs(44)
    drv.after_search(44)                                                  # without the flags: nothing more
    plain = list(calls)
    assert plain == ["search", "filterbylen", "translate", "filterbylen", "translate"]
    cp_plain = open(drv.opt.temp_dir + "cp.txt").read()
    assert cp_plain == "".join(f"{i}\tdone\n" for i in range(5))
    os.remove(drv.opt.temp_dir + "cp.txt")
    calls.clear()
    drv = _fresh_driver(tmp_path, monkeypatch, calls)
    drv.opt.derep, drv.opt.coverage, drv.opt.match_reads = True, others, others
    drv.search_contigs(44)
    drv.after_search(44)
    extra = (["coverage"] * 2 + ["matchreads"] * 2 if others else []) + ["derep"] * 2
    assert calls == plain + extra
    cp = open(drv.opt.temp_dir + "cp.txt").read()
    assert cp.startswith(cp_plain) and cp == "".join(f"{i}\tdone\n" for i in range(5 + len(extra)))
    # continuing a finished run: nothing runs, every checkpoint is passed
    calls.clear()
    drv = _fresh_driver(tmp_path, monkeypatch, calls)
    drv.opt.derep, drv.opt.coverage, drv.opt.match_reads = True, others, others
    drv.opt.continue_mode, drv.opt.last_cp = True, 4 + len(extra)
    drv.search_contigs(44)
    drv.after_search(44)
    assert calls == [] and drv.cp == 1 + len(extra)


def test_the_step_is_given_the_protein_and_the_nucleotide_contigs(tmp_path, monkeypatch):
    from megagta_amd import megagta as drv
    drv = importlib.reload(drv)
    cmds = []
    monkeypatch.setattr(drv, "run_step", lambda cmd, what, stdin_path=None, stdout_path=None: cmds.append(cmd))
    drv.opt.out_dir = str(tmp_path) + "/"
    drv.opt.temp_dir = drv.opt.out_dir + "tmp/"
    os.makedirs(drv.opt.temp_dir)
    drv.opt.lib = drv.opt.temp_dir + "reads.lib"
    drv.opt.gene_info = {"rplB": ("f", "r", "a")}
    drv.opt.derep = True
    drv.after_search(44)
    d = drv.opt.out_dir + "contigs/rplB"
    assert cmds == [[drv.opt.bin, "derep", d + "/prot_merged.fasta", d + "/prot_merged", d + "/nucl_merged.fasta", d + "/nucl_merged"]]
