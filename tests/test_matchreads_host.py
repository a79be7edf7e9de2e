"""Host side of read recruitment, no device: the matched-reads file (writer and reader), the driver's `--match-reads` flag and where
its checkpoints go."""
import importlib
import os

import numpy as np
import pytest

from megagta_amd import matchreads as mr
from megagta_amd import readlib

DNA = "ACGT"


def ragged_library(seed=9):
    rng = np.random.default_rng(seed)
    lens = [1, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100, 150] + [int(x) for x in rng.integers(1, 200, 40)]
    return [rng.integers(0, 4, n).astype(np.uint8) for n in lens]


def test_text_round_trip_on_a_ragged_library():
    reads = ragged_library()
    strs = ["".join(DNA[c] for c in r) for r in reads]
    packed, start = readlib.pack_for_build(reads)                         # every read stored reversed, as it is uploaded
    pick = [50, 0, 3, 4, 12, 7]                                           # any order in, ascending out
    text = mr.match_reads_text(pick, packed, start)
    assert text == "".join(f">r{i}\n{strs[i]}\n" for i in sorted(pick))
    idx, seqs = mr.parse_match_reads(text)
    assert idx.dtype == np.int64 and idx.tolist() == sorted(pick) and seqs == [strs[i] for i in sorted(pick)]
    mask = np.zeros(len(reads), dtype=bool)
    mask[pick] = True
    assert mr.match_reads_text(mask, packed, start) == text              # a bool mask over the reads selects the same records
    everything = mr.match_reads_text(np.arange(len(reads)), packed, start)
    assert mr.parse_match_reads(everything)[1] == strs
    # forward storage: the same text from the words as the .bin file holds them
    fwd = readlib.pack_codes(np.concatenate(reads))
    assert mr.match_reads_text(pick, fwd, start, reversed_storage=False) == text


def test_empty_selection_is_an_empty_file(tmp_path):
    reads = ragged_library()
    packed, start = readlib.pack_for_build(reads)
    assert mr.match_reads_text([], packed, start) == "" and mr.match_reads_text(np.zeros(len(reads), dtype=bool), packed, start) == ""
    path = str(tmp_path / "x_match_reads.fa")
    mr.write_match_reads(path, [], packed, start)
    assert os.path.getsize(path) == 0
    idx, seqs = mr.read_match_reads(path)
    assert idx.size == 0 and seqs == []
    mr.write_match_reads(path, [2, 1], packed, start)
    assert mr.read_match_reads(path)[0].tolist() == [1, 2]
    with pytest.raises(ValueError):
        mr.parse_match_reads(">x1\nACGT\n")
    with pytest.raises(ValueError):
        mr.parse_match_reads(">r1\n")


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
    assert drv.opt.match_reads is False
    out = str(tmp_path / "new_out")
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--match-reads"])
    assert drv.opt.match_reads is True and drv.opt.coverage is False
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--coverage", "--match-reads"])
    assert drv.opt.match_reads is True and drv.opt.coverage is True
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out])
    assert drv.opt.match_reads is False
    assert "--match-reads" in drv.USAGE


@pytest.mark.parametrize("coverage", [False, True])
def test_checkpoints_of_the_flag_come_last(tmp_path, monkeypatch, coverage):
    """the steps of --match-reads run behind every step of a run without the flag, and behind --coverage's; one checkpoint per gene"""
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
    drv.opt.match_reads, drv.opt.coverage = True, coverage
    drv.search_contigs(44)
    drv.after_search(44)
    extra = (["coverage"] * 2 if coverage else []) + ["matchreads"] * 2
    assert calls == plain + extra
    cp = open(drv.opt.temp_dir + "cp.txt").read()
    assert cp.startswith(cp_plain) and cp == "".join(f"{i}\tdone\n" for i in range(5 + len(extra)))
    # continuing a finished run: nothing runs, every checkpoint is passed
    calls.clear()
    drv = _fresh_driver(tmp_path, monkeypatch, calls)
    drv.opt.match_reads, drv.opt.coverage = True, coverage
    drv.opt.continue_mode, drv.opt.last_cp = True, 4 + len(extra)
    drv.search_contigs(44)
    drv.after_search(44)
    assert calls == [] and drv.cp == 1 + len(extra)


def test_the_step_is_given_the_graph_the_library_and_the_gene_contigs(tmp_path, monkeypatch):
    from megagta_amd import megagta as drv
    drv = importlib.reload(drv)
    cmds = []
    monkeypatch.setattr(drv, "run_step", lambda cmd, what, stdin_path=None, stdout_path=None: cmds.append(cmd))
    drv.opt.out_dir = str(tmp_path) + "/"
    drv.opt.temp_dir = drv.opt.out_dir + "tmp/"
    os.makedirs(drv.opt.temp_dir)
    drv.opt.lib = drv.opt.temp_dir + "reads.lib"
    drv.opt.gene_info = {"rplB": ("f", "r", "a")}
    drv.opt.match_reads = True
    drv.after_search(44)
    d = drv.opt.out_dir + "contigs/rplB"
    assert cmds == [[drv.opt.bin, "matchreads", drv.graph_prefix(44), drv.opt.lib, d + "/nucl_merged.fasta", d + "/nucl_merged"]]
