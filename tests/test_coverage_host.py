"""Coverage: what needs no GPU -- the exported symbols, the two file writers and their parser, the binary's usage, the driver's flag."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
NEW = ("mgta_ctx_keep_multiplicity", "mgta_ctx_set_coverage_batch", "mgta_sdbg_load_large", "mgta_sdbg_edge_multiplicity", "mgta_contig_coverage")


def test_library_exports_the_coverage_calls():
    from megagta_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
        assert name + "(" in header, name
    # the two structs the calls fill have the layout the header declares
    assert ctypes.sizeof(_lib.ContigCov) == 32 and ctypes.sizeof(_lib.CoverageStats) == 64
    from megagta_amd import api
    assert api.COV_DTYPE.itemsize == 32
    assert [api.COV_DTYPE.fields[n][1] for n in ("sum", "len", "n_windows", "n_covered", "min", "max", "median")] == [0, 8, 12, 16, 20, 24, 28]


def test_writers_and_parser_round_trip(tmp_path):
    from megagta_amd import coverage as cv
    k = 30
    windows = [[3, 0, 7, 7, 1, 2], [5, 5, 0, 9], [], [65535]]            # even count -> LOWER median; a contig shorter than k + 1; one window
    lens = [len(w) + k if w else 12 for w in windows]
    rows = [cv.stats_of_windows(w, n) for w, n in zip(windows, lens)]
    assert [r["median"] for r in rows] == [2, 5, 0, 65535]                # sorted [0,1,2,3,7,7] -> element (6 - 1) // 2 = 2; [0,5,5,9] -> 5
    assert rows[2] == dict(len=12, windows=0, covered=0, sum=0, median=0, min=0, max=0)
    names = ["g_contig_0_contig_1", "g_contig_2_contig_3", "short", "one"]
    cv.write_coverage(str(tmp_path / "x_coverage.txt"), names, rows)
    text = (tmp_path / "x_coverage.txt").read_text().splitlines()
    assert text[0] == "#contig\tlen\twindows\tcovered\tmean\tmedian\tmin\tmax"
    assert text[1] == "g_contig_0_contig_1\t36\t6\t5\t3.3333\t2\t0\t7"      # 20 / 6 as %.4f
    assert text[2] == "g_contig_2_contig_3\t34\t4\t3\t4.7500\t5\t0\t9"
    assert text[3] == "short\t12\t0\t0\t0.0000\t0\t0\t0"
    assert text[4] == "one\t31\t1\t1\t65535.0000\t65535\t65535\t65535"
    back = cv.read_coverage(str(tmp_path / "x_coverage.txt"))
    assert [b["contig"] for b in back] == names
    for b, r in zip(back, rows):
        assert all(b[c] == r[c] for c in ("len", "windows", "covered", "median", "min", "max"))
        assert abs(b["mean"] - (r["sum"] / r["windows"] if r["windows"] else 0.0)) < 5e-5
    # the same rows from the structured array the API returns
    from megagta_amd import api
    arr = np.zeros(len(rows), dtype=api.COV_DTYPE)
    for a, r in zip(arr, rows):
        a["sum"], a["len"], a["n_windows"], a["n_covered"], a["min"], a["max"], a["median"] = r["sum"], r["len"], r["windows"], r["covered"], r["min"], r["max"], r["median"]
    assert cv.coverage_text(names, arr) == (tmp_path / "x_coverage.txt").read_text()
    ab = np.zeros(65536, dtype=np.int64)
    ab[[1, 2, 300, 65535]] = [10, 4, 1, 2]
    cv.write_abundance(str(tmp_path / "x_abundance.txt"), ab)
    assert (tmp_path / "x_abundance.txt").read_text() == "1\t10\n2\t4\n300\t1\n65535\t2\n"
    assert np.array_equal(cv.read_abundance(str(tmp_path / "x_abundance.txt")), ab)


def test_fasta_reader_names_and_multi_line_records(tmp_path):
    from megagta_amd import coverage as cv
    (tmp_path / "c.fa").write_text(">a some comment\nACGT\nacgt\r\n>b\n\n>c\tx\nNN")
    assert cv.read_fasta(str(tmp_path / "c.fa")) == (["a", "b", "c"], ["ACGTacgt", "", "NN"])


def test_binary_lists_coverage_and_driver_accepts_the_flag(tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    r = subprocess.run([BIN], capture_output=True, text=True)
    assert r.returncode == 1 and "coverage" in r.stderr
    r = subprocess.run([BIN, "coverage", "only_one_argument"], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage: megagta coverage <sdbg_prefix> <contigs.fasta> <out_prefix>" in r.stderr
    from megagta_amd import megagta as drv
    assert "coverage" in drv.LONG and "--coverage" in drv.USAGE
    # the flag parses (the run then stops at the first real check: the read file does not exist)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "megagta_amd", "megagta.py"), "--coverage", "-r", str(tmp_path / "none.fa"), "-g", "x", "-o",
                        str(tmp_path / "o")], capture_output=True, text=True)
    assert r.returncode == 2 and "Cannot find file" in r.stderr and "not recognized" not in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "megagta_amd", "megagta.py"), "--no-such-flag", "-r", "x"], capture_output=True, text=True)
    assert r.returncode == 2 and "not recognized" in r.stderr
