"""megagta_amd/samplecov.py and the library table readers without a device: the readers of `.lib_info`, the writers and readers of the
three files, the integer formatting of masses above 2^53, the join with every branch, and the driver's usage error.  Expected numbers
are worked out here by hand or with fractions.Fraction, never taken from the module."""
import ctypes
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from megagta_amd import _lib, readlib
from megagta_amd import cluster as clustlib
from megagta_amd import samplecov as sc
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")


# ---- the library table ----------------------------------------------------------------------------------------------------------------
def test_read_lib_table_on_the_toy_library(golden_dir):
    prefix = os.path.join(golden_dir, "toy", "reads.lib")
    assert readlib.read_lib_table(prefix) == [("reads.fa", 0, 5999, 150, False)]
    assert readlib.read_lib_info(prefix) == (900000, 6000)               # (the reader of the first line is what it was)


THREE = "1234 10\nsample A: a.fa\n0 3 100 se\nsample B\tpair\n4 9 151 pe\nnothing here\n10 9 0 se\n"


def test_read_lib_table_se_pe_and_an_empty_library(tmp_path):
    p = str(tmp_path / "x.lib")
    open(p + ".lib_info", "w").write(THREE)
    assert readlib.read_lib_table(p) == [("sample A: a.fa", 0, 3, 100, False), ("sample B\tpair", 4, 9, 151, True), ("nothing here", 10, 9, 0, False)]
    open(p + ".lib_info", "w").write("0 0\nempty\n0 -1 0 se\n")           # an empty library first: to = from - 1 = -1
    assert readlib.read_lib_table(p) == [("empty", 0, -1, 0, False)]


@pytest.mark.parametrize("what,text", [
    ("overlap", "1234 10\na\n0 5 100 se\nb\n5 9 100 se\n"), ("gap", "1234 10\na\n0 3 100 se\nb\n5 9 100 se\n"), ("short", "1234 10\na\n0 8 100 se\n"),
    ("long", "1234 10\na\n0 10 100 se\n"), ("start", "1234 10\na\n1 9 100 se\n"), ("backwards", "1234 10\na\n0 9 100 se\nb\n10 7 100 se\n"),
    ("kind", "1234 10\na\n0 9 100 xx\n"), ("half", "1234 10\na\n"), ("first", "x\n")])
def test_read_lib_table_refuses_ranges_that_do_not_tile(tmp_path, what, text):
    p = str(tmp_path / "x.lib")
    open(p + ".lib_info", "w").write(text)
    with pytest.raises(ValueError):
        readlib.read_lib_table(p)


def test_formats_cpp_reads_the_same_table(tmp_path):
    """`megagta samplecov` dies on a table that does not tile, before it touches a device (the reader of formats.cpp)"""
    if not os.path.exists(BIN):
        import __graft_entry__
        __graft_entry__.build()
    (tmp_path / "c.fa").write_text(">c\nACGT\n")
    p = str(tmp_path / "x.lib")
    open(p + ".lib_info", "w").write("1234 10\na\n0 3 100 se\nb\n5 9 100 se\n")
    r = subprocess.run([BIN, "samplecov", str(tmp_path / "g"), p, str(tmp_path / "c.fa"), str(tmp_path / "o")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "library 2 holds the reads 5 .. 9, the libraries before it end at 4" in r.stderr
    assert not (tmp_path / "o_samplecov.txt").exists()
    src = open(os.path.join(ROOT, "megagta_amd", "csrc", "host", "formats.cpp")).read()
    assert "read_lib_table(const std::string &prefix)" in src


# ---- hand-written tables --------------------------------------------------------------------------------------------------------------
# eight nucleotide records; clusters 0 = {a0 (rep), a1, a2}, 3 = {b0 (rep), b1}, 5 = {c0}, 6 = {d0}; u0 is unaligned.  Three libraries,
# the second of them empty.
NAMES = ["a0", "a1", "a2", "b0", "u0", "c0", "d0", "b1"]
BIG = (1 << 60) + 1                                                       # a Q16 mass above 2^53: no double holds it
MASS_Q16 = [[10 * 65536, 0, 65536 // 3], [65536 // 3, 0, 7], [7, 0, 0], [5 * 65536 + 1, 0, BIG], [2 * 65536, 0, 65536], [65536 // 7, 0, 1], [3 * 65536, 0, 6], [0, 0, 0]]
CLUST = clustlib.CLUST_HEADER + "".join(line + "\n" for line in (
    "a0\trep\t0\ta0\t90\t0\t90", "a1\tmember\t0\ta0\t80\t0\t80", "a2\tmember\t0\ta0\t70\t1\t70", "b0\trep\t3\tb0\t90\t0\t90", "u0\tunaligned\t-\t-\t0\t0\t0",
    "c0\trep\t5\tc0\t60\t0\t60", "d0\trep\t6\td0\t60\t0\t60", "b1\tmember\t3\tb0\t50\t0\t50"))
LIBS = [dict(reads=4, read_windows=320, hit_windows=17, text="sample A: a.fa"), dict(reads=0, read_windows=0, hit_windows=0, text="nothing here"),
        dict(reads=6, read_windows=1 << 40, hit_windows=1 << 39, text="sample C 1.fq 2.fq")]


def e4(mass):
    return int(Fraction(mass, 65536) * 10000)                             # floor: the value is not negative


def cov_text(masses=MASS_Q16, names=NAMES):
    recs = [dict(len=100 + i, n_windows=60 + i, n_covered=(50 if any(m) else 0), n_unique=(5 if any(m) else 0), max_share=(9 if any(m) else 0)) for i, m in enumerate(masses)]
    return sc.samplecov_text(LIBS, names, recs, masses)


def test_samplecov_text_and_its_reader(tmp_path):
    text = cov_text()
    lines = text.splitlines()
    assert lines[0] == "#lib\t1\t4\t320\t17\tsample A: a.fa" and lines[1] == "#lib\t2\t0\t0\t0\tnothing here"
    assert lines[2] == "#lib\t3\t6\t%d\t%d\tsample C 1.fq 2.fq" % (1 << 40, 1 << 39)
    assert lines[3] == "#contig\tlen\twindows\tcovered\tunique\tmax_share\tmass_1\tmass_2\tmass_3"
    assert lines[4] == "a0\t100\t60\t50\t5\t9\t10.0000\t0.0000\t0.3333" and lines[5] == "a1\t101\t61\t50\t5\t9\t0.3333\t0.0000\t0.0001"
    assert lines[7] == "b0\t103\t63\t50\t5\t9\t5.0000\t0.0000\t17592186044416.0000" and lines[11] == "b1\t107\t67\t0\t0\t0\t0.0000\t0.0000\t0.0000"
    assert len(lines) == 3 + 1 + 8
    cov = sc.parse_samplecov(text)
    assert cov["libs"] == LIBS and [r["contig"] for r in cov["rows"]] == NAMES
    assert [r["mass"] for r in cov["rows"]] == [[e4(x) for x in m] for m in MASS_Q16]
    assert cov["rows"][3]["mass"][2] == (1 << 44) * 10000 and BIG > 1 << 53 and float(BIG) != BIG
    # a structured array and a uint64 matrix, as the API returns them, print the same bytes
    dt = [(n, "<u8" if n == "mass" else "<u4") for n in ("mass", "len", "n_windows", "n_covered", "n_unique", "max_share", "reserved_")]
    arr = np.array([(sum(m), 100 + i, 60 + i, 50 if any(m) else 0, 5 if any(m) else 0, 9 if any(m) else 0, 0) for i, m in enumerate(MASS_Q16)], dtype=dt)
    assert sc.samplecov_text(LIBS, NAMES, arr, np.array(MASS_Q16, dtype=np.uint64)) == text
    (tmp_path / "x_samplecov.txt").write_text(text)
    assert sc.read_samplecov(str(tmp_path / "x_samplecov.txt")) == cov
    for bad in (text.replace("#lib\t2", "#lib\t4"), text.replace("10.0000", "10.000"), text.replace("\tmass_3\n", "\n"), "\n".join(lines[3:]) + "\n",
                text.replace("b1\t107\t67\t0\t0\t0\t0.0000", "b1\t107\t67\t0\t0\t0\t0.0001"), text.replace("a0\t100\t60\t50", "a0\t100\t60\t61")):
        with pytest.raises(ValueError):
            sc.parse_samplecov(bad)
    with pytest.raises(ValueError):
        sc.samplecov_text(LIBS, NAMES[:1], arr[:1], [[1, 2]])              # two masses, three libraries
    tabbed = [dict(LIBS[0], text="sample B\tpair")]                        # the text is the last field: a tab in it comes back
    assert sc.parse_samplecov(sc.samplecov_text(tabbed, [], [], []))["libs"] == tabbed


@pytest.mark.parametrize("mass", [0, 1, 6, 7, 65535, 65536, 300 * 65536 // 7, (1 << 53) + 1, (1 << 63) + 12345, (1 << 64) - 1])
def test_masses_print_by_the_integer_rule(mass):
    text = sc.samplecov_text(LIBS[:1], ["c"], [dict(len=9, n_windows=3, n_covered=1, n_unique=1, max_share=1)], [[mass]])
    got = text.splitlines()[-1].split("\t")[-1]
    exact = Fraction(mass, 65536)
    q = int(exact * 10000)
    assert got == "%d.%04d" % (q // 10000, q % 10000) and re.fullmatch(r"\d+\.\d{4}", got)
    assert Fraction(q, 10000) <= exact < Fraction(q + 1, 10000)
    assert sc.parse_samplecov(text)["rows"][0]["mass"] == [q]
    assert {(1 << 64) - 1: "281474976710655.9999", (1 << 53) + 1: "137438953472.0000", 7: "0.0001"}.get(mass, got) == got


def test_lib_read_windows_and_libs_of():
    start = np.cumsum([0, 100, 20, 21, 0, 150, 19, 30], dtype=np.uint64)
    assert sc.lib_read_windows(start, [1, 1, 5, 7], 20) == [80, 0, 0 + 1 + 0 + 130, 0 + 10]
    assert sc.lib_read_windows(start, [7], 20) == [221] and sc.lib_read_windows(start, [3], 150) == [0]
    table = [("sample A: a.fa", 0, 3, 100, False), ("nothing here", 4, 3, 0, False), ("sample C 1.fq 2.fq", 4, 9, 151, True)]
    assert sc.libs_of(table, [320, 0, 1 << 40], np.array([17, 0, 1 << 39], dtype=np.uint64)) == LIBS


# ---- the join -------------------------------------------------------------------------------------------------------------------------
def test_join_adds_up_exactly_and_the_ppm_are_floors(tmp_path):
    cov = sc.parse_samplecov(cov_text())
    table = sc.join(cov, clustlib.parse_clust(CLUST))
    m = [[e4(x) for x in row] for row in MASS_Q16]
    add = lambda rows: [sum(m[i][s] for i in rows) for s in range(3)]
    assert table["rows"] == [dict(cluster=0, rep="a0", contigs=3, mass=add([0, 1, 2])), dict(cluster=3, rep="b0", contigs=2, mass=add([3, 7])),
                             dict(cluster=5, rep="c0", contigs=1, mass=m[5]), dict(cluster=6, rep="d0", contigs=1, mass=m[6]),
                             dict(cluster=None, rep=None, contigs=1, mass=m[4])]
    assert table["records"] == 8 and table["total"] == add(range(8)) and table["libs"] == LIBS
    text = sc.otu_samples_text(table)
    lines = text.splitlines()
    assert lines[:3] == cov_text().splitlines()[:3] and lines[3] == "#cluster\trep\tcontigs\tmass_1\tmass_2\tmass_3"
    assert lines[4] == "0\ta0\t3\t10.3334\t0.0000\t0.3334" and lines[8] == "-\t-\t1\t2.0000\t0.0000\t1.0000"
    assert lines[9] == "#total\t-\t8\t20.4762\t0.0000\t17592186044417.3334" and len(lines) == 10
    # every column sums to its total exactly, in ten-thousandths, above 2^53 too
    back = sc.parse_otu_samples(text)
    assert back == table
    for s in range(3):
        assert sum(r["mass"][s] for r in back["rows"]) == back["total"][s]
    assert back["total"][2] == (1 << 44) * 10000 + 13334 > 1 << 53
    # the ppm are floors of exact fractions, sum to at most 10^6, and 0 where the total is 0
    ptext = sc.otu_samples_ppm_text(table)
    ppm = sc.parse_otu_samples_ppm(ptext)
    for r, p in zip(table["rows"], ppm["rows"]):
        assert (p["cluster"], p["rep"], p["contigs"]) == (r["cluster"], r["rep"], r["contigs"])
        for s in range(3):
            want = int(Fraction(r["mass"][s] * 1000000, table["total"][s])) if table["total"][s] else 0
            assert p["mass"][s] == want
    assert ppm["total"] == [1000000, 0, 1000000] and all(sum(p["mass"][s] for p in ppm["rows"]) <= 1000000 for s in range(3))
    assert ptext.splitlines()[4] == "0\ta0\t3\t%d\t0\t0" % (103334 * 1000000 // 204762) and ptext.splitlines()[8].startswith("-\t-\t1\t")
    # without unaligned records there is no such line
    clean = CLUST.replace("u0\tunaligned\t-\t-\t0\t0\t0", "u0\trep\t4\tu0\t10\t0\t10")
    t2 = sc.join(cov, clustlib.parse_clust(clean))
    assert [r["cluster"] for r in t2["rows"]] == [0, 3, 4, 5, 6] and "\n-\t-\t" not in sc.otu_samples_text(t2) and sc.parse_otu_samples(sc.otu_samples_text(t2)) == t2
    # a table that does not add up is refused by the reader
    with pytest.raises(ValueError):
        sc.parse_otu_samples(text.replace("0\ta0\t3\t10.3334", "0\ta0\t3\t10.3335"))
    with pytest.raises(ValueError):
        sc.parse_otu_samples(text.replace("#total\t-\t8", "#total\t-\t9"))
    # the files
    (tmp_path / "n_samplecov.txt").write_text(cov_text())
    (tmp_path / "p_clust.txt").write_text(CLUST)
    assert sc.write_otu_samples(str(tmp_path / "p"), str(tmp_path / "n_samplecov.txt"), str(tmp_path / "p_clust.txt")) == table
    assert (tmp_path / "p_otu_samples.txt").read_text() == text and (tmp_path / "p_otu_samples_ppm.txt").read_text() == ptext
    assert sc.read_otu_samples(str(tmp_path / "p_otu_samples.txt")) == table and sc.read_otu_samples_ppm(str(tmp_path / "p_otu_samples_ppm.txt")) == ppm


def test_join_refuses_tables_that_do_not_fit_and_writes_nothing(tmp_path):
    cov = sc.parse_samplecov(cov_text())
    clust = clustlib.parse_clust(CLUST)
    with pytest.raises(ValueError, match="record 1 is 'a1' in the nucleotide file and 'zz' in the cluster table"):
        sc.join(cov, clustlib.parse_clust(CLUST.replace("a1\tmember", "zz\tmember")))
    with pytest.raises(ValueError, match="7 nucleotide records, 8 lines"):
        sc.join(dict(cov, rows=cov["rows"][:7]), clust)
    (tmp_path / "n_samplecov.txt").write_text(cov_text(names=["a0", "zz"] + NAMES[2:]))
    (tmp_path / "p_clust.txt").write_text(CLUST)
    r = subprocess.run([sys.executable, "-m", "megagta_amd.samplecov", str(tmp_path / "p"), str(tmp_path / "n_samplecov.txt"), str(tmp_path / "p_clust.txt")],
                       capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert r.returncode == 1 and "samplecov: record 1 is 'zz'" in r.stderr and sorted(os.listdir(tmp_path)) == ["n_samplecov.txt", "p_clust.txt"]
    (tmp_path / "n_samplecov.txt").write_text(cov_text())
    r = subprocess.run([sys.executable, "-m", "megagta_amd.samplecov", str(tmp_path / "p"), str(tmp_path / "n_samplecov.txt"), str(tmp_path / "p_clust.txt")],
                       capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert r.returncode == 0 and "4 clusters x 3 libraries" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["n_samplecov.txt", "p_clust.txt", "p_otu_samples.txt", "p_otu_samples_ppm.txt"]
    r = subprocess.run([sys.executable, "-m", "megagta_amd.samplecov", "x"], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert r.returncode == 2 and "Usage" in r.stderr


# ---- the driver and the library -------------------------------------------------------------------------------------------------------
def test_driver_sample_abund_needs_align_and_cluster(tmp_path):
    (tmp_path / "r.fa").write_text(">r\nACGT\n")
    (tmp_path / "g.txt").write_text("")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "r.fa"), "-g", str(tmp_path / "g.txt"), "-o", str(tmp_path / "out")]
    for flags in (["--sample-abund"], ["--sample-abund", "--align"], ["--sample-abund", "--nearest", "--chimera"]):
        r = subprocess.run(base + flags, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--sample-abund needs --align --cluster" in r.stderr, r.stderr
        assert not (tmp_path / "out").exists()
    r = subprocess.run([sys.executable, DRIVER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--sample-abund" in r.stdout


def test_library_and_header_have_the_symbol():
    assert "mgta_contig_sample_coverage" in _lib.SYMBOLS and len(_lib.SYMBOLS["mgta_contig_sample_coverage"][1]) == 14
    header = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    assert "int mgta_contig_sample_coverage(mgta_sdbg *, const mgta_reads *reads, int reads_reversed, const uint64_t *lib_end" in header
    assert "typedef struct mgta_sample_cov_stats {" in header
    fields = H.header_fields("mgta_sample_cov_stats", header)
    assert fields == [n for n, _ in _lib.SampleCovStats._fields_] and ctypes.sizeof(_lib.SampleCovStats) == 8 * len(fields)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mgta_contig_sample_coverage")
