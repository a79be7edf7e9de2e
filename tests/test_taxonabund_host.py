"""megagta_amd/taxonabund.py without a device: the integer formatting, the writers and readers, the join with every branch, and the
driver's usage error.  Expected numbers are worked out here by hand or with fractions.Fraction, never taken from the module."""
import ctypes
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from megagta_amd import _lib
from megagta_amd import chimera as chimlib
from megagta_amd import cluster as clustlib
from megagta_amd import nearest as nearlib
from megagta_amd import taxonabund as ta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")


@pytest.mark.parametrize("mass", [0, 1, 6, 7, 65535, 65536, 65537, 300 * 65536 // 7, 1 << 63, (1 << 64) - 1])
def test_mass_is_printed_by_integers_only(mass):
    exact = Fraction(mass, 65536)
    q = int(exact * 10000)                                                # floor: the value is not negative
    want = "%d.%04d" % (q // 10000, q % 10000)
    got = ta.q16_text(mass)
    assert got == want and ta.parse_e4(got) == q == ta.q16_to_e4(mass)
    assert Fraction(q, 10000) <= exact < Fraction(q + 1, 10000)
    if mass < 1 << 40:                                                    # where a double holds the value, the usual formatting agrees up to the rounding
        assert abs(float(got) - mass / 65536) < 1e-4
    assert {0: "0.0000", 1: "0.0000", 7: "0.0001", 65535: "0.9999", 65536: "1.0000", (1 << 64) - 1: "281474976710655.9999",
            1 << 63: "140737488355328.0000"}.get(mass, got) == got


def test_mass_outside_64_bits_is_refused():
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            ta.q16_text(bad)
    for bad in ("1", "1.5", "1.00000", "-1.0000", "1,0000", "a.0000", ""):
        with pytest.raises(ValueError):
            ta.parse_e4(bad)


# ---- hand-written tables --------------------------------------------------------------------------------------------------------------
# eight nucleotide records; clusters 0 = {a0 (rep), a1, a2}, 3 = {b0 (rep), b1}, 5 = {c0}, 6 = {d0}; u0 is unaligned
NAMES = ["a0", "a1", "a2", "b0", "u0", "c0", "d0", "b1"]
MASS_Q16 = [10 * 65536, 65536 // 3, 7, 5 * 65536 + 1, 2 * 65536, 65536 // 7, 3 * 65536, 0]
CLUST = clustlib.CLUST_HEADER + "".join(line + "\n" for line in (
    "a0\trep\t0\ta0\t90\t0\t90", "a1\tmember\t0\ta0\t80\t0\t80", "a2\tmember\t0\ta0\t70\t1\t70", "b0\trep\t3\tb0\t90\t0\t90", "u0\tunaligned\t-\t-\t0\t0\t0",
    "c0\trep\t5\tc0\t60\t0\t60", "d0\trep\t6\td0\t60\t0\t60", "b1\tmember\t3\tb0\t50\t0\t50"))
NEAREST = nearlib.NEAREST_HEADER + "".join(line + "\n" for line in (
    "a0\taligned\tR1\t400\t0.9778\t90\t100\t0\t90\t88\t86\t1\t1", "b0\taligned\tR3\t300\t0.8000\t90\t95\t0\t90\t90\t72\t0\t0",
    "c0\tunaligned\t-\t0\t0.0000\t60\t0\t0\t0\t0\t0\t0\t0", "d0\taligned\tR1\t200\t0.7500\t60\t100\t5\t65\t60\t45\t0\t0"))
CHIMERA = chimlib.CHIMERA_HEADER + "".join(line + "\n" for line in (
    "a0\tclean\tR1\t400\t90\t40\tR1\t200\tR3\t190\t390\t400\t-10", "b0\tchimeric\tR3\t300\t90\t45\tR1\t200\tR3\t180\t380\t300\t80",
    "c0\tunchecked\t-\t0\t60\t0\t-\t0\t-\t0\t0\t0\t0", "d0\tclean\tR1\t200\t60\t30\tR1\t100\tR2\t90\t190\t200\t-10"))
REFS = ">R1 Bacteria;Firmicutes; Bacillus subtilis\nMKV\n>R2\nMKL\n>R3\tArchaea  \nMRV\n"


def share_rows(masses=MASS_Q16):
    recs = [dict(len=100 + i, n_windows=60 + i, n_covered=(50 if m else 0), n_unique=(5 if m else 0), max_share=(9 if m else 0), mass=m) for i, m in enumerate(masses)]
    text = ta.sharecov_text(NAMES, recs)
    return text, ta.parse_sharecov(text)


def test_writers_and_readers_round_trip(tmp_path):
    text, rows = share_rows()
    assert text.splitlines()[0] == "#contig\tlen\twindows\tcovered\tunique\tmax_share\tmass"
    assert text.splitlines()[2] == "a1\t101\t61\t50\t5\t9\t0.3333" and text.splitlines()[8] == "b1\t107\t67\t0\t0\t0\t0.0000"
    assert [r["contig"] for r in rows] == NAMES and [r["mass"] for r in rows] == [100000, 3333, 1, 50000, 20000, 1428, 30000, 0]
    assert ta.sharecov_text(NAMES, np.array([(m, 100 + i, 60 + i, 50 if m else 0, 5 if m else 0, 9 if m else 0, 0) for i, m in enumerate(MASS_Q16)],
                                            dtype=[(n, "<u8" if n == "mass" else "<u4") for n in ("mass", "len", "n_windows", "n_covered", "n_unique", "max_share", "reserved_")])) == text
    (tmp_path / "x_sharecov.txt").write_text(text)
    assert ta.read_sharecov(str(tmp_path / "x_sharecov.txt")) == rows
    otu, taxon = ta.join(rows, clustlib.parse_clust(CLUST), nearlib.parse_nearest(NEAREST), chimlib.parse_chimera(CHIMERA), ta.parse_ref_headers(REFS))
    assert ta.parse_otu(ta.otu_text(otu)) == otu and ta.parse_taxon(ta.taxon_text(taxon)) == taxon
    (tmp_path / "x_otu_abund.txt").write_text(ta.otu_text(otu))
    (tmp_path / "x_taxon_abund.txt").write_text(ta.taxon_text(taxon))
    assert ta.read_otu(str(tmp_path / "x_otu_abund.txt")) == otu and ta.read_taxon(str(tmp_path / "x_taxon_abund.txt")) == taxon
    assert ta.parse_ref_headers(REFS) == [("R1", "Bacteria;Firmicutes; Bacillus subtilis"), ("R2", "-"), ("R3", "Archaea")]
    assert nearlib.parse_refs(REFS)[0] == ["R1", "R2", "R3"]              # the reader of the nearest step is what it was


def test_join_every_branch():
    _, rows = share_rows()
    total = 100000 + 3333 + 1 + 50000 + 20000 + 1428 + 30000
    otu, taxon = ta.join(rows, clustlib.parse_clust(CLUST), nearlib.parse_nearest(NEAREST), chimlib.parse_chimera(CHIMERA), ta.parse_ref_headers(REFS))
    assert ta.otu_text(otu) == ta.OTU_HEADER + "".join(line + "\n" for line in (
        "0\ta0\t3\t10.3334\t%d\tR1\t0.9778\tclean" % (103334 * 10**6 // total),
        "3\tb0\t2\t5.0000\t%d\tR3\t0.8000\tchimeric" % (50000 * 10**6 // total),
        "5\tc0\t1\t0.1428\t%d\t-\t0.0000\tunchecked" % (1428 * 10**6 // total),        # its representative is unaligned in the nearest table
        "6\td0\t1\t3.0000\t%d\tR1\t0.7500\tclean" % (30000 * 10**6 // total),
        "-\t-\t1\t2.0000\t%d\t-\t0.0000\t-" % (20000 * 10**6 // total)))
    assert ta.taxon_text(taxon) == ta.TAXON_HEADER + "".join(line + "\n" for line in (
        "R1\t2\t4\t13.3334\t%d\tBacteria;Firmicutes; Bacillus subtilis" % (133334 * 10**6 // total),
        "R2\t0\t0\t0.0000\t0\t-",                                         # a reference with no cluster
        "R3\t0\t0\t0.0000\t0\tArchaea",                                   # its only cluster is chimeric
        "#chimeric\t1\t2\t5.0000\t%d\t-" % (50000 * 10**6 // total),
        "#unassigned\t1\t2\t2.1428\t%d\t-" % (21428 * 10**6 // total)))
    # masses are conserved across both tables, the ppm are floors
    assert sum(r["mass"] for r in otu) == total == sum(r["mass"] for r in taxon) == sum(r["mass"] for r in rows)
    assert sum(r["contigs"] for r in otu) == len(NAMES) == sum(r["contigs"] for r in taxon)
    assert 10**6 - len(otu) < sum(r["ppm"] for r in otu) <= 10**6 and 10**6 - len(taxon) < sum(r["ppm"] for r in taxon) <= 10**6
    # no chimera table: `-`, and the chimeric cluster stays with its reference
    otu_nc, taxon_nc = ta.join(rows, clustlib.parse_clust(CLUST), nearlib.parse_nearest(NEAREST), None, ta.parse_ref_headers(REFS))
    assert [r["chimera"] for r in otu_nc] == ["-"] * 5 and [r["mass"] for r in taxon_nc] == [133334, 0, 50000, 0, 21428]
    assert sum(r["mass"] for r in taxon_nc) == total
    # no nearest table: no taxon table, `-` and 0.0000
    otu_nn, taxon_nn = ta.join(rows, clustlib.parse_clust(CLUST), None, chimlib.parse_chimera(CHIMERA))
    assert taxon_nn is None and [(r["ref"], r["identity"]) for r in otu_nn] == [(None, "0.0000")] * 5
    assert [r["chimera"] for r in otu_nn] == ["clean", "chimeric", "unchecked", "clean", "-"] and sum(r["mass"] for r in otu_nn) == total
    # neither
    otu_0, taxon_0 = ta.join(rows, clustlib.parse_clust(CLUST))
    assert taxon_0 is None and [r["mass"] for r in otu_0] == [103334, 50000, 1428, 30000, 20000]
    # total 0: every ppm is 0, nothing divides
    _, zero = share_rows([0] * 8)
    otu_z, taxon_z = ta.join(zero, clustlib.parse_clust(CLUST), nearlib.parse_nearest(NEAREST), chimlib.parse_chimera(CHIMERA), ta.parse_ref_headers(REFS))
    assert all(r["ppm"] == 0 and r["mass"] == 0 for r in otu_z + taxon_z) and len(otu_z) == 5 and len(taxon_z) == 5
    # no unaligned record: no last line
    clust_all = CLUST.replace("u0\tunaligned\t-\t-\t0\t0\t0", "u0\trep\t4\tu0\t9\t0\t9")
    otu_a, _ = ta.join(rows, clustlib.parse_clust(clust_all))
    assert [r["cluster"] for r in otu_a] == [0, 3, 4, 5, 6]


def test_tables_that_do_not_fit_are_refused_and_nothing_is_written(tmp_path):
    text, rows = share_rows()
    clust = clustlib.parse_clust(CLUST)
    with pytest.raises(ValueError, match="7 nucleotide records, 8 lines"):
        ta.join(rows[:-1], clust)
    swapped = [dict(r) for r in rows]
    swapped[1]["contig"], swapped[2]["contig"] = "a2", "a1"
    with pytest.raises(ValueError, match="record 1 is 'a2' in the nucleotide file and 'a1' in the cluster table"):
        ta.join(swapped, clust)
    with pytest.raises(ValueError, match="needs the reference file"):
        ta.join(rows, clust, nearlib.parse_nearest(NEAREST))
    with pytest.raises(ValueError, match="'d0' has no line in the nearest table"):
        ta.join(rows, clust, nearlib.parse_nearest(NEAREST.rsplit("d0", 1)[0]), None, ta.parse_ref_headers(REFS))
    with pytest.raises(ValueError, match="'d0' has no line in the chimera table"):
        ta.join(rows, clust, None, chimlib.parse_chimera(CHIMERA.rsplit("d0", 1)[0]))
    with pytest.raises(ValueError, match="names 'R3'"):
        ta.join(rows, clust, nearlib.parse_nearest(NEAREST), None, ta.parse_ref_headers(REFS)[:2])
    # through the files: the names differ -> an error and no output file
    (tmp_path / "n_sharecov.txt").write_text(text.replace("a2\t", "zz\t"))
    (tmp_path / "p_clust.txt").write_text(CLUST)
    with pytest.raises(ValueError, match="record 2"):
        ta.write_taxonabund(str(tmp_path / "p"), str(tmp_path / "n_sharecov.txt"), str(tmp_path / "p_clust.txt"))
    assert sorted(os.listdir(tmp_path)) == ["n_sharecov.txt", "p_clust.txt"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "megagta_amd.taxonabund", str(tmp_path / "p"), str(tmp_path / "n_sharecov.txt"), str(tmp_path / "p_clust.txt")],
                       capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 1 and "record 2" in r.stderr and sorted(os.listdir(tmp_path)) == ["n_sharecov.txt", "p_clust.txt"]
    # and the good files give both tables
    (tmp_path / "n_sharecov.txt").write_text(text)
    for name, body in (("p_rep_seqs_nearest.txt", NEAREST), ("p_rep_seqs_chimera.txt", CHIMERA), ("refs.faa", REFS)):
        (tmp_path / name).write_text(body)
    res = ta.write_taxonabund(str(tmp_path / "p"), str(tmp_path / "n_sharecov.txt"), str(tmp_path / "p_clust.txt"), str(tmp_path / "p_rep_seqs_nearest.txt"),
                              str(tmp_path / "p_rep_seqs_chimera.txt"), str(tmp_path / "refs.faa"))
    assert res["total"] == 204762 and ta.read_otu(str(tmp_path / "p_otu_abund.txt")) == res["otu"] and ta.read_taxon(str(tmp_path / "p_taxon_abund.txt")) == res["taxon"]


@pytest.mark.parametrize("bad", [
    "a0\t100\t60\t50\t5\t9",                      # a column short
    "a0\t100\t60\t50\t5\t9\t1.5",                 # not four decimals
    "a0\t100\t60\t50\t5\t9\t1e3",
    "a0\t100\t60\t61\t5\t9\t1.0000",              # more covered than windows
    "a0\t100\t60\t50\t51\t9\t1.0000",             # more unique than covered
    "a0\t100\t60\t0\t0\t0\t1.0000",               # mass without a covered window
    "a0\t100\t60\t50\t5\t0\t1.0000",              # covered windows without a share
    "a0\t-1\t60\t50\t5\t9\t1.0000",
])
def test_sharecov_reader_refuses_malformed_lines(bad):
    with pytest.raises(ValueError):
        ta.parse_sharecov(ta.SHARECOV_HEADER + bad + "\n")
    with pytest.raises(ValueError, match="header"):
        ta.parse_sharecov(bad + "\n")
    assert ta.parse_sharecov(ta.SHARECOV_HEADER) == []


def test_table_readers_refuse_malformed_lines():
    good_otu = "0\ta0\t3\t10.3334\t504000\tR1\t0.9778\tclean\n-\t-\t1\t2.0000\t97000\t-\t0.0000\t-\n"
    assert len(ta.parse_otu(ta.OTU_HEADER + good_otu)) == 2
    for bad in ("0\ta0\t3\t10.3334\t504000\tR1\t0.9778", "0\ta0\t3\t10.33\t504000\tR1\t0.9778\tclean", "0\ta0\t3\t10.3334\t1000001\tR1\t0.9778\tclean",
                "0\ta0\t3\t10.3334\t504000\tR1\t0.9778\tmaybe", "0\ta0\t0\t10.3334\t504000\tR1\t0.9778\tclean", "0\t-\t3\t10.3334\t504000\tR1\t0.9778\tclean",
                "0\ta0\t3\t10.3334\t504000\t-\t0.9778\tclean", "x\ta0\t3\t10.3334\t504000\tR1\t0.9778\tclean", "0\ta0\t3\t10.3334\t504000\tR1\t1\tclean",
                "-\t-\t1\t2.0000\t97000\tR1\t0.0000\t-", "-\t-\t0\t0.0000\t0\t-\t0.0000\t-"):
        with pytest.raises(ValueError):
            ta.parse_otu(ta.OTU_HEADER + bad + "\n")
    with pytest.raises(ValueError):                                       # the unaligned records are the last line
        ta.parse_otu(ta.OTU_HEADER + "".join(reversed(good_otu.splitlines(True))))
    with pytest.raises(ValueError, match="header"):
        ta.parse_otu(good_otu)
    tail = "#chimeric\t0\t0\t0.0000\t0\t-\n#unassigned\t0\t0\t0.0000\t0\t-\n"
    assert len(ta.parse_taxon(ta.TAXON_HEADER + "R1\t2\t4\t13.3334\t651000\tBacteria; x\n" + tail)) == 3
    for bad in ("R1\t2\t4\t13.3334\t651000", "R1\t2\t4\t13.3334\t651000\t", "R1\t5\t4\t13.3334\t651000\t-", "R1\t0\t0\t1.0000\t5\t-", "R1\t2\t4\t13\t651000\t-",
                "R1\t2\t4\t13.3334\t-5\t-"):
        with pytest.raises(ValueError):
            ta.parse_taxon(ta.TAXON_HEADER + bad + "\n" + tail)
    with pytest.raises(ValueError, match="#chimeric and #unassigned"):
        ta.parse_taxon(ta.TAXON_HEADER + "R1\t2\t4\t13.3334\t651000\t-\n")
    with pytest.raises(ValueError, match="header"):
        ta.parse_taxon(tail)


def test_driver_taxon_abund_needs_align_and_cluster(tmp_path):
    (tmp_path / "r.fa").write_text(">r\nACGT\n")
    (tmp_path / "g.txt").write_text("")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "r.fa"), "-g", str(tmp_path / "g.txt"), "-o", str(tmp_path / "out")]
    for flags in (["--taxon-abund"], ["--taxon-abund", "--align"], ["--taxon-abund", "--nearest", "--chimera"]):
        r = subprocess.run(base + flags, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--taxon-abund needs --align --cluster" in r.stderr, r.stderr
        assert not (tmp_path / "out").exists()
    r = subprocess.run(base + ["--cluster"], capture_output=True, text=True, timeout=60)          # (the wording it follows)
    assert r.returncode == 2 and "--cluster needs --align" in r.stderr
    r = subprocess.run([sys.executable, DRIVER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--taxon-abund" in r.stdout


def test_library_has_the_share_symbols():
    assert {"mgta_contig_share_coverage", "mgta_ctx_set_share_hash_bits"} <= set(_lib.SYMBOLS)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgta_contig_share_coverage", "mgta_ctx_set_share_hash_bits"):
        assert hasattr(lib, name), name
    assert ctypes.sizeof(_lib.ContigShare) == 32 and ctypes.sizeof(_lib.ShareStats) == 16 * 8
    from megagta_amd import api
    assert api.SHARE_DTYPE.itemsize == 32 and [api.SHARE_DTYPE.fields[n][1] for n, _ in _lib.ContigShare._fields_] == [getattr(_lib.ContigShare, n).offset for n, _ in _lib.ContigShare._fields_]
