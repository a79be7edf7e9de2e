"""Gapped pileup without a device: gapped.py's event rule, listing rule, writer and readers, as_read_place(); the header against the
ctypes mirrors; the driver's usage errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from megagta_amd import _lib, gapped as gp, pileup as pl
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def made_result():
    """two contigs, four reads, five hand-made gap records"""
    seqs = ["ACGTACGTAC", "ttgacca"]
    reads = ["ACGGGTAC", "GTACCC", np.array([0, 1, 2, 2, 2, 3], dtype=np.uint8), "TGGTTCAA"]     # read 3 lies on contig 1 reversed: TTGAACCA
    offsets = np.array([0, 10, 17], dtype=np.int64)
    counts = np.zeros((17, 4), dtype=np.uint32)
    counts[3] = (1, 0, 2, 4)
    counts[5] = (0, 3, 0, 0)
    counts[14] = (2, 2, 0, 0)
    gaps = np.array([(0, 0, 3, -2, 3, 0, 1),                                   # GG in front of contig 0's position 3 (read 0, b = 3)
                     (2, 0, 3, -2, 3, 0, 0),                                   # the same event from read 2
                     (1, 0, 5, 2, 4, 0, 1),                                    # CG deleted at position 5
                     (3, 1, 4, -1, 4, 1, 1),                                   # read 3 in orientation 1 = TTGAACCA: its letter 4 = A
                     (0, 0, 3, 2, 3, 0, 1)], dtype=gp.GAP_DTYPE)               # a deletion of 2 at the same position: another event
    rec = np.zeros(2, dtype=pl.CONTIG_DTYPE)
    rec["len"] = (10, 7)
    return seqs, reads, dict(counts=counts, uniq=np.zeros(17, dtype=np.uint32), contigs=rec, offsets=offsets, gaps=gaps)


def test_the_event_rule():
    seqs, reads, res = made_result()
    evs = gp.events(res["gaps"], seqs, reads, res["counts"], res["offsets"])
    assert evs == [dict(contig=0, pos=3, type="ins", len=2, seq="GG", reads=2, unique=1, depth=7),
                   dict(contig=0, pos=3, type="del", len=2, seq="TA", reads=1, unique=1, depth=7),
                   dict(contig=0, pos=5, type="del", len=2, seq="CG", reads=1, unique=1, depth=3),
                   dict(contig=1, pos=4, type="ins", len=1, seq="A", reads=1, unique=1, depth=4)]
    assert gp.read_letters("AACG", 1) == "CGTT" and gp.read_letters(np.array([0, 0, 1, 2]), 0) == "AACG"
    assert gp.events(res["gaps"][:0], seqs, reads, res["counts"], res["offsets"]) == []


def test_the_listing_rule():
    assert gp.min_reads() == 1 and gp.min_reads(8, 100) == 1 and gp.min_reads(8, 126) == 2 and gp.min_reads(20, 100) == 2 and gp.min_reads(0, 0) == 1
    assert gp.min_reads(21, 100) == 3 and gp.min_reads(1000, 1000) == 1000
    seqs, reads, res = made_result()
    evs = gp.events(res["gaps"], seqs, reads, res["counts"], res["offsets"])
    text = gp.format_indels(["c0", "c1"], evs, min_depth=20, min_alt_permille=100)
    assert text == gp.INDEL_HEADER + "c0\t4\tins\t2\tGG\t2\t1\t7\n"
    assert gp.INDEL_HEADER == "#contig\tpos\ttype\tlen\tseq\treads\tunique\tdepth\n"


def test_the_four_files_and_the_round_trip(tmp_path):
    seqs, reads, res = made_result()
    names = ["c0", "c1"]
    paths = gp.write_gapped(str(tmp_path / "x"), names, seqs, res, reads, min_depth=1)
    assert [os.path.basename(p) for p in paths] == ["x_pileup.txt", "x_pileup_variants.txt", "x_pileup_indels.txt"]
    text = open(paths[2]).read()
    assert text == (gp.INDEL_HEADER + "c0\t4\tins\t2\tGG\t2\t1\t7\nc0\t4\tdel\t2\tTA\t1\t1\t7\nc0\t6\tdel\t2\tCG\t1\t1\t3\nc1\t5\tins\t1\tA\t1\t1\t4\n")
    rows = gp.read_indels(paths[2])
    assert rows[0] == dict(contig="c0", pos=4, type="ins", len=2, seq="GG", reads=2, unique=1, depth=7) and len(rows) == 4
    assert open(paths[0]).read() == pl.format_pileup(names, seqs, res, min_depth=1)["summary"]
    texts = gp.format_gapped(names, seqs, res, reads, min_depth=1, per_base=True)
    assert texts["depth"] is not None and texts["indels"] == text
    for bad in ("", "#contig\tpos\n", gp.INDEL_HEADER + "c0\t4\tins\t3\tGG\t2\t1\t7\n", gp.INDEL_HEADER + "c0\t4\tsub\t2\tGG\t2\t1\t7\n",
                gp.INDEL_HEADER + "c0\t4\tins\t2\tGG\t1\t2\t7\n", gp.INDEL_HEADER + "c0\t4\tins\t2\tGG\t2\t1\n"):
        with pytest.raises(ValueError):
            gp.parse_indels(bad)
    assert gp.main([paths[2]]) == 0 and gp.main([]) == 2 and gp.main([str(tmp_path / "none")]) == 1


def test_as_read_place():
    places = np.array([(50, 2, 10, 0, 1, 0, 10, 0),                            # ungapped, placed once: kept
                       (44, 2, 10, 1, 1, 1, 13, 30),                           # gapped: no allele
                       (0, -1, 0, 0, 0, 0, 0, 0),                              # not placed
                       (60, 0, -4, 0, 2, 0, -4, 0),                            # ungapped lowest of two
                       (60, 0, 7, 0, 2, 0, 5, 41)], dtype=gp.PLACE_DTYPE)      # gapped lowest of two
    out = gp.as_read_place(places)
    assert out.dtype == pl.READ_DTYPE and out["n_placed"].tolist() == [1, 0, 0, 2, 0]
    for f in ("score", "contig", "diag", "orient", "n_mismatch"):
        assert out[f].tolist() == places[f].tolist()
    assert gp.as_read_place(places[:0]).shape == (0,)


def test_header_declares_the_entry_and_the_structures_match():
    hdr = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    assert re.search(r"int mgta_reads_pileup_gapped\(mgta_sdbg \*, const mgta_reads \*reads, int reads_reversed, uint64_t n_short_reads", hdr)
    assert "mgta_reads_pileup_gapped" in _lib.SYMBOLS and len(_lib.SYMBOLS["mgta_reads_pileup_gapped"][1]) == 15

    def fields(name):
        return [(ctype, member) for ctype, member, _ in H.header_structs(hdr)[name]]
    size = {"int32_t": 4, "uint32_t": 4, "int64_t": 8, "uint64_t": 8, "double": 8}
    assert [n for _, n in fields("mgta_gapped_params")] == [n for n, _ in _lib.GappedParams._fields_] and C.sizeof(_lib.GappedParams) == 24
    assert [n for _, n in fields("mgta_gapped_stats")] == [n for n, _ in _lib.GappedStats._fields_]
    assert sum(size[t] for t, _ in fields("mgta_gapped_stats")) == C.sizeof(_lib.GappedStats) == C.sizeof(_lib.PileupStats) + 7 * 8
    assert [n for n, _ in _lib.GappedStats._fields_[:len(_lib.PileupStats._fields_)]] == [n for n, _ in _lib.PileupStats._fields_]
    for name, dtype in (("mgta_gap_place", gp.PLACE_DTYPE), ("mgta_gap_rec", gp.GAP_DTYPE)):
        f = fields(name)
        assert [n for _, n in f] == list(dtype.names) and sum(size[t] for t, _ in f) == dtype.itemsize == 32
        assert [size[t] for t, _ in f] == [dtype[n].itemsize for n in dtype.names]
    assert list(gp.PLACE_DTYPE.names[:6]) == list(pl.READ_DTYPE.names)
    for word in ("max_gap", "gap_open", "gap_extend", "left-aligned", "One-gap candidate", "What it is not"):
        assert word in hdr, word


def test_driver_usage_errors_of_gapped(tmp_path, capsys):
    from megagta_amd import megagta as drv
    (tmp_path / "reads.fa").write_text(">r\nACGT\n")
    (tmp_path / "genes.txt").write_text("")
    base = ["megagta.py", "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "genes.txt"), "-o", str(tmp_path / "out")]
    for flag in ("--max-gap", "--gap-open", "--gap-extend"):
        drv.opt = drv.Opt()
        assert drv.main(base + ["--pileup", flag, "3"]) == 2
        assert flag + " needs --gapped" in capsys.readouterr().err
        drv.opt = drv.Opt()
        assert drv.main(base + ["--pileup", "--gapped", flag, "-3"]) == 2
        assert "a count is expected" in capsys.readouterr().err
        drv.opt = drv.Opt()
        assert drv.main(base + ["--pileup", "--gapped", flag, "256"]) == 2
        assert "at most 255" in capsys.readouterr().err
    drv.opt = drv.Opt()
    assert drv.main(base + ["--gapped"]) == 2
    assert "--gapped needs --pileup" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "out")
    drv.opt = drv.Opt()
    drv.parse_opt(base[1:] + ["--pileup", "--gapped", "--max-gap", "12", "--gap-open", "6"])
    drv.check_opt()
    assert drv.opt.gapped and drv.opt.gapped_opts == {"--max-gap": 12, "--gap-open": 6}
    drv.opt = drv.Opt()
    for flag in ("--gapped", "--max-gap", "--gap-open", "--gap-extend"):
        assert flag in drv.USAGE
