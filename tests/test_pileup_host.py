"""CPU-only: the variant rule and the writers and readers of the pileup files (megagta_amd/pileup.py) on a fixed small counts array, the
driver's usage errors around --pileup, and the header's declaration of the entry."""
import os
import re

import numpy as np
import pytest

from megagta_amd import _lib
from megagta_amd import pileup as pl
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["c1", "empty", "c3"]
SEQS = ["ACgTN", "", "TT"]


def fixed_result():
    """what Graph.pileup would return for SEQS: five positions, none, two"""
    counts = np.array([[10, 0, 0, 0],        # A: all reads agree
                       [1, 8, 0, 0],         # C: alt 1 of 9 = 111 permille: listed
                       [0, 0, 7, 7],         # g (lower case): alt 7 of 14
                       [1, 0, 0, 6],         # T: depth 7 is below 8
                       [0, 3, 3, 3],         # N: no base, alt = depth 9
                       [0, 0, 0, 0],         # T: no read
                       [1, 0, 0, 19]],       # T: alt 1 of 20 = 50 permille: not listed
                      dtype=np.uint32)
    uniq = np.array([10, 9, 3, 7, 0, 0, 20], dtype=np.uint32)
    rec = np.zeros(3, dtype=pl.CONTIG_DTYPE)
    rec[0] = (5, 5, 7, 14, 12, 9, 49, 17)
    rec[1] = (0, 0, 0, 0, 0, 0, 0, 0)
    rec[2] = (2, 1, 0, 20, 20, 20, 20, 1)
    return dict(counts=counts, uniq=uniq, contigs=rec, offsets=np.array([0, 5, 5, 7], dtype=np.int64))


def test_the_variant_rule():
    res = fixed_result()
    assert pl.variant_mask(SEQS[0], res["counts"][:5]).tolist() == [False, True, True, False, True]
    assert pl.variant_mask(SEQS[2], res["counts"][5:]).tolist() == [False, False]
    assert pl.variant_mask(SEQS[1], res["counts"][5:5]).tolist() == []
    assert pl.variant_mask(SEQS[0], res["counts"][:5], min_depth=7).tolist() == [False, True, True, True, True]      # 1 of 7 = 142 permille
    assert pl.variant_mask(SEQS[2], res["counts"][5:], min_depth=0, min_alt_permille=50).tolist() == [True, True]    # depth 0: 0 >= 0
    assert pl.variant_mask(SEQS[0], res["counts"][:5], min_alt_permille=112).tolist() == [False, False, True, False, True]
    assert pl.variant_mask(SEQS[0].encode(), res["counts"][:5]).tolist() == [False, True, True, False, True]


def test_the_three_files_and_the_round_trip(tmp_path):
    res = fixed_result()
    t = pl.format_pileup(NAMES, SEQS, res, per_base=True)
    assert t["summary"] == ("#contig\tlen\treads\tunique\tcovered\tmin\tmax\tmean\tmismatches\tvariants\n"
                            "c1\t5\t12\t9\t5\t7\t14\t9.8000\t17\t3\n"
                            "empty\t0\t0\t0\t0\t0\t0\t0.0000\t0\t0\n"
                            "c3\t2\t20\t20\t1\t0\t20\t10.0000\t1\t0\n")
    assert t["variants"] == ("#contig\tpos\tref\tdepth\tA\tC\tG\tT\tunique\n"
                             "c1\t2\tC\t9\t1\t8\t0\t0\t9\n"
                             "c1\t3\tg\t14\t0\t0\t7\t7\t3\n"
                             "c1\t5\tN\t9\t0\t3\t3\t3\t0\n")
    assert t["depth"].splitlines()[1:] == ["c1\t1\tA\t10\t10\t0\t0\t0\t10", "c1\t2\tC\t9\t1\t8\t0\t0\t9", "c1\t3\tg\t14\t0\t0\t7\t7\t3", "c1\t4\tT\t7\t1\t0\t0\t6\t7",
                                           "c1\t5\tN\t9\t0\t3\t3\t3\t0", "c3\t1\tT\t0\t0\t0\t0\t0\t0", "c3\t2\tT\t20\t1\t0\t0\t19\t20"]
    assert pl.format_pileup(NAMES, SEQS, res)["depth"] is None
    # the mean is floored: 49 / 5 = 9.8 exactly, 1 / 3 = 0.3333
    third = dict(counts=np.array([[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.uint32), uniq=np.zeros(3, dtype=np.uint32),
                 contigs=np.array([(3, 1, 0, 1, 1, 0, 1, 0)], dtype=pl.CONTIG_DTYPE), offsets=np.array([0, 3], dtype=np.int64))
    assert pl.format_pileup(["x"], ["AAA"], third)["summary"].splitlines()[1] == "x\t3\t1\t0\t1\t0\t1\t0.3333\t0\t0"
    # the round trip through the files
    prefix = str(tmp_path / "g")
    paths = pl.write_pileup(prefix, NAMES, SEQS, res, per_base=True)
    assert [os.path.basename(p) for p in paths] == ["g_pileup.txt", "g_pileup_variants.txt", "g_pileup_depth.txt"]
    assert [open(p).read() for p in paths] == [t["summary"], t["variants"], t["depth"]]
    assert [os.path.basename(p) for p in pl.write_pileup(str(tmp_path / "h"), NAMES, SEQS, res)] == ["h_pileup.txt", "h_pileup_variants.txt"]
    rows = pl.parse_summary(open(paths[0]).read())
    assert [r["contig"] for r in rows] == NAMES and [r["len"] for r in rows] == [5, 0, 2] and [r["mean_e4"] for r in rows] == [98000, 0, 100000]
    assert [(r["reads"], r["unique"], r["covered"], r["min"], r["max"], r["mismatches"], r["variants"]) for r in rows] == [(12, 9, 5, 7, 14, 17, 3), (0,) * 7, (20, 20, 1, 0, 20, 1, 0)]
    var, depth = pl.parse_bases(open(paths[1]).read()), pl.parse_bases(open(paths[2]).read())
    assert [(r["contig"], r["pos"], r["ref"]) for r in var] == [("c1", 2, "C"), ("c1", 3, "g"), ("c1", 5, "N")]
    assert [[r[b] for b in "ACGT"] for r in depth] == res["counts"].tolist() and [r["unique"] for r in depth] == res["uniq"].tolist()
    assert [r for r in depth if (r["contig"], r["pos"]) in {(v["contig"], v["pos"]) for v in var}] == var
    with pytest.raises(ValueError, match="header"):
        pl.parse_summary(t["variants"])
    with pytest.raises(ValueError, match="header"):
        pl.parse_bases(t["summary"])
    with pytest.raises(ValueError, match=r"A \+ C \+ G \+ T"):
        pl.parse_bases(pl.BASE_HEADER + "c\t1\tA\t5\t1\t1\t1\t1\t0\n")
    with pytest.raises(ValueError, match="other sequences"):
        pl.format_pileup(NAMES, ["ACGT", "", "TT"], res)
    with pytest.raises(ValueError, match="differ in number"):
        pl.format_pileup(NAMES[:2], SEQS[:2], res)


def test_read_fasta_names_and_letters(tmp_path):
    p = tmp_path / "x.fa"
    p.write_text("junk\n>a first record \nAC\n gT\t\n\n>b\tx\n>\nNN\n")
    assert pl.read_fasta(str(p)) == (["a", "b", ""], ["ACgT", "", "NN"])


def test_driver_usage_errors_of_pileup(tmp_path, capsys):
    from megagta_amd import megagta as drv
    (tmp_path / "reads.fa").write_text(">r\nACGT\n")
    (tmp_path / "genes.txt").write_text("")
    base = ["megagta.py", "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "genes.txt"), "-o", str(tmp_path / "out")]
    for flag in ("--min-anchors", "--min-overlap", "--max-mismatch-permille", "--min-depth", "--min-alt-permille"):
        drv.opt = drv.Opt()
        assert drv.main(base + [flag, "3"]) == 2
        assert flag + " needs --pileup" in capsys.readouterr().err
        drv.opt = drv.Opt()
        assert drv.main(base + ["--pileup", flag, "-3"]) == 2
        assert "a count is expected" in capsys.readouterr().err
    for flag in ("--max-mismatch-permille", "--min-alt-permille"):
        drv.opt = drv.Opt()
        assert drv.main(base + ["--pileup", flag, "1001"]) == 2
        assert "shares of 1000" in capsys.readouterr().err
    drv.opt = drv.Opt()
    assert not os.path.exists(tmp_path / "out")
    drv.parse_opt(base[1:] + ["--pileup", "--min-depth", "4", "--min-overlap", "30"])
    drv.check_opt()
    assert drv.opt.pileup and drv.opt.pileup_opts == {"--min-depth": 4, "--min-overlap": 30}
    drv.opt = drv.Opt()
    for flag in ("--pileup", "--min-anchors", "--min-alt-permille"):
        assert flag in drv.USAGE


def test_header_declares_the_entry_and_the_structures_match():
    hdr = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    assert re.search(r"int mgta_reads_pileup\(mgta_sdbg \*, const mgta_reads \*reads, int reads_reversed, uint64_t n_short_reads", hdr)
    assert re.search(r"int mgta_ctx_set_pileup_chunk\(mgta_ctx \*, uint32_t reads\);", hdr)
    assert "typedef struct mgta_pileup_params { int32_t min_anchors, min_overlap, max_mismatch_permille; } mgta_pileup_params;" in hdr
    assert "mgta_reads_pileup" in _lib.SYMBOLS and "mgta_ctx_set_pileup_chunk" in _lib.SYMBOLS and len(_lib.SYMBOLS["mgta_reads_pileup"][1]) == 13
    assert pl.CONTIG_DTYPE.itemsize == 48 and pl.READ_DTYPE.itemsize == 24
    fields = H.header_fields("mgta_pileup_stats", hdr)
    assert fields == [n for n, _ in _lib.PileupStats._fields_]
