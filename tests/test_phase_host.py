"""CPU-only: mgta_phase_pairs (host-only entry) against a Python two-pointer and its EINVAL cases; the link rule, the block rule and the
writers and readers of the phase files (megagta_amd/phase.py) on hand-written tables; the header's declarations; the driver's usage
errors around --phase."""
import os
import re

import numpy as np
import pytest

from megagta_amd import _lib
from megagta_amd import phase as ph
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pairs_by_two_pointer(sites, max_span):
    span = max_span or 1000
    per_site = []
    for pos in sites:
        v = 0
        for u in range(len(pos)):
            v = max(v, u + 1)
            while v < len(pos) and pos[v] - pos[u] < span:
                v += 1
            per_site.append(v - u - 1)
    return [0] + np.cumsum(per_site, dtype=np.int64).tolist() if per_site else [0]


def raw_pairs(site_off, site_pos, n, max_span, fill=7):
    L = _lib.load()
    off = np.asarray(site_off, dtype=np.uint64)
    pos = np.asarray(site_pos, dtype=np.uint32)
    out = np.full(len(site_pos) + 1, fill, dtype=np.uint64)
    code = L.mgta_phase_pairs(off.ctypes.data, pos.ctypes.data if pos.size else None, n, max_span, out.ctypes.data)
    return code, L.mgta_last_error(), out


def test_phase_pairs_equals_the_two_pointer():
    from megagta_amd import api
    rng = np.random.default_rng(5)
    sites = [[0, 10, 59, 60, 61, 200, 1199, 1200, 1300],        # 10 -> 59 is 49 apart, 10 -> 60 is 50; 200 -> 1199 is 999, 200 -> 1200 is 1000
             [5],                                                # one site
             [],                                                 # none
             sorted(set(int(x) for x in rng.integers(0, 5000, 300))),
             list(range(100, 180))]                              # adjacent positions
    pairs = api.Context.phase_pairs                              # (a static method: the entry is host-only and needs no context)
    for span in (50, 0, 1000, 1, 2, 7, 100000):
        got = pairs(sites, span).tolist()
        assert got == pairs_by_two_pointer(sites, span), span
    at50 = pairs(sites, 50)
    assert int(at50[2] - at50[1]) == 1 and int(at50[3] - at50[2]) == 2      # site 10: 59 only; site 59: 60 and 61
    at0 = pairs(sites, 0)
    assert int(at0[6] - at0[5]) == 1 and at0.tolist() == pairs(sites, 1000).tolist()   # site 200: 1199 (999 apart), not 1200
    assert pairs(sites, 1).tolist() == [0] * (sum(map(len, sites)) + 1)                 # a span of 1 tables nothing
    assert pairs([], 0).tolist() == [0] and pairs([[], []], 9).tolist() == [0]
    # the index of a pair: every tabled (u, v) has a slot of its own
    po = pairs(sites, 50)
    seen = set()
    base = 0
    for pos in sites:
        for u in range(len(pos)):
            for v in range(u + 1, len(pos)):
                if pos[v] - pos[u] < 50:
                    seen.add(int(po[base + u]) + v - u - 1)
        base += len(pos)
    assert seen == set(range(int(po[-1])))


def test_phase_pairs_einval():
    for off, pos, n, span, word in (([0, 3], [4, 4, 9], 1, 0, b"ascend"), ([0, 3], [4, 3, 9], 1, 0, b"ascend"), ([0, 1, 3], [9, 5, 5], 2, 0, b"ascend"),
                                    ([1, 3], [1, 2, 3], 1, 0, b"site_off[0]"), ([0, 2, 1], [1, 2], 2, 0, b"site_off must ascend"),
                                    ([0, 2], [1, 2], 1, -1, b"max_span"), ([0], [], -1, 0, b"contig count")):
        code, msg, out = raw_pairs(off, pos, n, span)
        assert code == -1 and word in msg, (off, pos, msg)
        assert (out == 7).all()                                               # nothing written
    L = _lib.load()
    assert L.mgta_phase_pairs(None, None, 0, 0, np.zeros(1, dtype=np.uint64).ctypes.data) == -1
    assert L.mgta_phase_pairs(np.zeros(1, dtype=np.uint64).ctypes.data, None, 0, 0, None) == -1
    code, msg, out = raw_pairs([0, 2, 3], [9, 5 + 9, 5], 2, 0)               # a new contig may start below the last position of the one before
    assert code == 0 and out.tolist() == [0, 1, 1, 1]


def cells(**kw):
    c = np.zeros(16, dtype=np.uint32)
    for h, n in kw.items():
        c["ACGT".index(h[0]) * 4 + "ACGT".index(h[1])] = n
    return c


def table():
    """two contigs: c1 with the sites a b c d at 9, 19, 29, 39 (0-based), all six pairs tabled; c2 with two sites, one pair"""
    site_off = np.array([0, 4, 6], dtype=np.int64)
    site_pos = np.array([9, 19, 29, 39, 0, 5], dtype=np.uint32)
    pair_off = np.array([0, 3, 5, 6, 6, 7, 7], dtype=np.uint64)
    joint = np.stack([cells(AC=12, GT=9, AT=2),        # a-b: AT is 2 of 23 = 86 permille, below 100: phased
                      cells(AC=6, AT=5),                # a-c: AC, AT share the A: not phased
                      cells(AA=3),                      # a-d: below min_link 4
                      cells(CC=5, TG=5),                # b-c: phased (the tie is ordered by the letters)
                      cells(CA=4),                      # b-d: one cell: not phased
                      np.zeros(16, dtype=np.uint32),    # c-d: no fragment
                      cells(GG=2, TT=2, GT=1)])         # c2: GT is 200 permille and shares G and T: not phased
    return dict(site_off=site_off, site_pos=site_pos, pair_off=pair_off, joint=joint)


def test_the_link_rule():
    assert not ph.is_phased(cells(AC=6, AT=5))
    assert ph.is_phased(cells(AC=12, GT=9, AT=2)) and not ph.is_phased(cells(AC=12, GT=9, AT=2), min_hap_permille=80)
    assert ph.is_phased(cells(AC=90, GT=10)) and not ph.is_phased(cells(AC=91, GT=9))        # 100 permille exactly counts, 90 does not
    assert not ph.is_phased(cells(AC=7)) and not ph.is_phased(cells())
    assert not ph.is_phased(cells(AC=5, GC=5)) and ph.is_phased(cells(AC=5, GT=5, TA=5))      # the letter at pos2 shared; three haplotypes
    assert ph.haplotype_cells(cells(CC=5, TG=5, AA=7, AC=1)) == [("AA", 7), ("CC", 5), ("TG", 5), ("AC", 1)]
    rows = ph.links(table())
    assert [(int(r["contig"]), int(r["u"]), int(r["v"]), int(r["fragments"]), int(r["phased"])) for r in rows] == \
        [(0, 0, 1, 23, 1), (0, 0, 2, 11, 0), (0, 1, 2, 10, 1), (0, 1, 3, 4, 0), (1, 4, 5, 5, 0)]
    assert len(ph.links(table(), min_link=1)) == 6 and len(ph.links(table(), min_link=0)) == 6        # a pair without a fragment is never listed
    assert [int(r["fragments"]) for r in ph.links(table(), min_link=11)] == [23, 11]


def test_the_two_files_and_the_round_trip(tmp_path):
    res = table()
    t = ph.format_phase(["c1", "c2"], res)
    assert t["links"] == ("#contig\tpos1\tpos2\tfragments\thaplotypes\tphased\n"
                          "c1\t10\t20\t23\tAC:12,GT:9,AT:2\t1\n"
                          "c1\t10\t30\t11\tAC:6,AT:5\t0\n"
                          "c1\t20\t30\t10\tCC:5,TG:5\t1\n"
                          "c1\t20\t40\t4\tCA:4\t0\n"
                          "c2\t1\t6\t5\tGG:2,TT:2,GT:1\t0\n")
    # a-b and b-c phased, a-c not: one block of three
    assert t["blocks"] == "#contig\tblock\tsites\tfirst\tlast\tpositions\nc1\t1\t3\t10\t30\t10,20,30\n"
    # with GT of c2 below the permille both contigs have a block, each numbered from 1
    t2 = ph.format_phase(["c1", "c2"], res, min_link=1, min_hap_permille=250)
    assert t2["blocks"].splitlines()[1:] == ["c1\t1\t3\t10\t30\t10,20,30", "c2\t1\t2\t1\t6\t1,6"]
    res3 = table()
    res3["joint"][3] = cells(CC=5, CG=5)
    res3["joint"][5] = cells(AA=2, CC=2)
    res3["joint"][0] = cells(AC=1)
    assert ph.format_phase(["c1", "c2"], res3)["blocks"].splitlines()[1:] == ["c1\t1\t2\t30\t40\t30,40"]   # only c-d is left phased
    res3["joint"][5] = cells(AA=3, CC=2)
    res3["joint"][2] = cells(AC=3, CA=3)
    assert ph.format_phase(["c1", "c2"], res3)["blocks"].splitlines()[1:] == ["c1\t1\t3\t10\t40\t10,30,40"]  # a-d and c-d: a block that skips b
    res3["joint"][2] = cells(AA=9)
    res3["joint"][0] = cells(AC=4, CA=4)
    assert ph.format_phase(["c1", "c2"], res3)["blocks"].splitlines()[1:] == ["c1\t1\t2\t10\t20\t10,20", "c1\t2\t2\t30\t40\t30,40"]   # two blocks of one contig
    paths = ph.write_phase(str(tmp_path / "g"), ["c1", "c2"], res)
    assert [os.path.basename(p) for p in paths] == ["g_phase_links.txt", "g_phase_blocks.txt"]
    assert [open(p).read() for p in paths] == [t["links"], t["blocks"]]
    rows = ph.parse_links(open(paths[0]).read())
    assert [(r["contig"], r["pos1"], r["pos2"], r["fragments"], r["phased"]) for r in rows] == \
        [("c1", 10, 20, 23, 1), ("c1", 10, 30, 11, 0), ("c1", 20, 30, 10, 1), ("c1", 20, 40, 4, 0), ("c2", 1, 6, 5, 0)]
    assert rows[0]["haplotypes"] == [("AC", 12), ("GT", 9), ("AT", 2)]
    assert ph.parse_blocks(open(paths[1]).read()) == [dict(contig="c1", block=1, sites=3, first=10, last=30, positions=[10, 20, 30])]
    with pytest.raises(ValueError, match="header"):
        ph.parse_links(t["blocks"])
    with pytest.raises(ValueError, match="header"):
        ph.parse_blocks(t["links"])
    with pytest.raises(ValueError, match="sum of the haplotypes"):
        ph.parse_links(ph.LINKS_HEADER + "c\t1\t2\t5\tAC:4\t0\n")
    with pytest.raises(ValueError, match="do not fit"):
        ph.parse_blocks(ph.BLOCKS_HEADER + "c\t1\t3\t1\t9\t1,9\n")
    with pytest.raises(ValueError, match="differ in number"):
        ph.format_phase(["c1"], res)


def test_sites_from_pileup_applies_the_variant_rule():
    counts = np.array([[10, 0, 0, 0], [1, 8, 0, 0], [0, 0, 7, 7], [1, 0, 0, 6], [0, 3, 3, 3], [0, 0, 0, 0], [1, 0, 0, 19]], dtype=np.uint32)
    res = dict(counts=counts, offsets=np.array([0, 5, 5, 7], dtype=np.int64))
    seqs = ["ACgTN", "", "TT"]
    assert [s.tolist() for s in ph.sites_from_pileup(seqs, res)] == [[1, 2, 4], [], []]
    assert [s.tolist() for s in ph.sites_from_pileup(seqs, res, min_depth=7, min_alt_permille=50)] == [[1, 2, 3, 4], [], [1]]


def test_header_declares_the_entries_and_the_structures_match():
    hdr = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    assert re.search(r"int mgta_phase_pairs\(const uint64_t \*site_off[^;]*const uint32_t \*site_pos[^;]*int64_t n, int32_t max_span,\s*uint64_t \*pair_off[^;]*\);", hdr)
    assert re.search(r"int mgta_reads_phase\(const mgta_reads \*reads, int reads_reversed, const mgta_read_place \*place", hdr)
    assert re.search(r"int mgta_ctx_set_phase_chunk\(mgta_ctx \*, uint32_t slots\);", hdr)
    assert "typedef struct mgta_phase_params { int32_t max_span; } mgta_phase_params;" in hdr
    for name, n_args in (("mgta_phase_pairs", 5), ("mgta_reads_phase", 16), ("mgta_ctx_set_phase_chunk", 2)):
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == n_args, name
        assert hasattr(_lib.load(), name)
    fields = H.header_fields("mgta_phase_stats", hdr)
    assert fields == [n for n, _ in _lib.PhaseStats._fields_]
    assert "PREFIX_phase_links.txt" in ph.__doc__ and ph.LINK_DTYPE.names == ("contig", "u", "v", "fragments", "phased")


def test_driver_usage_errors_of_phase(tmp_path, capsys):
    from megagta_amd import megagta as drv
    (tmp_path / "reads.fa").write_text(">r\nACGT\n")
    (tmp_path / "genes.txt").write_text("")
    base = ["megagta.py", "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "genes.txt"), "-o", str(tmp_path / "out")]
    drv.opt = drv.Opt()
    assert drv.main(base + ["--phase"]) == 2
    assert "--phase needs --pileup: it is an option of that step" in capsys.readouterr().err
    for flag in ("--max-span", "--min-link", "--min-hap-permille"):
        drv.opt = drv.Opt()
        assert drv.main(base + ["--pileup", flag, "3"]) == 2
        assert flag + " needs --phase" in capsys.readouterr().err
        drv.opt = drv.Opt()
        assert drv.main(base + ["--pileup", "--phase", flag, "-3"]) == 2
        assert "a count is expected" in capsys.readouterr().err
    drv.opt = drv.Opt()
    assert drv.main(base + ["--pileup", "--phase", "--min-hap-permille", "1001"]) == 2
    assert "share of 1000" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "out")
    drv.opt = drv.Opt()
    drv.parse_opt(base[1:] + ["--pileup", "--phase", "--min-link", "2", "--max-span", "300", "--min-depth", "4"])
    drv.check_opt()
    assert drv.opt.phase and drv.opt.phase_opts == {"--min-link": 2, "--max-span": 300} and drv.opt.pileup_opts == {"--min-depth": 4}
    drv.opt = drv.Opt()
    for flag in ("--phase", "--max-span", "--min-link", "--min-hap-permille"):
        assert flag in drv.USAGE
