"""CPU-only: the yardstick of the recruit tests (tests/recruit_ref.py) on hand-written reads whose answer is worked out here, its numpy
form against its scalar loops, the writers and readers of the four recruit files (megagta_amd/recruit.py), the assembled fraction, the
usage errors of `megagta recruit` and of the driver's --recruit options, and the header's declaration of the entry."""
import ctypes
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest

from megagta_amd import _lib
from megagta_amd import hmm as H
from megagta_amd import readlib, synth
from megagta_amd import recruit as rc
from tests import helpers
from tests import recruit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
NEG = float("-inf")


def tiny_model():
    """two columns over the letters K and N: column 1 likes K (2) and dislikes N (-1), column 2 the other way round (-1, 3); the only
    finite transition is match -> match out of column 1 (-0.5)"""
    alpha = np.full(128, -1, dtype=np.int32)
    alpha[ord("K")] = alpha[ord("k")] = 0
    alpha[ord("N")] = alpha[ord("n")] = 1
    msc = np.array([[0.0, 0.0], [2.0, -1.0], [-1.0, 3.0]])
    tsc = np.full((7, 3), NEG)
    tsc[ref.MM, 1] = -0.5
    return types.SimpleNamespace(M=2, A=2, msc=msc, tsc=tsc, alpha=alpha)


def test_translation_stretch_and_frames_by_hand():
    # AAAAAC: frame 0 = AAA AAC = K N, frame 1 = AAA (AC left over) = K, frame 2 = AAA (C left over) = K;
    # its reverse complement GTTTTT: frame 3 = GTT TTT = V F, frame 4 = TTT (TT left over) = F, frame 5 = TTT = F
    assert ref.frames(ref.codes_of("AAAAAC")) == ["KN", "K", "K", "VF", "F", "F"]
    assert ref.frames(ref.codes_of("")) == [""] * 6 and ref.frames(ref.codes_of("AC")) == [""] * 6
    assert ref.frames(ref.codes_of("ACG")) == ["T", "", "", "R", "", ""]            # ACG = T; CGT = R
    # TAA TAA: a stop in every codon of frame 0; frame 1 = AAT (AA) = N, frame 2 = ATA (A) = I; TTATTA: frame 3 = L L, 4 = Y (TA), 5 = I (A)
    assert ref.frames(ref.codes_of("TAATAA")) == ["**", "N", "I", "LL", "Y", "I"]
    assert ref.stretch("**") == (0, 0) and ref.stretch("") == (0, 0)
    assert ref.stretch("*KN") == (1, 2) and ref.stretch("KN*") == (0, 2)
    assert ref.stretch("KN*NK") == (0, 2)                                           # two equally long runs: the first
    assert ref.stretch("K*NKK*KKK*") == (2, 3) and ref.stretch("K*NK*KKK*") == (5, 3) and ref.stretch("KKK*KK") == (0, 3)


def test_score_and_best_frame_by_hand():
    hm = tiny_model()
    # "KN": VM[1][1] = 0 + 2, VM[1][2] = 0 - 1; VM[2][2] = (VM[1][1] - 0.5) + 3 = 4.5, VM[2][1] = -inf: score 4.5, columns 1 .. 2
    assert ref.score_carry(hm, "KN") == (4.5, 1, 2)
    # "K": VM[1][1] = 2, VM[1][2] = -1: column 1 alone.  "N": VM[1][1] = -1, VM[1][2] = 3: column 2 alone
    assert ref.score_carry(hm, "K") == (2.0, 1, 1) and ref.score_carry(hm, "N") == (3.0, 2, 2)
    # "VF" emits 0 everywhere: VM[2][2] = 0 - 0.5 + 0.  "F": both columns reach 0, the lower one wins.  Three residues fit no path
    assert ref.score_carry(hm, "VF") == (-0.5, 1, 2) and ref.score_carry(hm, "F") == (0.0, 1, 1)
    assert ref.score_carry(hm, "KNK") == (NEG, 0, 0) and ref.score_carry(hm, "") == (NEG, 0, 0)
    # the read AAAAAC with min_aa = 1: frames score 4.5, 2, 2, -0.5, 0, 0: frame 0 wins
    out = ref.recruit(hm, [ref.codes_of("AAAAAC")], min_aa=1, min_score=4.5)
    assert out["recs"] == [dict(status=0, score=4.5, frame=0, aa_from=0, aa_len=2, model_from=1, model_to=2)]
    assert out["bits"].tolist() == [True] and out["col_depth"].tolist() == [1, 1]   # the threshold is inclusive
    assert out["stats"] == dict(n_reads=1, n_frames_scored=6, n_cells=(2 + 1 + 1 + 2 + 1 + 1) * 2, n_unaligned=0, n_unscored=0, n_recruited=1,
                                n_recruited_frame=[1, 0, 0, 0, 0, 0])
    assert ref.recruit(hm, [ref.codes_of("AAAAAC")], min_aa=1, min_score=np.nextafter(4.5, 5.0))["bits"].tolist() == [False]
    # min_aa = 2: frames 0 and 3 alone are scored.  min_aa = 3: none is, the read is unscored
    two = ref.recruit(hm, [ref.codes_of("AAAAAC")], min_aa=2, min_score=NEG)
    assert [s[:4] for s in two["stretches"]] == [(0, 0, 0, 2), (0, 3, 0, 2)] and two["recs"][0]["frame"] == 0
    none = ref.recruit(hm, [ref.codes_of("AAAAAC")], min_aa=3, min_score=NEG)
    assert none["recs"] == [dict(status=2, score=NEG, frame=0, aa_from=0, aa_len=0, model_from=0, model_to=0)] and none["bits"].tolist() == [False]
    # AAAAACAAA: frame 0 = K N K and frame 3 (TTTGTTTTT) = F V F have three residues, which no path over two columns without an
    # insert takes; the other frames (KT, KQ, LF, CF) have two and are not scored at min_aa = 3
    una = ref.recruit(hm, [ref.codes_of("AAAAACAAA")], min_aa=3, min_score=NEG)
    assert [s[1] for s in una["stretches"]] == [0, 3]
    assert una["recs"] == [dict(status=1, score=NEG, frame=0, aa_from=0, aa_len=3, model_from=0, model_to=0)]
    assert una["bits"].tolist() == [False] and una["stats"]["n_unaligned"] == 1      # not recruited even at -inf
    # AAATTT is its own reverse complement: frames 3 .. 5 repeat 0 .. 2 (KF, N, I).  N scores 3 in column 2, in frame 1 and again in
    # frame 4: the lower frame keeps the record
    pal = ref.recruit(hm, [ref.codes_of("AAATTT")], min_aa=1, min_score=NEG)
    assert ref.frames(ref.codes_of("AAATTT")) == ["KF", "N", "I"] * 2
    assert pal["recs"] == [dict(status=0, score=3.0, frame=1, aa_from=0, aa_len=1, model_from=2, model_to=2)]


def test_numpy_form_is_the_scalar_loops(tmp_path):
    rng = np.random.default_rng(3)
    prot = "".join(synth.AA_ORDER[c] for c in rng.integers(0, 20, 23))
    (tmp_path / "p.hmm").write_text(synth.hmm_text("p", prot))
    hm = H.parse_hmm(str(tmp_path / "p.hmm"))
    for L in (1, 2, 7, 23, 30):
        seqs = [prot[a:a + L] if a + L <= 23 else "".join(synth.AA_ORDER[c] for c in rng.integers(0, 20, L)) for a in (0, 3, 11, 40)]
        seqs.append("".join(synth.AA_ORDER[c] for c in rng.integers(0, 20, L)))
        fast = ref.score_carry_equal(hm, seqs)
        for s, got in zip(seqs, fast):
            want = ref.score_carry(hm, s)
            assert struct.pack("<d", got[0]) == struct.pack("<d", want[0]) and got[1:] == want[1:], (L, s)
    tiny = tiny_model()
    assert ref.score_carry_equal(tiny, ["KN", "VF", "NK"]) == [ref.score_carry(tiny, s) for s in ("KN", "VF", "NK")]
    assert ref.score_all(tiny, ["KN", "K", "KNK", "N", ""]) == [ref.score_carry(tiny, s) for s in ("KN", "K", "KNK", "N", "")]


def fixed_result():
    """what Context.recruit would return for five reads of which 1 and 3 are recruited"""
    recs = np.zeros(5, dtype=rc.REC)
    recs[1] = (20.0 * rc.LN2, 3, 9, 2, 21, 4, 0, (0, 0))
    recs[3] = (33.5, 1, 4, 0, 50, 0, 0, (0, 0))
    recs[0]["status"], recs[2]["status"] = 2, 1
    recs[0]["score"] = recs[2]["score"] = recs[4]["score"] = NEG
    stats = dict(n_reads=5, n_frames_scored=11, n_cells=990, n_unaligned=1, n_unscored=1, n_recruited=2, n_recruited_frame=[1, 0, 0, 0, 1, 0])
    return dict(hit_bits=np.array([0b01010], dtype=np.uint64), recs=recs, col_depth=np.array([1, 1, 2, 2, 1, 1, 1, 1, 1, 0], dtype=np.uint64), stats=stats)


def test_the_four_files_and_the_round_trip(tmp_path):
    res = fixed_result()
    reads = [ref.codes_of(s) for s in ("ACGT", "AACCGGTTA", "T", "GATTACA", "CC")]
    packed, start = readlib.pack_for_build(reads)
    assert rc.hit_indices(res["hit_bits"], 5).tolist() == [1, 3] and rc.lib_counts(res["hit_bits"], [2, 2, 5]) == [1, 0, 1]
    paths = rc.write_files(str(tmp_path), res, packed, start, lib_end=[2, 5], matched=[0, 3, 4])
    assert sorted(os.path.basename(p) for p in paths.values()) == ["recruit.txt", "recruit_cols.txt", "recruit_reads.fa", "recruit_summary.txt"]
    assert open(paths["recruit_reads.fa"]).read() == ">r1\nAACCGGTTA\n>r3\nGATTACA\n"
    assert open(paths["recruit.txt"]).read() == ("#read\tframe\taa_from\taa_len\tbits\tmodel_from\tmodel_to\n"
                                                "1\t4\t2\t21\t20.0000\t3\t9\n"
                                                "3\t0\t0\t50\t%.4f\t1\t4\n" % (33.5 / np.log(2.0)))
    assert open(paths["recruit_cols.txt"]).read() == "#column\tdepth\n" + "".join("%d\t%d\n" % (j + 1, d) for j, d in enumerate([1, 1, 2, 2, 1, 1, 1, 1, 1, 0]))
    assert open(paths["recruit_summary.txt"]).read() == ("reads_scanned\t5\nreads_scored\t4\nreads_recruited\t2\nrecruited_frame0\t1\nrecruited_frame1\t0\n"
                                                        "recruited_frame2\t0\nrecruited_frame3\t0\nrecruited_frame4\t1\nrecruited_frame5\t0\n"
                                                        "recruited_lib0\t1\nrecruited_lib1\t1\nrecruited_and_matched\t1\nassembled_fraction\t0.5000\n")
    back = rc.read_files(str(tmp_path))
    assert back["reads"].tolist() == [1, 3] and back["seqs"] == ["AACCGGTTA", "GATTACA"]
    assert back["recs"] == [dict(read=1, frame=4, aa_from=2, aa_len=21, bits=20.0, model_from=3, model_to=9),
                            dict(read=3, frame=0, aa_from=0, aa_len=50, bits=round(33.5 / np.log(2.0), 4), model_from=1, model_to=4)]
    assert back["col_depth"].tolist() == res["col_depth"].tolist()
    assert back["summary"]["reads_recruited"] == 2 and back["summary"]["assembled_fraction"] == 0.5 and back["summary"]["recruited_lib1"] == 1
    # without libraries and without the matched reads those lines are not written
    assert "lib" not in rc.summary_text(res["stats"]) and "assembled" not in rc.summary_text(res["stats"])
    for bad in ("", "#read\tframe\n", rc.HEADER + "\n1\t2\n"):
        with pytest.raises(ValueError):
            rc.parse_recruit(bad)
    with pytest.raises(ValueError):
        rc.parse_cols(rc.COLS_HEADER + "\n2\t1\n")


def test_assembled_fraction_from_two_index_sets(tmp_path):
    assert rc.assembled_fraction([1, 3, 5, 7], [0, 3, 7, 9]) == (2, 0.5)
    assert rc.assembled_fraction([], [1, 2]) == (0, 0.0) and rc.assembled_fraction([4], []) == (0, 0.0)
    assert rc.assembled_fraction([2, 4, 6], [6, 4, 2, 0]) == (3, 1.0)
    assert rc.assembled_fraction([5, 1, 9], [9])[1] == 1 / 3
    # the driver's join: the two lines go behind the summary of `megagta recruit`, once however often it runs
    (tmp_path / "s.txt").write_text("reads_scanned\t9\nreads_scored\t8\nreads_recruited\t3\n")
    (tmp_path / "r.fa").write_text(">r1\nAC\n>r5\nGG\n>r9\nT\n")
    (tmp_path / "m.fa").write_text(">r0\nA\n>r9\nT\n")
    for _ in range(2):
        assert rc.append_assembled(str(tmp_path / "s.txt"), str(tmp_path / "r.fa"), str(tmp_path / "m.fa")) == (1, 1 / 3)
        assert (tmp_path / "s.txt").read_text() == "reads_scanned\t9\nreads_scored\t8\nreads_recruited\t3\nrecruited_and_matched\t1\nassembled_fraction\t0.3333\n"


def test_cli_usage_errors():
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    usage = "Usage: megagta recruit <model.hmm> <read.lib> <out_prefix> [--min-bits B] [--min-aa N]"
    for args, says in ((["recruit"], usage), (["recruit", "m.hmm", "lib"], usage), (["recruit", "m.hmm", "lib", "out", "--min-bits"], usage),
                       (["recruit", "m.hmm", "lib", "out", "--nonsense", "1"], usage), (["recruit", "m.hmm", "lib", "out", "--min-aa", "0"], "--min-aa 0 is not a count"),
                       (["recruit", "m.hmm", "lib", "out", "--min-aa", "x"], "--min-aa x is not a count"),
                       (["recruit", "m.hmm", "lib", "out", "--min-bits", "nan"], "--min-bits nan is not a number"),
                       (["recruit", "m.hmm", "lib", "out", "--min-bits", "2x"], "--min-bits 2x is not a number")):
        r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and says in r.stderr and usage in r.stderr, (args, r.stderr)


def test_driver_usage_errors(tmp_path, capsys):
    from megagta_amd import megagta as drv
    reads = tmp_path / "r.fa"
    reads.write_text(">r\nACGT\n")
    base = ["megagta.py", "-r", str(reads), "-g", str(tmp_path / "genes.txt"), "-o", str(tmp_path / "out")]
    try:
        for flag, val in (("--recruit-bits", "20"), ("--recruit-min-aa", "20")):
            drv.opt = drv.Opt()
            assert drv.main(base + [flag, val]) == 2
            assert flag + " needs --recruit" in capsys.readouterr().err
        for flag, val, says in (("--recruit-bits", "many", "a number of bits is expected"), ("--recruit-bits", "nan", "a number of bits is expected"),
                                ("--recruit-min-aa", "0", "a count of 1 .. 4096 residues is expected"), ("--recruit-min-aa", "-4", "a count of 1 .. 4096")):
            drv.opt = drv.Opt()
            assert drv.main(base + ["--recruit", flag, val]) == 2
            assert says in capsys.readouterr().err
        drv.opt = drv.Opt()
        drv.parse_opt(base[1:] + ["--recruit", "--recruit-bits", "-3.5", "--recruit-min-aa", "12"])
        assert drv.opt.recruit and drv.opt.recruit_opts == {"--recruit-bits": "-3.5", "--recruit-min-aa": "12"}
        assert not os.path.exists(tmp_path / "out")
    finally:
        drv.opt = drv.Opt()
    for flag in ("--recruit", "--recruit-bits", "--recruit-min-aa"):
        assert flag in drv.USAGE


def test_header_declares_the_entry_and_the_structures_match():
    hdr = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    assert re.search(r"int mgta_reads_recruit\(mgta_ctx \*, const mgta_hmm \*, const mgta_reads \*, int reads_reversed, uint64_t n_short_reads,", hdr)
    assert re.search(r"int mgta_ctx_set_recruit_chunk\(mgta_ctx \*, uint32_t reads\);", hdr)
    assert ("typedef struct mgta_recruit_rec { double score; int32_t model_from, model_to; uint16_t aa_from, aa_len; uint8_t frame, status; uint8_t pad[2]; } "
            "mgta_recruit_rec;") in hdr
    assert "mgta_reads_recruit" in _lib.SYMBOLS and "mgta_ctx_set_recruit_chunk" in _lib.SYMBOLS and len(_lib.SYMBOLS["mgta_reads_recruit"][1]) == 10
    assert rc.REC.itemsize == ctypes.sizeof(_lib.RecruitRec) == 24 and ctypes.sizeof(_lib.RecruitParams) == 16
    assert [rc.REC.fields[n][1] for n in ("score", "model_from", "model_to", "aa_from", "aa_len", "frame", "status")] == [0, 8, 12, 16, 18, 20, 21]
    fields = helpers.header_fields("mgta_recruit_stats", hdr)
    assert fields == [n for n, _ in _lib.RecruitStats._fields_]
    assert os.path.exists(_lib.LIB_PATH), "libmegagta_hip.so missing: run __graft_entry__.build()"
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "mgta_reads_recruit") and hasattr(L, "mgta_ctx_set_recruit_chunk")
    # the guards that need no device: a NULL context is refused before anything else is looked at
    L.mgta_reads_recruit.restype, L.mgta_reads_recruit.argtypes = _lib.SYMBOLS["mgta_reads_recruit"]
    L.mgta_ctx_set_recruit_chunk.restype, L.mgta_ctx_set_recruit_chunk.argtypes = _lib.SYMBOLS["mgta_ctx_set_recruit_chunk"]
    L.mgta_last_error.restype = ctypes.c_char_p
    assert L.mgta_reads_recruit(None, None, None, 1, 0, None, None, None, None, None) == -1 and b"ctx" in L.mgta_last_error()
    assert L.mgta_ctx_set_recruit_chunk(None, 4) == -1 and b"ctx" in L.mgta_last_error()
