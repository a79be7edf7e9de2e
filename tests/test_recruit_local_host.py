"""CPU-only: the yardstick of local read recruitment (tests/recruit_local_ref.py) against what defines it -- the maximum, over every
substring of a stretch, of the global rule (tests/recruit_ref.score_carry), and for the fields an enumeration of every path of every
substring under the tie order; the delete-after-entry case; its numpy form against its scalar loops; the `recruit_mode` line of the
summary file; the usage errors of `megagta recruit --local` and of the driver's --recruit-local; the header's `mode`."""
import ctypes
import os
import struct
import subprocess
import types

import numpy as np
import pytest

from megagta_amd import _lib
from megagta_amd import recruit as rc
from tests import helpers
from tests import recruit_local_ref as lref
from tests import recruit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
NEG = float("-inf")
LETTERS = "KNTR"


def eight(x):
    return struct.pack("<d", float(x))


def random_model(rng, M, stars=0.0, whole=False):
    """M columns over the letters K N T R (any other letter emits 0): tables at random, `stars` of their entries -inf; whole = small
    integers, so that sums are exact and ties are frequent"""
    alpha = np.full(128, -1, dtype=np.int32)
    for k, c in enumerate(LETTERS):
        alpha[ord(c)] = alpha[ord(c.lower())] = k
    if whole:
        msc = rng.integers(-2, 3, (M + 1, len(LETTERS))).astype(np.float64)
        tsc = rng.integers(-2, 1, (7, M + 1)).astype(np.float64)
    else:
        msc = rng.normal(0.0, 2.0, (M + 1, len(LETTERS)))
        tsc = -rng.exponential(1.0, (7, M + 1))
    msc[rng.random(msc.shape) < stars] = NEG
    tsc[rng.random(tsc.shape) < stars] = NEG
    msc[0] = 0.0
    return types.SimpleNamespace(M=M, A=len(LETTERS), msc=msc, tsc=tsc, alpha=alpha)


def random_seq(rng, n):
    return "".join("KNTRW"[c] for c in rng.integers(0, 5, n))             # W is not a letter of the model


def best_substring_score(hm, seq):
    return max(ref.score_carry(hm, seq[a:b])[0] for b in range(1, len(seq) + 1) for a in range(b))


def test_score_is_the_maximum_over_every_substring():
    rng = np.random.default_rng(101)
    n_inf = 0
    for M in range(1, 13):
        for stars in (0.0, 0.2):
            hm = random_model(rng, M, stars)
            seqs = [random_seq(rng, int(n)) for n in (1, 2, 3, 7, 16, 30)] + [random_seq(rng, int(rng.integers(1, 31))) for _ in range(3)]
            many = lref.sweep_many(hm, seqs)
            for s, m in zip(seqs, many):
                got = lref.sweep(hm, s)
                assert eight(got[0]) == eight(best_substring_score(hm, s)), (M, stars, s)
                assert got == m and eight(got[0]) == eight(m[0]), (M, stars, s)       # the numpy form is the scalar loops
                if got[0] > NEG:                                           # the span it reports, aligned globally, has that score and those columns
                    back = ref.score_carry(hm, s[got[3]:got[3] + got[4]])
                    assert eight(back[0]) == eight(got[0]) and 1 <= got[1] <= got[2] <= M and got[4] >= 1, (M, stars, s)
                n_inf += got[0] == NEG
    # a model whose every match emission is a star places nothing; the empty stretch neither
    dead = random_model(rng, 3)
    dead.msc[1:] = NEG
    assert lref.sweep(dead, "KNT") == lref.NONE and lref.sweep_many(dead, ["KNT", "K", "NN", "TT"]) == [lref.NONE] * 4 and lref.sweep(dead, "") == lref.NONE
    assert lref.sweep(dead, "WW")[0] == 0.0                                 # a letter outside the alphabet emits 0


# ---- every path of every substring -----------------------------------------------------------------------------------------------------
B_, M_, I_, D_ = 0, 1, 2, 3


def paths_of(hm, seq):
    """every path of mgta_seqs_align over `seq` as a protein -> [(score, end column, entry column, how every state was reached, last
    state first)]: a path starts in the match state of row 1 and any column (reached from B), ends in a match state of the last row,
    has no delete state in row 1 and no insert state in column M; (previous + transition) first, then + e"""
    M, L = hm.M, len(seq)
    msc, tsc, alpha = hm.msc.tolist(), hm.tsc.tolist(), hm.alpha.tolist()

    def e(j, i):
        a = alpha[ord(seq[i - 1])]
        return msc[j][a] if a >= 0 else 0.0

    out = []

    def walk(state, i, j, score, entry, how):
        if state == M_ and i == L:
            out.append((score, j, entry, tuple(reversed(how))))
        t_m, t_i, t_d = {M_: (ref.MM, ref.MI, ref.MD), I_: (ref.IM, ref.II, None), D_: (ref.DM, None, ref.DD)}[state]
        if i < L and j < M:
            walk(M_, i + 1, j + 1, (score + tsc[t_m][j]) + e(j + 1, i + 1), entry, how + [state])
        if t_i is not None and i < L and j < M:
            walk(I_, i + 1, j, score + tsc[t_i][j], entry, how + [state])
        if t_d is not None and i > 1 and j < M:
            walk(D_, i, j + 1, score + tsc[t_d][j], entry, how + [state])

    for j in range(1, M + 1):
        walk(M_, 1, j, 0.0 + e(j, 1), j, [B_])
    return out


def best_path(hm, seq):
    """the winner among the paths of all substrings: the highest score, the lowest end column, the lowest end row, then at every state
    from the end backwards the candidate written first (B, M, I, D) -> (score, model_from, model_to, first, length)"""
    best, key = lref.NONE, None
    for b in range(1, len(seq) + 1):
        for a in range(b):
            for score, j_end, entry, how in paths_of(hm, seq[a:b]):
                if score == NEG:
                    continue
                k = (-score, j_end, b, how)
                if key is None or k < key:
                    best, key = (score, entry, j_end, a, b - a), k
    return best


def test_every_field_against_all_paths_of_all_substrings():
    rng = np.random.default_rng(102)
    n_ties = 0
    for M in (1, 2, 3, 4):
        for whole in (False, True):
            for stars in (0.0, 0.25):
                for _ in range(6):
                    hm = random_model(rng, M, stars, whole)
                    for L in (1, 2, 3, 4, 5):
                        s = "".join(LETTERS[c] for c in rng.integers(0, 3, L))
                        want = best_path(hm, s)
                        got = lref.sweep(hm, s)
                        assert got == want and eight(got[0]) == eight(want[0]), (M, whole, stars, s, hm.msc.tolist(), hm.tsc.tolist())
                        if whole and want[0] > NEG:
                            top = [p for b in range(1, L + 1) for a in range(b) for p in paths_of(hm, s[a:b]) if p[0] == want[0]]
                            n_ties += len(top) > 1
    assert n_ties > 50                                                      # the whole-number tables did put the tie order to work


def test_ties_by_hand():
    # every match emission 1, every transition 0, two columns: "KK" reaches 2 only as M1 M2 over both residues; "K" reaches 1 in both
    # columns and takes the lower one
    hm = random_model(np.random.default_rng(1), 2)
    hm.msc[1:] = 1.0
    hm.tsc[:] = 0.0
    assert lref.sweep(hm, "K") == (1.0, 1, 1, 0, 1) and lref.sweep(hm, "KK") == (2.0, 1, 2, 0, 2)
    # three residues over two columns: M1 M2 at rows 1 - 2 and at rows 2 - 3 reach 2 in column 2 (M1 I1 M2 reaches 2 there too, in row 3):
    # the lowest row wins, the span is the first two residues
    assert lref.sweep(hm, "KKK") == (2.0, 1, 2, 0, 2)
    # a continuing candidate of exactly 0.0: column 1 emits 0 and MM = 0, so VM[2][2] could continue from (1, 1) with 0.0 or enter: B wins
    hm.msc[1] = 0.0
    assert lref.sweep(hm, "KK") == (1.0, 2, 2, 0, 1) and best_path(hm, "KK") == (1.0, 2, 2, 0, 1)
    hm.msc[1] = 0.5                                                         # a positive one continues: 0.5 + 0 + 1
    assert lref.sweep(hm, "KK") == (1.5, 1, 2, 0, 2)


def test_no_delete_straight_after_the_first_match():
    # columns 1 and 3 like K (5), column 2 likes nothing (-10), match <-> delete costs 0.1: over the two residues "KK" the path M1 D2 M3
    # would reach 5 - 0.1 - 0.1 + 5 = 9.8, but it deletes in the row of its first match, which mgta_seqs_align has no state for
    rng = np.random.default_rng(2)
    hm = random_model(rng, 3)
    hm.msc[1], hm.msc[2], hm.msc[3] = 5.0, -10.0, 5.0
    hm.tsc[:] = -20.0
    hm.tsc[ref.MD], hm.tsc[ref.DM] = -0.1, -0.1
    assert best_substring_score(hm, "KK") == 5.0 and ref.score_carry(hm, "KK")[0] < 0
    assert lref.sweep(hm, "KK") == (5.0, 1, 1, 0, 1) == best_path(hm, "KK") and lref.sweep_many(hm, ["KK"] * 4) == [(5.0, 1, 1, 0, 1)] * 4
    # with a third residue the delete state is legal in row 2: M1 (row 1) M2 (row 2) is poor, but M1, then row 2 = insert ... is not what wins:
    # the yardstick and the enumeration agree on whatever does
    assert lref.sweep(hm, "KKK") == best_path(hm, "KKK") and eight(lref.sweep(hm, "KKK")[0]) == eight(best_substring_score(hm, "KKK"))
    # a sweep that fed the delete state with B's value would report 9.8 here
    assert lref.sweep(hm, "KK")[0] != 9.8


def test_every_stretch_and_the_best_of_a_read():
    assert lref.all_stretches("KN*T**RKK*", 1) == [(0, 2), (3, 1), (6, 3)] and lref.all_stretches("KN*T**RKK*", 2) == [(0, 2), (6, 3)]
    assert lref.all_stretches("", 1) == [] and lref.all_stretches("***", 1) == [] and lref.all_stretches("KKK", 1) == [(0, 3)] and lref.all_stretches("KKK", 4) == []
    assert lref.all_stretches("K", 0) == [(0, 1)]
    hm = random_model(np.random.default_rng(3), 2)
    hm.msc[1], hm.msc[2] = [2.0, -1.0, -1.0, -1.0], [-1.0, 3.0, -1.0, -1.0]
    hm.tsc[:] = NEG
    hm.tsc[ref.MM, 1] = -0.5
    # AAA AAC TAA AAA AAC: frame 0 = K N * K N: two equal stretches, each 2 - 0.5 + 3 = 4.5 over columns 1 .. 2: the lower aa_from
    codes = ref.codes_of("AAAAACTAAAAAAAC")
    assert ref.frames(codes)[0] == "KN*KN"
    out = lref.recruit(hm, [codes], min_aa=2, min_score=4.5)
    assert [s[:4] for s in out["stretches"] if s[1] == 0] == [(0, 0, 0, 2), (0, 0, 3, 2)]
    assert out["recs"] == [dict(status=0, score=4.5, frame=0, aa_from=0, aa_len=2, model_from=1, model_to=2)] and out["bits"].tolist() == [True]
    assert out["stats"]["n_frames_scored"] == len(out["stretches"]) and out["stats"]["n_cells"] == sum(s[3] for s in out["stretches"]) * 2
    # the global rule scores one stretch of that frame; K N K in one stretch has no global path at all, and the local rule finds K N in it
    codes = ref.codes_of("AAAAACAAA")
    assert ref.recruit(hm, [codes], min_aa=3, min_score=NEG)["recs"][0]["status"] == 1
    loc = lref.recruit(hm, [codes], min_aa=3, min_score=NEG)
    assert loc["recs"] == [dict(status=0, score=4.5, frame=0, aa_from=0, aa_len=2, model_from=1, model_to=2)]
    # every emission a star: scored and unaligned, the record carries the whole first scored stretch
    hm.msc[1:] = NEG
    hm.alpha[:] = 0                                                         # (every letter of every frame)
    una = lref.recruit(hm, [ref.codes_of("TAAAAAAACTAA")], min_aa=2, min_score=NEG)
    assert una["recs"][0] == dict(status=1, score=NEG, frame=0, aa_from=1, aa_len=2, model_from=0, model_to=0) and not una["bits"].any()
    assert lref.recruit(hm, [ref.codes_of("AAAAAC")], min_aa=3)["recs"][0]["status"] == 2


# ---- files, flags, header --------------------------------------------------------------------------------------------------------------
def test_recruit_mode_line_through_writer_reader_and_join(tmp_path):
    stats = dict(n_reads=9, n_unscored=1, n_recruited=3, n_recruited_frame=[1, 0, 0, 2, 0, 0])
    plain, local = rc.summary_text(stats, [3]), rc.summary_text(stats, [3], local=True)
    assert "recruit_mode" not in plain and local == plain + "recruit_mode\tlocal\n"
    assert rc.parse_summary(local) == dict(rc.parse_summary(plain), recruit_mode="local")
    with_matched = rc.summary_text(stats, [3], [1, 5, 9], [0, 9], local=True)
    assert with_matched == local + "recruited_and_matched\t1\nassembled_fraction\t0.3333\n"
    # the driver's join keeps the line, however often it runs
    (tmp_path / "s.txt").write_text(local)
    (tmp_path / "r.fa").write_text(">r1\nAC\n>r5\nGG\n>r9\nT\n")
    (tmp_path / "m.fa").write_text(">r0\nA\n>r9\nT\n")
    for _ in range(2):
        rc.append_assembled(str(tmp_path / "s.txt"), str(tmp_path / "r.fa"), str(tmp_path / "m.fa"))
        assert (tmp_path / "s.txt").read_text() == with_matched
    assert rc.parse_summary((tmp_path / "s.txt").read_text())["recruit_mode"] == "local"
    # write_files passes it on; the other three files do not change
    from megagta_amd import readlib
    recs = np.zeros(2, dtype=rc.REC)
    recs[1] = (30.0, 2, 7, 4, 6, 1, 0, (0, 0))
    res = dict(hit_bits=np.array([0b10], dtype=np.uint64), recs=recs, col_depth=np.array([0, 1, 1], dtype=np.uint64),
               stats=dict(n_reads=2, n_unscored=1, n_recruited=1, n_recruited_frame=[0, 1, 0, 0, 0, 0]))
    packed, start = readlib.pack_for_build([ref.codes_of("ACGT"), ref.codes_of("GATTACA")])
    texts = {}
    for name, local_mode in (("g", False), ("l", True)):
        (tmp_path / name).mkdir()
        paths = rc.write_files(str(tmp_path / name), res, packed, start, local=local_mode)
        texts[name] = {os.path.basename(p): open(p).read() for p in paths.values()}
    assert texts["l"]["recruit_summary.txt"] == texts["g"]["recruit_summary.txt"] + "recruit_mode\tlocal\n"
    assert all(texts["l"][f] == texts["g"][f] for f in ("recruit_reads.fa", "recruit.txt", "recruit_cols.txt"))
    assert rc.read_files(str(tmp_path / "l"))["summary"]["recruit_mode"] == "local" and "recruit_mode" not in rc.read_files(str(tmp_path / "g"))["summary"]
    assert rc.read_files(str(tmp_path / "l"))["recs"] == [dict(read=1, frame=1, aa_from=4, aa_len=6, bits=round(30.0 / np.log(2.0), 4), model_from=2, model_to=7)]


def test_cli_local_flag_usage():
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    usage = "Usage: megagta recruit <model.hmm> <read.lib> <out_prefix> [--min-bits B] [--min-aa N] [--local]\n"
    for args, says in ((["recruit"], usage), (["recruit", "m.hmm", "lib", "out", "--local", "--nonsense", "1"], usage),
                       (["recruit", "m.hmm", "lib", "out", "--local", "1"], usage), (["recruit", "m.hmm", "lib", "out", "--locally"], usage),
                       # --local is taken, anywhere among the options: the error is the one of the option behind or before it
                       (["recruit", "m.hmm", "lib", "out", "--local", "--min-aa", "0"], "--min-aa 0 is not a count"),
                       (["recruit", "m.hmm", "lib", "out", "--min-bits", "2x", "--local"], "--min-bits 2x is not a number")):
        r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and says in r.stderr and usage in r.stderr, (args, r.stderr)


def test_driver_recruit_local_usage(tmp_path, capsys):
    from megagta_amd import megagta as drv
    reads = tmp_path / "r.fa"
    reads.write_text(">r\nACGT\n")
    base = ["megagta.py", "-r", str(reads), "-g", str(tmp_path / "genes.txt"), "-o", str(tmp_path / "out")]
    try:
        drv.opt = drv.Opt()
        assert drv.main(base + ["--recruit-local"]) == 2
        assert "--recruit-local needs --recruit" in capsys.readouterr().err
        drv.opt = drv.Opt()
        assert drv.main(base + ["--recruit", "--recruit-local=1"]) == 2        # it takes no value
        capsys.readouterr()
        drv.opt = drv.Opt()
        drv.parse_opt(base[1:] + ["--recruit", "--recruit-local", "--recruit-bits", "25"])
        assert drv.opt.recruit and drv.opt.recruit_opts == {"--recruit-local": "", "--recruit-bits": "25"}
        drv.opt = drv.Opt()
        drv.parse_opt(base[1:] + ["--recruit"])
        assert drv.opt.recruit and drv.opt.recruit_opts == {}
        assert not os.path.exists(tmp_path / "out")
    finally:
        drv.opt = drv.Opt()
    line = [ln for ln in drv.USAGE.splitlines() if ln.strip().startswith("--recruit-local")]
    assert len(line) == 1 and "needs --recruit" in line[0]
    assert "median 12.0 bits" in drv.USAGE and "17.6" in drv.USAGE           # the threshold sits close to noise in this mode, and the usage says so


def test_header_declares_mode():
    hdr = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    assert helpers.header_fields("mgta_recruit_params", hdr) == ["min_aa", "mode", "min_score"] == [n for n, _ in _lib.RecruitParams._fields_]
    assert "#define MGTA_RECRUIT_GLOBAL 0\n" in hdr and "#define MGTA_RECRUIT_LOCAL 1\n" in hdr
    assert ctypes.sizeof(_lib.RecruitParams) == 16 and _lib.RecruitParams.mode.offset == 4 and _lib.RecruitParams.min_score.offset == 8
    assert _lib.RecruitParams().mode == 0                                   # a caller that sets nothing asks for the global rule
    # no new entry point: the one call serves both modes, and the record and the stats keep their layouts
    assert len(_lib.SYMBOLS["mgta_reads_recruit"][1]) == 10 and rc.REC.itemsize == 24
    assert helpers.header_fields("mgta_recruit_stats", hdr) == [n for n, _ in _lib.RecruitStats._fields_]
    for text in ("MGTA_RECRUIT_LOCAL places reads locally", "WITHOUT its B candidate", "the lowest column", "ALIGNED SPAN", "median of 12.0", "17.6 bits"):
        assert text in hdr, text
