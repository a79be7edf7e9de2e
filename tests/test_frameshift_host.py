"""mgta_seqs_frameshift without a device: the Python restatement of the rule (tests/frameshift_ref.py) against an enumeration of every
state path, which pins the tie order before any kernel is compared with it; what a path makes of its contig (megagta_amd/frameshift.py)
and the round trip through PREFIX_frameshift.txt; the stand-alone check of csrc/frameshift_seq.hpp under the sanitizers; the refusals of
`megagta nearest --frameshift`."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from megagta_amd import frameshift as fsm
from tests import frameshift_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "megagta_amd", "csrc")
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")


# ---- the restatement against every path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("go,ge,fs,seed", [(2, 1, 1, 0), (1, 0, 0, 1), (3, 3, 2, 2)])
def test_restatement_is_the_best_of_every_path(go, ge, fs, seed):
    """all contigs of L <= 7 over {A, C} against all references of R <= 3 over {K, P}: score, end column and path are those of the
    best path written out and scored on its own, ties included"""
    sub = np.random.default_rng(seed).integers(-3, 4, (27, 27)).astype(np.int8)
    kinds, n_scored, n_none = set(), 0, 0
    for L in range(8):
        for x in map("".join, itertools.product("AC", repeat=L)):
            for R in range(4):
                for y in map("".join, itertools.product("KP", repeat=R)):
                    a, b = ref.pair(x, y, sub, go, ge, fs), ref.enumerate_best(x, y, sub, go, ge, fs)
                    if b is None:
                        assert a is None, (x, y, a)
                        n_none += 1
                        continue
                    assert a is not None and (a["score"], a["jend"], a["path"]) == b, (x, y, a, b)
                    assert fsm.corrected(x, a["path"])[0] is not None                        # the path consumes exactly the contig
                    kinds |= set(a["path"])
                    n_scored += 1
    assert kinds == set("M<>ID") and n_scored > 2000 and n_none > 200                        # every candidate kind wins somewhere
    # what has no score by the rule: L = 0, L = 1, R = 0, and R = 1 with L >= 5
    for x, y in (("", "K"), ("A", "KP"), ("ACA", ""), ("ACACA", "K"), ("ACACACA", "P")):
        assert ref.pair(x, y, sub, go, ge, fs) is None
    assert ref.pair("AC", "K", sub, go, ge, fs)["path"] == "<" and ref.pair("ACAC", "P", sub, go, ge, fs) is not None


def test_restatement_on_a_designed_pair():
    sub = np.full((27, 27), -4, dtype=np.int8)
    for a in range(1, 27):
        sub[a, a] = 5
    # GCT ATG AAA = A M K in frame; one letter less, one more
    assert ref.pair("GCTATGAAA", "AMK", sub, 10, 1, 8) == dict(score=15, jend=3, ref_from=1, n_match=3, n_ident=3, n_insert=0, n_delete=0, n_short=0, n_long=0, path="MMM")
    p = ref.pair("GCTAGAAA", "AMK", sub, 10, 1, 8)
    assert (p["score"], p["path"], p["n_short"], p["n_ident"]) == (5 - 4 - 8 + 5, "M<M", 1, 2)
    p = ref.pair("GCTCATGAAA", "AMK", sub, 10, 1, 8)
    assert (p["score"], p["path"], p["n_long"], p["n_ident"]) == (15 - 8, "M>M", 1, 3)
    # N inside a codon is X, TAA is class 0
    sub[24, 13] = 3                                                                          # X against M
    sub[0, 11] = 2                                                                           # * against K
    assert ref.pair("GCTANGTAA", "AMK", sub, 10, 1, 8)["score"] == 5 + 3 + 2


# ---- corrected sequences and the table -----------------------------------------------------------------------------------------------
def random_path(rng):
    path, x = [], []
    for _ in range(int(rng.integers(0, 40))):
        s = "MMMM<>ID"[int(rng.integers(8))]
        path.append(s)
        x.append("".join("ACGTacgtN"[int(k)] for k in rng.integers(0, 9, {"M": 3, "I": 3, "<": 2, ">": 4, "D": 0}[s])))
    return "".join(x), "".join(path)


def test_corrected_sequences_over_random_paths():
    rng = np.random.default_rng(5)
    for trial in range(500):
        x, path = random_path(rng)
        prot, nt = fsm.corrected(x, path)
        assert len(nt) == 3 * len(prot) == 3 * sum(s != "D" for s in path)
        assert "".join(fsm.codon_residue(nt[k:k + 3]) for k in range(0, len(nt), 3)) == prot.upper()
        assert all(c == (c.lower() if s == "I" else c.upper()) for c, s in zip(prot, path.replace("D", "")))
        sh = fsm.shifts_of(path)
        assert len(sh) == path.count("<") + path.count(">") and fsm.parse_shifts(fsm.shifts_text(sh)) == sh
        # the letters that stay are the contig's, in order: all but the dropped ones, and an N behind every short codon
        dropped = {v - 1 for v in sh if v > 0}
        padded = "".join(("" if k in dropped else c) + ("N" if -(k + 1) in sh else "") for k, c in enumerate(x))
        assert nt.upper() == padded.upper()
        if x:
            with pytest.raises(ValueError):
                fsm.corrected(x[:-1], path)
    assert fsm.corrected("GCTATCGAAtggTAA", "M<D>IM") == ("AXEw*", "GCTATNGAAtggTAA") and fsm.shifts_of("M<D>IM") == [-5, 6]
    assert fsm.shifts_text([-5, 6]) == "-5,+6" and fsm.shifts_text([]) == "."
    with pytest.raises(ValueError):
        fsm.corrected("ACG", "Z")


def test_table_round_trip(tmp_path):
    rng = np.random.default_rng(6)
    nucl, paths, recs = [], [], np.zeros(30, dtype=fsm.REC)
    for i in range(30):
        x, path = random_path(rng)
        if i % 7 == 3 or not path:
            nucl.append(x); paths.append("")
            recs[i] = (1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0)
            continue
        n = {s: path.count(s) for s in "M<>ID"}
        cols = n["M"] + n["<"] + n[">"] + n["D"]
        recs[i] = (0, int(rng.integers(0, 3)), int(rng.integers(-50, 200)), 2, 1 + cols, n["M"], int(rng.integers(0, n["M"] + n[">"] + 1)), n["I"], n["D"], n["<"], n[">"])
        nucl.append(x); paths.append(path)
    headers = [f"c{i} len={len(x)}" for i, x in enumerate(nucl)]
    ref_names, ref_seqs = ["r0", "r1", "r2"], ["A" * 50, "C" * 60, "D" * 70]
    fsm.write_frameshift(str(tmp_path / "t"), headers, nucl, ref_names, ref_seqs, dict(recs=recs, paths=paths))
    back = fsm.read_frameshift(str(tmp_path / "t_frameshift.txt"))
    assert back["names"] == [f"c{i}" for i in range(30)] and back["lens"].tolist() == [len(x) for x in nucl]
    assert back["shifts"] == [fsm.shifts_of(p) for p in paths]
    assert [(-1 if x is None else ref_names.index(x)) for x in back["ref_names"]] == recs["ref"].tolist()
    for f in fsm.REC.names:
        assert f == "ref" or np.array_equal(back["recs"][f], recs[f]), f
    assert np.allclose(back["identity"], [fsm.identity(r) for r in recs], atol=5e-5)
    # the two FASTA files: the aligned records, three letters per residue
    from megagta_amd.nearest import parse_fasta
    prot = parse_fasta(open(tmp_path / "t_corr_prot.fasta").read())
    nt = parse_fasta(open(tmp_path / "t_corr_nucl.fasta").read())
    assert [h for h, _ in prot] == [h for h, _ in nt] == [f"c{i}" for i in range(30) if recs[i]["status"] == 0]
    assert all(len(b) == 3 * len(a) for (_, a), (_, b) in zip(prot, nt))
    with pytest.raises(ValueError):
        fsm.parse_frameshift("no header\n")


# ---- the stand-alone check of the shared header --------------------------------------------------------------------------------------
def test_codons_and_corrected_sequences_under_sanitizers(tmp_path):
    exe = str(tmp_path / "frameshift_seq_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(CSRC, "host", "frameshift_seq_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# ---- the refusals of the command ----------------------------------------------------------------------------------------------------
FS_USAGE = "Usage: megagta nearest --frameshift <cost> <ref.faa> <nucl.fasta> <out_prefix> <gap_open> <gap_extend> <scoring>"


def run_cli(tmp_path, args):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    before = sorted(os.listdir(tmp_path))
    r = subprocess.run([BIN, "nearest"] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert sorted(os.listdir(tmp_path)) == before, "a refused call left a file"
    return r


@pytest.mark.parametrize("cost", ["a", "-1", "1025"])
def test_cli_refuses_a_bad_cost(tmp_path, cost):
    (tmp_path / "r.faa").write_text(">r\nAMK\n")
    (tmp_path / "n.fa").write_text(">c\nGCTATGAAA\n")
    r = run_cli(tmp_path, ["--frameshift", cost, "r.faa", "n.fa", "out", "10", "1", "5,-4"])
    assert r.returncode == 1 and "nearest" in r.stderr and "cost" in r.stderr and r.stdout == ""


@pytest.mark.parametrize("args", [["--frameshift"], ["--frameshift", "10"], ["--frameshift", "10", "r.faa", "n.fa", "out", "10", "1"],
                                  ["--frameshift", "10", "r.faa", "n.fa", "out", "10", "1", "5,-4", "more"], ["--frameshift", "r.faa", "n.fa", "out", "10", "1", "5,-4"]])
def test_cli_refuses_a_wrong_count_with_its_own_usage_line(tmp_path, args):
    r = run_cli(tmp_path, args)
    assert r.returncode == 1 and r.stderr.strip() == FS_USAGE and r.stdout == ""


@pytest.mark.parametrize("go,ge", [("7", "8"), ("1025", "1"), ("6", "-1"), ("x", "1")])
def test_cli_refuses_gap_costs_out_of_range(tmp_path, go, ge):
    (tmp_path / "r.faa").write_text(">r\nAMK\n")
    (tmp_path / "n.fa").write_text(">c\nGCTATGAAA\n")
    r = run_cli(tmp_path, ["--frameshift", "10", "r.faa", "n.fa", "out", go, ge, "5,-4"])
    assert r.returncode == 1 and "nearest" in r.stderr and "gap_open" in r.stderr
    r = run_cli(tmp_path, ["--frameshift", "10", "r.faa", "n.fa", "out", "10", "1", "5;-4"])
    assert r.returncode == 1 and "nearest: scoring" in r.stderr


def test_nearest_with_six_arguments_prints_its_usage_line_as_before(tmp_path):
    for args in (["a", "b", "c", "d", "e"], ["r.faa", "--frameshift", "10", "n.fa", "out", "10", "1", "5,-4"], []):
        r = run_cli(tmp_path, args)
        assert r.returncode == 1 and r.stderr.strip() == "Usage: megagta nearest <ref.faa> <prot.fasta> <out_prefix> <gap_open> <gap_extend> <scoring>"
