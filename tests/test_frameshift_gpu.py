"""mgta_seqs_frameshift on the device against tests/frameshift_ref.py, the rule of include/megagta_hip.h restated in Python (and pinned,
tie order included, by test_frameshift_host.py against an enumeration of every path).  Every comparison is exact: the score of EVERY
pair through `scores`, every record and every path byte for byte.  FrameBot is not available; the rule is this project's own
(INTEGRATION.md 2l')."""
import os
import subprocess
import sys

import numpy as np
import pytest

from megagta_amd import frameshift as fsm
from megagta_amd import nearest as nr
from megagta_amd import synth
from megagta_amd._lib import MegaGtaError
from tests import frameshift_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
NO_SCORE = -2 ** 31
NONE_REC = (1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0)


def mm(match=5, mismatch=-4):
    return nr.match_mismatch(match, mismatch)


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


def assert_is(ctx, nucl, refs, sub, go, ge, fs, what=""):
    """every pair's score, every record and every path against the restatement; returns (result, want)"""
    want = ref.frameshift(nucl, refs, sub, go, ge, fs)
    res = ctx.frameshift(nucl, refs, sub, go, ge, fs, scores=True, paths=True)
    assert res["scores"].shape == (len(nucl), len(refs))
    bad = np.argwhere(res["scores"] != want["scores"])
    assert bad.size == 0, (what, "score", bad[:5].tolist(), [(int(res["scores"][i, r]), int(want["scores"][i, r])) for i, r in bad[:5]])
    for i in range(len(nucl)):
        assert tuple(int(v) for v in res["recs"][i]) == tuple(int(v) for v in want["recs"][i]), (what, "record", i, tuple(res["recs"][i]), tuple(want["recs"][i]))
        assert res["paths"][i] == want["paths"][i], (what, "path", i, res["paths"][i], want["paths"][i])
        assert len(res["paths"][i]) <= len(nucl[i]) // 2 + (len(refs[int(want["recs"][i]["ref"])]) if want["recs"][i]["status"] == 0 else 0)
    st = res["stats"]
    al = want["recs"]["status"] == 0
    assert st["n_seqs"] == len(nucl) and st["n_refs"] == len(refs) and st["n_pairs"] == len(nucl) * len(refs)
    assert st["n_unaligned"] == int((~al).sum()) and st["n_cells"] == sum(map(len, nucl)) * sum(map(len, refs))
    assert st["n_trace_cells"] == sum(len(nucl[i]) * len(refs[int(want["recs"][i]["ref"])]) for i in range(len(nucl)) if al[i])
    assert st["n_shifted"] == int(((want["recs"]["n_short"] + want["recs"]["n_long"] > 0) & al).sum())
    # the records do not depend on whether every pair's score is asked for
    plain = ctx.frameshift(nucl, refs, sub, go, ge, fs)
    assert np.array_equal(plain["recs"], res["recs"]) and "scores" not in plain and "paths" not in plain, what
    return res, want


def steps(path, ref_from):
    """(state, the nucleotide row it ends at, its column) of every state of a path"""
    i, j, out = 0, ref_from - 1, []
    for s in path:
        i += {"M": 3, "I": 3, "<": 2, ">": 4, "D": 0}[s]
        j += s != "I"
        out.append((s, i, j))
    return out


def random_nt(rng, length, letters="AC"):
    return "".join(letters[int(k)] for k in rng.integers(0, len(letters), length))


def random_aa(rng, length, letters="KNTQHP"):                               # what the codons over {A, C} give
    return "".join(letters[int(k)] for k in rng.integers(0, len(letters), length))


def back_translate(rng, prot):
    """random synonymous codons"""
    out = []
    for a in prot:
        c = int(rng.choice(synth.codons_for(a)))
        out.append("ACGT"[c >> 4] + "ACGT"[(c >> 2) & 3] + "ACGT"[c & 3])
    return "".join(out)


# ---- 1. row and strip edges ----------------------------------------------------------------------------------------------------------
ROWS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 191, 192, 193]


@pytest.mark.parametrize("R", [1, 2, 3, 4, 63, 64, 65, 66, 68, 128, 129])
def test_row_and_strip_edges(ctx, R):
    rng = np.random.default_rng(100 + R)
    refs = [random_aa(rng, R), random_aa(rng, R)]
    nucl = [random_nt(rng, L) for L in ROWS]
    # contigs that follow the reference across the strip edges, with one letter taken out of, or put into, the codon of column 65 / 129
    planted = []
    for col in (65, 129):
        if R >= col:
            lo, hi = col - 6, min(R, col + 3)
            seg = back_translate(rng, refs[0][lo:hi])
            at = 3 * (col - 1 - lo)                                         # the first letter of the codon of column `col`
            # a letter that spoils the codon before it when that takes it in: only the long codon on column `col` keeps every residue
            extra = next(c for c in "GTCA" if fsm.codon_residue(seg[at - 2:at] + c) != refs[0][col - 2])
            planted += [(col, "<", seg[:at + 1] + seg[at + 2:]), (col, ">", seg[:at] + extra + seg[at:])]
    nucl += [x for _, _, x in planted]
    seen = set()
    for fs in (0, 3):
        res, want = assert_is(ctx, nucl, refs, mm(), 4, 1, fs, what=f"R={R} fs={fs}")
        for i in range(len(nucl)):
            if want["recs"][i]["status"] == 0:
                seen |= {(s, j) for s, _, j in steps(want["paths"][i], int(want["recs"][i]["ref_from"]))}
                seen |= {("B", row) for s, row, _ in steps(want["paths"][i], 1)[:1]}
        assert [int(s) for s in want["recs"]["status"][:2]] == [1, 1]       # L = 0 and L = 1 have no score
        assert (want["recs"]["status"][2:5] == 0).all()                     # L = 2, 3, 4 end in the first match state
    # the case tests what it claims: shifted codons on the first column of a strip, whose history came through the boundary rows, and B
    # at rows 2, 3 and 4
    for col, kind, _ in planted:
        assert (kind, col) in seen, (R, kind, col)
    assert {("B", 2), ("B", 3), ("B", 4)} <= seen and {"M", "<", ">"} <= {s for s, _ in seen}


# ---- 2. planted shifts ---------------------------------------------------------------------------------------------------------------
def test_planted_shifts(ctx):
    rng = np.random.default_rng(2)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    refs = [random_aa(rng, 50, aa), random_aa(rng, 40, aa)]
    nucl, segs, kinds = [], [], []
    for trial in range(80):
        at = int(rng.integers(0, 21))
        seg = refs[0][at:at + 30]
        x = back_translate(rng, seg)
        p = int(rng.integers(9, len(x) - 9))
        kind = "<" if trial % 2 == 0 else ">"
        nucl.append(x[:p] + x[p + 1:] if kind == "<" else x[:p] + "ACGT"[int(rng.integers(4))] + x[p:])
        segs.append(seg); kinds.append(kind)
    res, want = assert_is(ctx, nucl, refs, mm(5, -4), 10, 1, 8, what="planted")
    for i, (seg, kind) in enumerate(zip(segs, kinds)):
        rec, path = res["recs"][i], res["paths"][i]
        assert rec["ref"] == 0 and path.count(kind) == 1 and set(path) == {"M", kind} and len(path) == 30, (i, kind, path)
        assert rec["score"] >= 29 * 5 - 4 - 8
        prot, nt = fsm.corrected(nucl[i], path)
        assert sum(a == b for a, b in zip(prot, seg)) >= 29 and len(nt) == 90, (i, prot, seg)
    assert res["stats"]["n_shifted"] == 80


# ---- 3. in frame it is nearest ---------------------------------------------------------------------------------------------------------
def test_in_frame_is_nearest(ctx):
    rng = np.random.default_rng(3)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    sub = rng.integers(-4, 6, (27, 27)).astype(np.int8)
    refs = [random_aa(rng, int(n), aa) for n in (30, 45, 64, 70)]
    nucl = []
    for n in list(rng.integers(1, 41, 20)) + [1, 2, 40]:
        base = refs[int(rng.integers(4))]
        at = int(rng.integers(0, len(base)))
        prot = "".join(c if rng.random() < 0.8 else aa[int(rng.integers(20))] for c in (base + base)[at:at + int(n)])
        x = back_translate(rng, prot)
        if rng.random() < 0.3:
            x = x[:3 * (int(n) // 2)] + "TAA" + x[3 * (int(n) // 2) + 3:]     # a stop: class 0 on both sides
        nucl.append(x)
    prots = ["".join(fsm.codon_residue(x[k:k + 3]) for k in range(0, len(x), 3)) for x in nucl]
    near = ctx.nearest(prots, refs, sub, 9, 2, scores=True, paths=True)
    got = ctx.frameshift(nucl, refs, sub, 9, 2, 1024, scores=True, paths=True)
    assert (near["recs"]["status"] == 0).all()
    assert np.array_equal(got["scores"], near["scores"])
    for f in ("status", "ref", "score", "ref_from", "ref_to", "n_match", "n_ident", "n_insert", "n_delete"):
        assert np.array_equal(got["recs"][f], near["recs"][f]), f
    assert got["paths"] == near["paths"] and (got["recs"]["n_short"] == 0).all() and (got["recs"]["n_long"] == 0).all()
    assert got["stats"]["n_shifted"] == 0 and got["stats"]["n_cells"] == 3 * near["stats"]["n_cells"]
    assert_is(ctx, nucl[:6], refs, sub, 9, 2, 1024, what="in frame")


# ---- 4. reference boundaries inside strips -------------------------------------------------------------------------------------------
def test_reference_boundaries_inside_strips(ctx):
    rng = np.random.default_rng(4)
    refs = [random_aa(rng, 1 + k % 9) for k in range(40)] + [random_aa(rng, 70)]
    assert sorted(set(map(len, refs))) == list(range(1, 10)) + [70]
    # contigs that would run on from the tail of one reference into the head of the next if anything crossed a boundary, at every depth
    # of the history: joined in frame, one letter short and one letter long
    nucl = []
    for r in (3, 8, 12, 17, 25, 33, 39):
        a, b = back_translate(rng, refs[r]), back_translate(rng, refs[r + 1][:8])
        nucl += [a + b, a[:-1] + b, a + "C" + b]
    nucl += [random_nt(rng, int(n)) for n in (2, 3, 4, 11, 30)]
    for fs in (0, 3):
        res, want = assert_is(ctx, nucl, refs, mm(), 4, 1, fs, what=f"boundaries fs={fs}")
        assert res["stats"]["n_unaligned"] == 0 and (res["scores"][:, 40] > NO_SCORE).all()
    # first columns fell on many lanes
    starts = np.cumsum([0] + [len(r) for r in refs[:-1]])
    assert len({int(s) % 64 for s in starts}) >= 30


# ---- 5. segments -----------------------------------------------------------------------------------------------------------------------
def test_segments_of_references(ctx):
    rng = np.random.default_rng(5)
    refs = [random_aa(rng, int(n)) for n in rng.integers(90, 110, 24)]
    refs[23] = refs[1]                                                      # the same reference in the first and in the last segment: the lower index
    nucl = [back_translate(rng, refs[1][10:22]), back_translate(rng, refs[16][40:52])[:-2] + "A", random_nt(rng, 31)]
    res, want = assert_is(ctx, nucl, refs, mm(), 6, 1, 3, what="segments")
    assert res["stats"]["n_segments"] > 1 and sum(map(len, refs)) >= 2048
    assert res["recs"]["ref"][0] == 1 and res["scores"][0, 1] == res["scores"][0, 23]
    # with contigs enough to fill the device the references are one segment: the same records, scores and paths
    many = nucl + [""] * 10000
    one = ctx.frameshift(many, refs, mm(), 6, 1, 3, scores=True, paths=True)
    assert one["stats"]["n_segments"] == 1
    assert np.array_equal(one["recs"][:3], res["recs"]) and np.array_equal(one["scores"][:3], res["scores"]) and one["paths"][:3] == res["paths"]
    assert (one["recs"]["status"][3:] == 1).all() and (one["scores"][3:] == NO_SCORE).all()


# ---- 6. undefined pairs --------------------------------------------------------------------------------------------------------------
def test_undefined_pairs(ctx):
    sub = mm()
    # L = 0; L = 1; R = 1 with L = 5; among aligned contigs; an empty reference
    nucl, refs = ["", "A", "ACACA", "AAAAAC", "AC", "AAA", "AAAA"], ["K", "", "KN"]
    res, want = assert_is(ctx, nucl, refs, sub, 3, 1, 2, what="undefined")
    assert res["recs"]["status"].tolist() == [1, 1, 0, 0, 0, 0, 0] and res["stats"]["n_unaligned"] == 2
    assert (res["scores"][:2] == NO_SCORE).all() and (res["scores"][:, 1] == NO_SCORE).all()
    assert res["scores"][2, 0] == NO_SCORE and res["scores"][2, 2] > NO_SCORE                # R = 1 with L = 5 has no score, R = 2 has
    assert res["scores"][3].tolist() == [NO_SCORE, NO_SCORE, 10] and res["paths"][3] == "MM"
    res, want = assert_is(ctx, ["ACACA", "ACACACA"], ["K", "N"], sub, 3, 1, 2, what="every pair undefined")
    assert [tuple(r) for r in res["recs"]] == [NONE_REC] * 2
    # every contig empty, every reference empty, no reference at all
    for nucl, refs in ((["", ""], ["KN"]), (["AAA", "AC"], ["", ""]), (["AAA", "AC"], [])):
        res = ctx.frameshift(nucl, refs, sub, 3, 1, 2, scores=True, paths=True)
        assert [tuple(r) for r in res["recs"]] == [NONE_REC] * 2 and res["paths"] == ["", ""]
        assert res["scores"].shape == (2, len(refs)) and (res["scores"] == NO_SCORE).all()
        assert res["stats"]["n_unaligned"] == 2 and res["stats"]["n_batches"] == 0 and res["stats"]["n_refs"] == len(refs)
    res = ctx.frameshift([], ["KN"], sub, 3, 1, 2, scores=True, paths=True)
    assert len(res["recs"]) == 0 and all(v == 0 for v in res["stats"].values())


# ---- 7. ties -------------------------------------------------------------------------------------------------------------------------
def test_ties(ctx):
    # homopolymers: every place of the reference fits as well as every other, the lowest end column wins, and a codon before a shift
    nucl = ["A" * n for n in (2, 3, 4, 5, 6, 7, 8, 9, 30, 64)]
    refs = ["K" * n for n in (1, 2, 5, 70)]
    res, want = assert_is(ctx, nucl, refs, mm(), 3, 1, 2, what="homopolymers")
    assert res["recs"]["ref"][4] == 1 and res["paths"][4] == "MM" and (res["recs"]["ref_from"][4], res["recs"]["ref_to"][4]) == (1, 2)
    assert res["paths"][8] == "M" * 10 and res["recs"]["ref"][8] == 3 and res["recs"]["ref_to"][8] == 10
    # everything ties: sub all zero, gaps and shifts free; the candidate written first wins everywhere
    zero = np.zeros((27, 27), dtype=np.int8)
    res, want = assert_is(ctx, nucl + ["ACGTN" * 13], refs + ["KNTP" * 17], zero, 0, 0, 0, what="all zero")
    assert (res["recs"]["score"] == 0).all() and res["recs"]["ref"].tolist()[:4] == [0, 0, 0, 1]
    # u(j) equals e(i, j): a short codon ties with a codon one row further up
    same = np.full((27, 27), 2, dtype=np.int8)
    assert_is(ctx, nucl, refs, same, 2, 2, 0, what="all equal")
    assert_is(ctx, nucl, refs, mm(), 1, 0, 0, what="extend 0")


# ---- 8. the limits, in closed form ---------------------------------------------------------------------------------------------------
def path_score(x, y, sub, go, ge, fs, ref_from, path):
    total, prev = 0, None
    for s, i, j in steps(path, ref_from):
        if s in "M>":
            total += int(sub[nr.residue_class(ord(fsm.codon_residue(x[i - 3:i])))][nr.residue_class(ord(y[j - 1]))]) - (fs if s == ">" else 0)
        elif s == "<":
            total += int(sub[24][nr.residue_class(ord(y[j - 1]))]) - fs
        else:
            total -= ge if prev == s else go
        prev = s
    return total, i, j


def test_range_at_the_limits(ctx):
    hi = np.full((27, 27), 127, dtype=np.int8)
    res = ctx.frameshift(["GCT" * 4096], ["A" * 4096], hi, 1024, 1024, 1024, scores=True, paths=True)
    assert tuple(res["recs"][0]) == (0, 0, 127 * 4096, 1, 4096, 4096, 4096, 0, 0, 0, 0) and res["paths"][0] == "M" * 4096
    assert res["scores"].tolist() == [[127 * 4096]]
    st = res["stats"]
    assert st["waves_per_block"] == 1 and st["lds_bytes"] == 864 + 9 * 12288 and st["blocks_per_cu"] >= 1 and st["n_cells"] == 12288 * 4096
    # the worst: every residue costs 128, every gap residue and every shift 1024.  12288 letters against 2048 columns: a match state
    # takes three letters for 128, an insert state three for 1024, a long codon four for 1152, so the best path has all 2048 match
    # states and 2048 insert states between them, no shift, and ends on the last column
    lo = np.full((27, 27), -128, dtype=np.int8)
    x, y = "GCT" * 4096, "A" * 2048
    res = ctx.frameshift([x], [y], lo, 1024, 1024, 1024, scores=True, paths=True)
    rec = res["recs"][0]
    assert (rec["status"], rec["ref"], rec["score"]) == (0, 0, -(128 + 1024) * 2048) and res["scores"].tolist() == [[-(128 + 1024) * 2048]]
    assert (rec["ref_from"], rec["ref_to"], rec["n_match"], rec["n_insert"], rec["n_delete"], rec["n_short"], rec["n_long"], rec["n_ident"]) == (1, 2048, 2048, 2048, 0, 0, 0, 2048)
    assert path_score(x, y, lo, 1024, 1024, 1024, 1, res["paths"][0]) == (int(rec["score"]), 12288, 2048)
    # one more letter, one more residue
    for nucl, refs, word in ((["A" * 12289], ["K"], "12288 nucleotides per contig"), (["AAA"], ["K" * 4097], "4096 residues per reference")):
        with pytest.raises(MegaGtaError) as e:
            ctx.frameshift(nucl, refs, hi, 3, 1, 2)
        assert word in str(e.value)


# ---- 9. unknown letters and stops ----------------------------------------------------------------------------------------------------
def test_unknown_letters_and_stops(ctx):
    sub = mm()
    sub[24, :] = -1                                                         # X against anything
    sub[24, 13] = 3                                                         # X against M
    sub[0, :] = -2                                                          # a stop (class 0) against anything
    sub[0, 11] = 2                                                          # against K
    refs = ["AMK", "AKK", "MMMMMM"]
    nucl = ["GCTANGTAA", "GCTANGAAA", "gctatgaaa", "GCTATGAAA", "GCT-TGTGA", "NNNNNN", "GCTAT\xc1AAA", "TAATAGTGA"]
    res, want = assert_is(ctx, nucl, refs, sub, 10, 1, 8, what="unknown letters")
    assert res["scores"][0, 0] == 5 + 3 + 2 and res["recs"]["n_ident"][0] == 1                # N inside a codon scores as X, TAA as class 0
    assert res["scores"][1, 0] == 5 + 3 + 5 and res["scores"][2, 0] == res["scores"][3, 0] == 15
    assert res["recs"]["n_ident"][7] == 0 and res["recs"]["n_ident"][5] == 0                 # class 0 is never identical; X is not M


# ---- 10. the batch switch ------------------------------------------------------------------------------------------------------------
def test_batch_switch_moves_no_output(ctx):
    rng = np.random.default_rng(10)
    refs = [random_aa(rng, int(n)) for n in rng.integers(20, 50, 6)]
    nucl = [random_nt(rng, int(n)) for n in rng.integers(6, 90, 17)] + ["", "A"]
    try:
        ctx.set_nearest_batch(0)
        want = ctx.frameshift(nucl, refs, mm(), 4, 1, 3, scores=True, paths=True)
        assert want["stats"]["n_batches"] == 1
        n_aligned = len(nucl) - want["stats"]["n_unaligned"]
        seen = set()
        for cells in (1, 5000, 12000):                                     # pairs here have 500 to 3 800 cells
            ctx.set_nearest_batch(cells)
            got = ctx.frameshift(nucl, refs, mm(), 4, 1, 3, scores=True, paths=True)
            assert np.array_equal(got["recs"], want["recs"]) and got["paths"] == want["paths"] and np.array_equal(got["scores"], want["scores"]), cells
            for f in ("n_unaligned", "n_cells", "n_trace_cells", "n_shifted"):
                assert got["stats"][f] == want["stats"][f]
            seen.add(got["stats"]["n_batches"])
            assert got["stats"]["n_batches"] == n_aligned if cells == 1 else 1 < got["stats"]["n_batches"] < n_aligned
        assert len(seen) == 3
    finally:
        ctx.set_nearest_batch(0)
    assert_is(ctx, nucl[:5] + nucl[-2:], refs[:3], mm(), 4, 1, 3, what="batches")


# ---- 11. guards ----------------------------------------------------------------------------------------------------------------------
def test_guards(ctx):
    L = ctx._L
    nucl, refs = b"GCTATGAAAGCTAAA", b"AMKAKNT"
    off, roff = np.array([0, 9, 15], dtype=np.uint64), np.array([0, 3, 7], dtype=np.uint64)
    sub = mm()
    recs = np.full(2 * 11, 77, dtype=np.int32)
    scores = np.full(4, 77, dtype=np.int32)
    path = np.full(15 + 2 * 4096, 77, dtype=np.uint8)
    plen = np.full(2, 77, dtype=np.int32)
    stats = np.full(16, 77, dtype=np.int64)

    def call(nucl_p=nucl, off_p=off.ctypes.data, n=2, refs_p=refs, roff_p=roff.ctypes.data, n_ref=2, sub_p=sub.ctypes.data, go=6, ge=1, fs=4, recs_p=recs.ctypes.data,
             path_p=path.ctypes.data, plen_p=plen.ctypes.data, h=None):
        return L.mgta_seqs_frameshift(ctx.h if h is None else h[0], nucl_p, off_p, n, refs_p, roff_p, n_ref, sub_p, go, ge, fs, recs_p, scores.ctypes.data, path_p, plen_p,
                                      stats.ctypes.data)

    def refused(word, **kw):
        assert call(**kw) == -1 and word in L.mgta_last_error() and b"mgta_seqs_frameshift" in L.mgta_last_error(), (kw, L.mgta_last_error())

    refused(b"ctx", h=(None,))
    refused(b"n = -1", n=-1)
    refused(b"n_ref = -1", n_ref=-1)
    refused(b"offsets", off_p=None)
    refused(b"ref_offsets", roff_p=None)
    refused(b"recs", recs_p=None)
    refused(b"sub", sub_p=None)
    refused(b"nucl", nucl_p=None)
    refused(b"refs", refs_p=None)
    refused(b"path_len", plen_p=None)
    for go, ge in ((6, 7), (6, -1), (1025, 1), (-1, -1)):
        refused(b"gap_open", go=go, ge=ge)
    for fs in (-1, 1025):
        refused(b"0 <= frameshift <= 1024", fs=fs)
    down = np.array([0, 5, 4], dtype=np.uint64)
    refused(b"ascend", off_p=down.ctypes.data)
    refused(b"ascend", roff_p=down.ctypes.data)
    long_off, long_roff = np.array([0, 12289, 12290], dtype=np.uint64), np.array([0, 4097, 4098], dtype=np.uint64)
    refused(b"12288 nucleotides per contig", off_p=long_off.ctypes.data)
    refused(b"4096 residues per reference", roff_p=long_roff.ctypes.data)
    many = np.arange(0, (2 ** 19 + 1) * 4096, 4096, dtype=np.uint64)       # 2^19 references of 4096 residues: 2^31 columns
    refused(b"2^31 residues", roff_p=many.ctypes.data, n_ref=many.size - 1)
    refused(b"2^31 contigs", n=2 ** 31)
    refused(b"2^31 references", n_ref=2 ** 31)
    # nothing was written by the refused calls
    assert (recs == 77).all() and (scores == 77).all() and (path == 77).all() and (plen == 77).all() and (stats == 77).all()
    # the same arguments with everything in place: a valid call
    assert call() == 0
    want = ref.frameshift(["GCTATGAAA", "GCTAAA"], ["AMK", "AKNT"], sub, 6, 1, 4)
    assert np.array_equal(scores.reshape(2, 2), want["scores"]) and np.array_equal(recs.view(fsm.REC), want["recs"])
    assert plen.tolist() == [3, 2] and path[:3].tobytes() == b"MMM" and path[9 + 4096:9 + 4096 + 2].tobytes().decode() == want["paths"][1]
    assert stats[0] == 2 and stats[1] == 2 and stats[2] == 4 and stats[15] == 0
    # n = 0: MGTA_OK, stats all zero, whatever else is NULL
    assert L.mgta_seqs_frameshift(ctx.h, None, None, 0, None, None, 0, None, 6, 1, 4, None, None, None, None, stats.ctypes.data) == 0 and (stats[:13] == 0).all() and stats[15] == 0


# ---- 12. files: one process per call and the worker ----------------------------------------------------------------------------------
MATRIX = """# a few letters and the rest
   A  K  N  T  X  *
A  4 -1 -2 -1 -1 -4
K -1  6 -3 -2 -1 -4
N -2 -3  5  2 -1 -4
T -1 -2  2  5 -1 -4
X -1 -1 -1 -1 -1 -4
* -4 -4 -4 -4 -4  1
"""


def fasta_case(seed):
    rng = np.random.default_rng(seed)
    aa = "AKNTQHP"
    ref_names = [f"ref{j}" for j in range(5)]
    ref_lines = []
    for j in range(5):
        s = random_aa(rng, int(rng.integers(40, 70)), aa)
        at = int(rng.integers(5, 30))
        ref_lines.append(s[:at].lower() + "--." + s[at:at + 20] + "\n" + s[at + 20:] + "*")        # an alignment, on two lines
    clean = [s.replace("-", "").replace(".", "").replace("*", "").replace("\n", "").upper() for s in ref_lines]
    nucl = []
    for k in range(24):
        r = clean[int(rng.integers(5))]
        at = int(rng.integers(0, len(r) - 15))
        x = back_translate(rng, r[at:at + int(rng.integers(8, 15))])
        p = int(rng.integers(4, len(x) - 4))
        nucl.append(x if k % 3 == 0 else x[:p] + x[p + 1:] if k % 3 == 1 else x[:p] + "T" + x[p:])
    nucl += ["", "A", "ACNGT-ACGTAC", "gctatgaaa"]
    headers = [f"c{j} len={len(s)}" if j % 3 else f"c{j}" for j, s in enumerate(nucl)]
    return headers, nucl, ref_names, ref_lines, clean


def test_one_shot_and_worker_write_the_same_files(ctx, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    (tmp_path / "m.txt").write_text(MATRIX)
    cases = [fasta_case(4), fasta_case(5)]
    scoring = ["5,-4", str(tmp_path / "m.txt")]
    tails = ("_frameshift.txt", "_corr_prot.fasta", "_corr_nucl.fasta")
    for i, (headers, nucl, ref_names, ref_lines, _) in enumerate(cases):
        open(tmp_path / f"n{i}.fa", "w").write("".join(f">{h}\n{s}\n" for h, s in zip(headers, nucl)))
        open(tmp_path / f"r{i}.faa", "w").write("".join(f">{h} some words\n{s}\n" for h, s in zip(ref_names, ref_lines)))
        subprocess.run([BIN, "nearest", "--frameshift", "6", str(tmp_path / f"r{i}.faa"), str(tmp_path / f"n{i}.fa"), str(tmp_path / f"one{i}"), "7", "2", scoring[i]],
                       check=True, capture_output=True, timeout=120)
    req = "".join(f"nearest\t--frameshift\t6\t{tmp_path}/r{i}.faa\t{tmp_path}/n{i}.fa\t{tmp_path}/w{i}\t7\t2\t{scoring[i]}\n" for i in range(2)) + "quit\n"
    r = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0", "DONE", "0"], r.stderr[-2000:]
    for i, (headers, nucl, ref_names, ref_lines, clean) in enumerate(cases):
        names, ref_seqs = nr.read_refs(str(tmp_path / f"r{i}.faa"))
        assert names == ref_names and ref_seqs == clean
        sub = nr.parse_scoring(scoring[i])
        res, want = assert_is(ctx, nucl, ref_seqs, sub, 7, 2, 6, what=f"files {i}")
        assert res["stats"]["n_unaligned"] == 2 and res["stats"]["n_shifted"] >= 8
        fsm.write_frameshift(str(tmp_path / f"py{i}"), headers, nucl, names, ref_seqs, res)
        for tail in tails:
            text = open(f"{tmp_path}/py{i}{tail}").read()
            assert open(f"{tmp_path}/one{i}{tail}").read() == open(f"{tmp_path}/w{i}{tail}").read() == text and len(text) > 0, (i, tail)
        back = fsm.read_frameshift(f"{tmp_path}/one{i}_frameshift.txt")
        first = nr.ref_index(names)
        assert [(-1 if x is None else first[x]) for x in back["ref_names"]] == res["recs"]["ref"].tolist()
        for f in fsm.REC.names:
            assert f == "ref" or np.array_equal(back["recs"][f], res["recs"][f]), f
        assert back["shifts"] == [fsm.shifts_of(p) for p in res["paths"]]
    # no file of `nearest` itself, and nothing but the three files per prefix
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("one0")) == sorted("one0" + t for t in tails)
    # a cost out of range, a matrix with a value outside int8: the step fails and leaves nothing
    (tmp_path / "bad.txt").write_text(MATRIX.replace(" 6 ", " 200 "))
    for j, (cost, tail) in enumerate((("1025", ["7", "2", "5,-4"]), ("6", ["7", "2", str(tmp_path / "bad.txt")]))):
        r = subprocess.run([BIN, "nearest", "--frameshift", cost, str(tmp_path / "r0.faa"), str(tmp_path / "n0.fa"), str(tmp_path / f"bad{j}")] + tail,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "nearest" in r.stderr
    assert [f for f in os.listdir(tmp_path) if f.startswith("bad") and f != "bad.txt"] == []


# ---- 13. driver end to end -----------------------------------------------------------------------------------------------------------
def check_driver_files(nucl_prefix, prot_prefix, ref_path, scoring, go, ge, fs):
    """NUCL_PREFIX.fasta and its three files: every line is what the restatement gives on the file's sequences; on this clean sample
    no contig is shifted and its corrected protein is its record of PROT_PREFIX.fasta"""
    with open(nucl_prefix + ".fasta", encoding="latin-1") as fh:
        records = nr.parse_fasta(fh.read())
    with open(prot_prefix + ".fasta", encoding="latin-1") as fh:
        prot_records = nr.parse_fasta(fh.read())
    names, ref_seqs = nr.read_refs(ref_path)
    nucl = [s for _, s in records]
    want = ref.frameshift(nucl, ref_seqs, nr.parse_scoring(scoring), go, ge, fs)
    assert len(records) > 0 and (want["recs"]["status"] == 0).all()
    cnames = [nr.record_name(h) for h, _ in records]
    assert open(nucl_prefix + "_frameshift.txt", encoding="latin-1").read() == fsm.frameshift_text(cnames, [len(s) for s in nucl], names, [len(s) for s in ref_seqs],
                                                                                                   want["recs"], want["paths"])
    prot, nt = fsm.corrected_texts(cnames, nucl, want["recs"], want["paths"])
    assert open(nucl_prefix + "_corr_prot.fasta", encoding="latin-1").read() == prot and open(nucl_prefix + "_corr_nucl.fasta", encoding="latin-1").read() == nt
    table = fsm.read_frameshift(nucl_prefix + "_frameshift.txt")
    assert table["shifts"] == [[]] * len(records)
    corr = nr.parse_fasta(prot)
    assert [nr.record_name(h) for h, _ in prot_records] == cnames and [s.upper() for _, s in corr] == [s.upper() for _, s in prot_records]
    return len(records)


def test_driver_frameshift_end_to_end(golden_dir, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    mg = synth.make_metagenome(6000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)    # the sample of test_driver_nearest_end_to_end
    synth.write_fasta(mg.reads, str(tmp_path / "reads.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "45", "-t", "4", "--min-contig-len", "150"]

    def step_files(out):
        return sorted(f for _, _, files in os.walk(out) for f in files if "_frameshift" in f or "_corr_" in f)

    # without the flag: no file of the step, and the checkpoints of a run without flags
    out = tmp_path / "out"
    r = subprocess.run(base + ["-o", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
    assert step_files(out) == [] and open(out / "tmp" / "cp.txt").read().splitlines() == [f"{i}\tdone" for i in range(6)]
    assert "Placing the nucleotide contigs" not in open(out / "log").read()
    # the flag alone: the step reads every nucleotide contig, and its checkpoint is the last
    out1 = tmp_path / "out1"
    r = subprocess.run(base + ["-o", str(out1), "--frameshift"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out1 / "log").read()[-2000:]
    d = out1 / "contigs" / "rplB"
    assert step_files(out1) == ["nucl_merged_corr_nucl.fasta", "nucl_merged_corr_prot.fasta", "nucl_merged_frameshift.txt"]
    n_all = check_driver_files(str(d / "nucl_merged"), str(d / "prot_merged"), f"{toy}/ref_aligned.faa", "5,-4", 10, 1, 10)
    assert open(d / "nucl_merged.fasta").read() == open(out / "contigs" / "rplB" / "nucl_merged.fasta").read()      # the run is what it was
    assert open(out1 / "tmp" / "cp.txt").read().splitlines() == [f"{i}\tdone" for i in range(6 + 1)]
    assert open(out1 / "log").read().count("Placing the nucleotide contigs of rplB on the references with frameshifts") == 1
    # behind --derep --align --cluster --nearest, with parameters of its own: the step reads the representatives, and its checkpoint is the last
    out2 = tmp_path / "out2"
    r = subprocess.run(base + ["-o", str(out2), "--derep", "--align", "--cluster", "--nearest", "--frameshift", "--frameshift-cost", "7", "--nearest-scoring", "3,-2",
                               "--nearest-gap-open", "5", "--nearest-gap-extend", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out2 / "log").read()[-2000:]
    d = out2 / "contigs" / "rplB"
    assert step_files(out2) == [f"nucl_merged_rmdup_rep_seqs_{t}" for t in ("corr_nucl.fasta", "corr_prot.fasta", "frameshift.txt")]
    n_rep = check_driver_files(str(d / "nucl_merged_rmdup_rep_seqs"), str(d / "prot_merged_rmdup_rep_seqs"), f"{toy}/ref_aligned.faa", "3,-2", 5, 2, 7)
    assert 0 < n_rep <= n_all
    # the checkpoints: six of a run without flags, then derep, align, cluster, nearest, frameshift (one gene each)
    assert open(out2 / "tmp" / "cp.txt").read().splitlines() == [f"{i}\tdone" for i in range(6 + 5)]
    log = open(out2 / "log").read()
    assert log.index("Finding the nearest reference") < log.index("Placing the nucleotide contigs")
    # an option out of range is refused before anything runs
    r = subprocess.run(base + ["-o", str(tmp_path / "out3"), "--frameshift", "--frameshift-cost", "1025"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--frameshift-cost" in r.stderr + r.stdout and not os.path.exists(tmp_path / "out3" / "contigs")
    print(f"driver: {n_all} contigs, {n_rep} representatives")
