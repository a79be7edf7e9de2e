"""mgta_seqs_nearest on the device against `restate`, the rule of include/megagta_hip.h written out in Python: nested loops over Python
ints, None for undefined, the tie rules spelled out.  Every comparison is exact: the score of EVERY pair through `scores`, every record
and every path byte for byte.  FrameBot and RDPTools are not available; the rule is this project's own."""
import os
import subprocess
import sys

import numpy as np
import pytest

from megagta_amd import nearest as nr
from megagta_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
NO_SCORE = -2 ** 31


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------
def cls(b: int) -> int:
    if 65 <= b <= 90:
        return b - 64
    if 97 <= b <= 122:
        return b - 96
    return 0


def restate(x: bytes, y: bytes, sub, go: int, ge: int):
    """None when the pair has no score, else dict(score, ref_from, ref_to, n_match, n_ident, n_insert, n_delete, path)"""
    L, R = len(x), len(y)
    if L == 0 or R == 0:
        return None
    S = [[int(v) for v in row] for row in sub]
    cx, cy = [cls(b) for b in x], [cls(b) for b in y]
    M = [[None] * (R + 1) for _ in range(L + 1)]
    X = [[None] * (R + 1) for _ in range(L + 1)]
    Y = [[None] * (R + 1) for _ in range(L + 1)]
    fM = [[None] * (R + 1) for _ in range(L + 1)]
    fX = [[None] * (R + 1) for _ in range(L + 1)]
    fY = [[None] * (R + 1) for _ in range(L + 1)]
    for i in range(1, L + 1):
        Mi, Xi, Yi, Mp, Xp, Yp, Si = M[i], X[i], Y[i], M[i - 1], X[i - 1], Y[i - 1], S[cx[i - 1]]
        for j in range(1, R + 1):
            # M: the candidates in the order B, M, X, Y; a later one wins only when it is strictly larger
            v = f = None
            if i == 1:
                v, f = 0, "B"
            elif j > 1:
                for name, c in (("M", Mp[j - 1]), ("X", Xp[j - 1]), ("Y", Yp[j - 1])):
                    if c is not None and (v is None or c > v):
                        v, f = c, name
            if v is not None:
                Mi[j], fM[i][j] = Si[cy[j - 1]] + v, f
            # X: M, X
            if i > 1:
                v = f = None
                if Mp[j] is not None:
                    v, f = Mp[j] - go, "M"
                if Xp[j] is not None and (v is None or Xp[j] - ge > v):
                    v, f = Xp[j] - ge, "X"
                Xi[j], fX[i][j] = v, f
            # Y: M, Y
            if j > 1:
                v = f = None
                if Mi[j - 1] is not None:
                    v, f = Mi[j - 1] - go, "M"
                if Yi[j - 1] is not None and (v is None or Yi[j - 1] - ge > v):
                    v, f = Yi[j - 1] - ge, "Y"
                Yi[j], fY[i][j] = v, f
    ends = [j for j in range(1, R + 1) if M[L][j] is not None]
    if not ends:
        return None
    score = max(M[L][j] for j in ends)
    end = min(j for j in ends if M[L][j] == score)                        # the lowest column that reaches the score
    out = dict(score=score, ref_to=end, n_match=0, n_ident=0, n_insert=0, n_delete=0)
    i, j, state, path = L, end, "M", []
    while state != "B":
        path.append({"M": "M", "X": "I", "Y": "D"}[state])
        if state == "M":
            out["n_match"] += 1
            out["n_ident"] += int(cx[i - 1] == cy[j - 1] != 0)
            out["ref_from"] = j
            state, i, j = fM[i][j], i - 1, j - 1
        elif state == "X":
            out["n_insert"] += 1
            state, i = fX[i][j], i - 1
        else:
            out["n_delete"] += 1
            state, j = fY[i][j], j - 1
    assert i == 0
    out["path"] = "".join(reversed(path))
    return out


def restate_nearest(seqs, refs, sub, go, ge):
    """-> (scores as a list of lists with None, per contig None or (ref, the dict of restate))"""
    table = [[restate(x, y, sub, go, ge) for y in refs] for x in seqs]
    scores = [[None if t is None else t["score"] for t in row] for row in table]
    near = []
    for row in table:
        best = None
        for r, t in enumerate(row):
            if t is not None and (best is None or t["score"] > row[best]["score"]):      # on a tie the lowest reference index
                best = r
        near.append(None if best is None else (best, row[best]))
    return scores, near


def last_row_by_diagonals(x: bytes, y: bytes, sub, go: int, ge: int):
    """score(x, y) of the same rule, one numpy step per anti-diagonal in int64 with a sentinel far below every value (for the sizes
    where `restate` would take minutes; test_diagonals_agree_with_restate ties it to `restate`)"""
    L, R = len(x), len(y)
    if L == 0 or R == 0:
        return None
    NEG = -(1 << 50)
    S = np.asarray(sub, dtype=np.int64)
    cx, cy = np.array([cls(b) for b in x]), np.array([cls(b) for b in y])
    new = lambda: np.full(L + 1, NEG, dtype=np.int64)                    # indexed by the row; a diagonal holds the cells with i + j = d
    M1, X1, Y1, D2 = new(), new(), new(), new()
    last = np.full(R + 1, NEG, dtype=np.int64)
    for d in range(2, L + R + 1):
        lo, hi = max(1, d - R), min(L, d - 1)
        i = np.arange(lo, hi + 1)
        j = d - i
        Md, Xd, Yd = new(), new(), new()
        diag = np.where(i == 1, 0, np.where(j > 1, D2[i - 1], NEG))
        Md[i] = np.where(diag > NEG // 2, S[cx[i - 1], cy[j - 1]] + diag, NEG)
        Xd[i] = np.where(i > 1, np.maximum(M1[i - 1] - go, X1[i - 1] - ge), NEG)
        Yd[i] = np.where(j > 1, np.maximum(M1[i] - go, Y1[i] - ge), NEG)
        for T in (Xd, Yd):
            T[T < NEG // 2] = NEG
        if hi == L:
            last[d - L] = Md[L]
        D2 = np.maximum(np.maximum(M1, X1), Y1)
        M1, X1, Y1 = Md, Xd, Yd
    best = int(last.max())
    return None if best < NEG // 2 else best


def path_score(x: bytes, y: bytes, sub, go, ge, ref_from, path):
    """the score of one state path under the rule, and where it ends"""
    i, j, total, prev = 0, ref_from - 1, 0, None
    for s in path:
        if s == "M":
            i, j = i + 1, j + 1
            total += int(sub[cls(x[i - 1])][cls(y[j - 1])])
        elif s == "I":
            i += 1
            total -= ge if prev == "I" else go
        else:
            j += 1
            total -= ge if prev == "D" else go
        prev = s
    return total, i, j


def mm(match=5, mismatch=-4):
    return nr.match_mismatch(match, mismatch)


def assert_is(ctx, seqs, refs, sub, go, ge, what=""):
    """every pair's score, every record and every path against restate; returns (result, near)"""
    want_scores, near = restate_nearest(seqs, refs, sub, go, ge)
    res = ctx.nearest(seqs, refs, sub, go, ge, scores=True, paths=True)
    got = res["scores"]
    assert got.shape == (len(seqs), len(refs))
    for i, row in enumerate(want_scores):
        for r, v in enumerate(row):
            assert got[i, r] == (NO_SCORE if v is None else v), (what, "score", i, r, int(got[i, r]), v)
    for i, t in enumerate(near):
        rec = res["recs"][i]
        if t is None:
            assert tuple(rec) == (1, -1, 0, 0, 0, 0, 0, 0, 0) and res["paths"][i] == "", (what, "unaligned", i, tuple(rec))
            continue
        r, w = t
        assert tuple(int(v) for v in rec) == (0, r, w["score"], w["ref_from"], w["ref_to"], w["n_match"], w["n_ident"], w["n_insert"], w["n_delete"]), \
            (what, "record", i, tuple(rec), r, w)
        assert res["paths"][i] == w["path"] and len(w["path"]) == len(seqs[i]) + w["n_delete"], (what, "path", i)
    st = res["stats"]
    assert st["n_seqs"] == len(seqs) and st["n_refs"] == len(refs) and st["n_pairs"] == len(seqs) * len(refs)
    assert st["n_unaligned"] == sum(t is None for t in near) and st["n_cells"] == sum(map(len, seqs)) * sum(map(len, refs))
    assert st["n_trace_cells"] == sum(len(seqs[i]) * len(refs[t[0]]) for i, t in enumerate(near) if t is not None)
    # the records do not depend on whether every pair's score is asked for
    plain = ctx.nearest(seqs, refs, sub, go, ge)
    assert np.array_equal(plain["recs"], res["recs"]) and "scores" not in plain and "paths" not in plain, what
    return res, near


ALPHABET = b"ACDEK"


def variant(rng, base: bytes, length: int, subs=0.15, indels=0.06) -> bytes:
    """`length` residues that follow `base` with substitutions, insertions and deletions (a small alphabet: ties and gaps are common)"""
    out, p = bytearray(), int(rng.integers(0, max(1, len(base) - length + 1))) if len(base) > length else 0
    while len(out) < length:
        u = rng.random()
        if u < indels:
            out.append(ALPHABET[int(rng.integers(len(ALPHABET)))])        # an inserted residue
        elif u < 2 * indels:
            p += 1                                                        # a skipped one
        else:
            c = base[p % len(base)] if base else ALPHABET[0]
            out.append(ALPHABET[int(rng.integers(len(ALPHABET)))] if rng.random() < subs else c)
            p += 1
    return bytes(out)


def random_seq(rng, length: int) -> bytes:
    return bytes(ALPHABET[int(k)] for k in rng.integers(0, len(ALPHABET), length))


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


# ---- 0. the two restatements agree (no device) -----------------------------------------------------------------------------------------
def test_diagonals_agree_with_restate():
    rng = np.random.default_rng(7)
    sub = mm()
    sub[0, :] = sub[:, 0] = -2
    for trial in range(60):
        L, R = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        x, y = random_seq(rng, L), random_seq(rng, R)
        go = int(rng.integers(0, 9))
        ge = int(rng.integers(0, go + 1))
        t = restate(x, y, sub, go, ge)
        assert last_row_by_diagonals(x, y, sub, go, ge) == (None if t is None else t["score"]), (trial, x, y, go, ge)
        if t is not None:
            assert path_score(x, y, sub, go, ge, t["ref_from"], t["path"]) == (t["score"], L, t["ref_to"])
    assert restate(b"AC", b"A", sub, 3, 1) is None and last_row_by_diagonals(b"AC", b"A", sub, 3, 1) is None


# ---- 1. strip and row edges ----------------------------------------------------------------------------------------------------------
EDGES = [1, 2, 63, 64, 65, 128, 129]


@pytest.mark.parametrize("R", EDGES)
@pytest.mark.parametrize("L", EDGES)
def test_strip_and_row_edges(ctx, L, R):
    rng = np.random.default_rng(1000 * L + R)
    base = random_seq(rng, 160)
    refs = [variant(rng, base, R) for _ in range(2)]
    seqs = [variant(rng, base, L), variant(rng, refs[1], L, subs=0.05, indels=0.03)]
    assert_is(ctx, seqs, refs, mm(), 6, 1, what=f"L={L} R={R}")


# ---- 2. reference boundaries that do not fall on a strip boundary ---------------------------------------------------------------------
def boundary_refs(rng):
    lens = []
    for k in range(20):                                                   # 1, 63, 1, 64, 2, 65, 2, 66, ...: 40 references
        lens += [1 + k // 2, 63 + k]
    return [random_seq(rng, n) for n in lens]


def test_reference_boundaries_inside_strips(ctx):
    rng = np.random.default_rng(21)
    refs = boundary_refs(rng)
    assert len(refs) == 40 and [len(r) for r in refs[:6]] == [1, 63, 1, 64, 2, 65]
    # contigs whose best alignment would cross a boundary if the reset were missing: the tail of reference r and the head of r + 1
    seqs = []
    for r in (1, 2, 5, 8, 17, 30, 37):
        seqs.append(refs[r][-16:] + refs[r + 1][:16])
    seqs += [refs[3][-10:] + refs[4] + refs[5][:10], refs[39][-20:], refs[0] + refs[1][:20]]
    res, near = assert_is(ctx, seqs, refs, mm(), 8, 2, what="boundaries")
    assert res["stats"]["n_unaligned"] == 0
    # the joined contig fits no single reference: it pays for the half it does not share
    for i in range(7):
        assert near[i][1]["score"] < 5 * len(seqs[i])
    assert near[8] == (39, restate(seqs[8], refs[39], mm(), 8, 2)) and near[8][1]["score"] == 100 and near[8][1]["ref_to"] == len(refs[39])


def test_segments_of_references(ctx):
    """few contigs and many columns: the score pass cuts the references into segments; the same reference in the first and in the last
    segment ties, and the lower index wins"""
    rng = np.random.default_rng(22)
    base = random_seq(rng, 120)
    refs = [variant(rng, base, int(rng.integers(100, 110))) for _ in range(22)]
    refs[21] = refs[1]
    seqs = [variant(rng, refs[1], 34, subs=0.02, indels=0.02), variant(rng, refs[16], 30), variant(rng, base, 26)]
    res, near = assert_is(ctx, seqs, refs, mm(), 7, 1, what="segments")
    assert res["stats"]["n_segments"] > 1 and sum(map(len, refs)) >= 2048
    assert near[0][0] == 1 and res["scores"][0, 1] == res["scores"][0, 21]


# ---- 3. undefined pairs --------------------------------------------------------------------------------------------------------------
def test_undefined_pairs(ctx):
    sub = mm()
    # R = 1 < L: no M[L][1]; an empty contig; an empty reference; an unaligned contig among aligned ones
    res, near = assert_is(ctx, [b"ACD", b"", b"A", b"CC"], [b"A", b"", b"C"], sub, 3, 1, what="undefined")
    assert [t is None for t in near] == [True, True, False, True] and res["stats"]["n_unaligned"] == 3
    assert (res["scores"][0] == NO_SCORE).all() and res["scores"][2].tolist() == [5, NO_SCORE, -4]
    res, near = assert_is(ctx, [b"ACDE", b"AC"], [b"C", b"ACDEK", b""], sub, 3, 1, what="one aligned")
    assert [t is None for t in near] == [False, False] and res["recs"]["ref"].tolist() == [1, 1]
    # every contig empty, every reference empty, no reference at all
    for seqs, refs in (([b"", b""], [b"ACD"]), ([b"ACD", b"A"], [b"", b""]), ([b"ACD", b"A"], [])):
        res = ctx.nearest(seqs, refs, sub, 3, 1, scores=True, paths=True)
        assert [tuple(r) for r in res["recs"]] == [(1, -1, 0, 0, 0, 0, 0, 0, 0)] * 2 and res["paths"] == ["", ""]
        assert res["scores"].shape == (2, len(refs)) and (res["scores"] == NO_SCORE).all()
        assert res["stats"]["n_unaligned"] == 2 and res["stats"]["n_batches"] == 0 and res["stats"]["n_refs"] == len(refs)
    res = ctx.nearest([], [b"ACD"], sub, 3, 1, scores=True, paths=True)
    assert len(res["recs"]) == 0 and all(v == 0 for v in res["stats"].values())


# ---- 4. ties -------------------------------------------------------------------------------------------------------------------------
def test_ties(ctx):
    rng = np.random.default_rng(41)
    p, q = random_seq(rng, 30), random_seq(rng, 70)
    # equal-scoring references: the lowest index; a contig that fits one reference at two places: the lowest end column
    refs = [q, b"KK" + p + b"KK", b"KK" + p + b"KK", p + q + p, p]
    res, near = assert_is(ctx, [p, p[3:27], q[5:60]], refs, mm(), 6, 1, what="ties")
    assert near[0][0] == 1 and near[0][1]["score"] == 150 and res["scores"][0].tolist()[1:] == [150] * 4
    res, near = assert_is(ctx, [p], [p + q + p, q], mm(), 6, 1, what="two places")
    assert near[0][1]["ref_to"] == 30 and near[0][1]["ref_from"] == 1
    # B / M / X / Y ties everywhere: sub all zero, gaps free
    zero = np.zeros((27, 27), dtype=np.int8)
    seqs = [random_seq(rng, n) for n in (1, 2, 5, 64, 70)]
    refs = [random_seq(rng, n) for n in (1, 3, 66, 64)]
    res, near = assert_is(ctx, seqs, refs, zero, 0, 0, what="all zero")
    assert all(t[1]["score"] == 0 for t in near) and [t[0] for t in near] == [0, 1, 1, 1, 1]     # R = 1 < L has no score; R = 3 has
    # gap_open == gap_extend, and a gap that costs nothing to open
    base = random_seq(rng, 90)
    seqs = [variant(rng, base, n, indels=0.12) for n in (40, 66, 80)]
    refs = [variant(rng, base, n, indels=0.12) for n in (70, 90, 64)]
    assert_is(ctx, seqs, refs, mm(), 3, 3, what="open == extend")
    assert_is(ctx, seqs, refs, mm(2, -3), 1, 0, what="extend 0")


# ---- 5. range ------------------------------------------------------------------------------------------------------------------------
def test_range_at_the_limits(ctx):
    """sub at +-127 (and -128 against a byte that is no letter) with L = R = 4096: the largest and the smallest defined values.  `restate`
    would take minutes here: every pair's score is compared with last_row_by_diagonals, and every record with its own path scored under
    the rule"""
    rng = np.random.default_rng(51)
    sub = nr.match_mismatch(127, -127)
    sub[0, :] = sub[:, 0] = -128
    p = bytes(b"ACDEFGHIKLMNPQRSTVWY"[int(k)] for k in rng.integers(0, 20, 4096))
    seqs, refs = [p, b"B" * 2048 + b"*" * 2048], [p]
    go = ge = 1024
    res = ctx.nearest(seqs, refs, sub, go, ge, scores=True, paths=True)
    for i, x in enumerate(seqs):
        want = last_row_by_diagonals(x, p, sub, go, ge)
        print(f"range: contig {i}: score {int(res['scores'][i, 0])}, by diagonals {want}")
        assert res["scores"][i, 0] == want
    assert res["scores"][:, 0].tolist() == [127 * 4096, -127 * 2048 - 128 * 2048]
    assert tuple(res["recs"][0]) == (0, 0, 127 * 4096, 1, 4096, 4096, 4096, 0, 0) and res["paths"][0] == "M" * 4096
    assert tuple(res["recs"][1]) == (0, 0, -255 * 2048, 1, 4096, 4096, 0, 0, 0) and res["paths"][1] == "M" * 4096
    for i, rec in enumerate(res["recs"]):
        assert path_score(seqs[i], p, sub, go, ge, int(rec["ref_from"]), res["paths"][i]) == (int(rec["score"]), 4096, int(rec["ref_to"]))
    assert res["stats"]["waves_per_block"] == 2 and res["stats"]["n_cells"] == 2 * 4096 * 4096


def test_forced_long_gap_at_the_largest_gap_cost(ctx):
    """gap_open = gap_extend = 1024 and a contig longer than every reference: L - R inserts are forced, and the undefined cells next to
    them hold values as far below the sentinel as the rule allows"""
    rng = np.random.default_rng(52)
    base = random_seq(rng, 70)
    refs = [variant(rng, base, 40), variant(rng, base, 66), b"A"]
    seqs = [variant(rng, base, 200), variant(rng, base, 130), variant(rng, base, 67)]
    sub = nr.match_mismatch(127, -127)
    res, near = assert_is(ctx, seqs, refs, sub, 1024, 1024, what="forced inserts")
    assert near[0][1]["n_insert"] >= 200 - 66 and near[0][1]["score"] <= -1024 * (200 - 66) + 127 * 66
    res, near = assert_is(ctx, seqs, refs, sub, 1024, 0, what="forced inserts, free extension")
    assert near[0][1]["n_insert"] >= 200 - 66
    # a long delete that pays: the contig is the two ends of a reference
    p = random_seq(rng, 300)
    res, near = assert_is(ctx, [p[:40] + p[-40:]], [p, p[:200]], sub, 1024, 1, what="long delete")
    assert near[0][0] == 0 and near[0][1]["n_delete"] == 220 and near[0][1]["score"] == 80 * 127 - 1024 - 219


# ---- 6. bytes ------------------------------------------------------------------------------------------------------------------------
def test_bytes(ctx):
    rng = np.random.default_rng(61)
    sub = mm()
    sub[0, 0] = 9                                                         # class 0 against class 0 scores well and is never identical
    sub[0, 1:] = sub[1:, 0] = -6
    p = random_seq(rng, 70)
    refs = [p, p.lower(), bytes(p[:20]) + b"*-\x80\xff." + bytes(p[25:])]
    seqs = [p.lower(), p[:30] + p[30:].lower(), bytes(p[:20]) + b"-*\xc1\xe9@" + bytes(p[25:]), b"*" * 10, b"[`{\x00\x7f"]
    res, near = assert_is(ctx, seqs, refs, sub, 6, 1, what="bytes")
    assert res["scores"][0].tolist()[:2] == [350, 350] and near[0][0] == 0 and near[0][1]["n_ident"] == 70            # lower case equals upper case
    assert near[2][0] == 2 and near[2][1]["score"] == 65 * 5 + 5 * 9 and near[2][1]["n_match"] == 70 and near[2][1]["n_ident"] == 65
    assert near[3][1]["n_ident"] == 0 and near[4][1]["n_ident"] == 0 and near[4][0] == 2 and near[4][1]["score"] == 45
    # the same bytes in upper case: the same numbers
    up = ctx.nearest([s.upper() for s in seqs[:2]], [r.upper() for r in refs], sub, 6, 1, scores=True)
    assert np.array_equal(up["scores"], res["scores"][:2]) and np.array_equal(up["recs"], res["recs"][:2])


# ---- 7. the batch switch -------------------------------------------------------------------------------------------------------------
def test_batch_switch_moves_no_output(ctx):
    rng = np.random.default_rng(71)
    base = random_seq(rng, 120)
    refs = [variant(rng, base, int(n)) for n in rng.integers(60, 120, 9)]
    seqs = [variant(rng, base, int(n)) for n in rng.integers(20, 90, 23)] + [b"", b"*"]
    try:
        ctx.set_nearest_batch(0)
        want = ctx.nearest(seqs, refs, mm(), 7, 2, scores=True, paths=True)
        assert want["stats"]["n_batches"] == 1
        n_aligned = len(seqs) - want["stats"]["n_unaligned"]
        seen = set()
        for cells in (1, 20000, 7 * 90 * 120):
            ctx.set_nearest_batch(cells)
            for scores in (True, False):
                got = ctx.nearest(seqs, refs, mm(), 7, 2, scores=scores, paths=True)
                assert np.array_equal(got["recs"], want["recs"]) and got["paths"] == want["paths"], (cells, scores)
                assert not scores or np.array_equal(got["scores"], want["scores"])
                for f in ("n_unaligned", "n_cells", "n_trace_cells"):
                    assert got["stats"][f] == want["stats"][f]
            seen.add(got["stats"]["n_batches"])
            if cells == 1:
                assert got["stats"]["n_batches"] == n_aligned             # a batch always holds one pair
            else:
                assert 1 < got["stats"]["n_batches"] < n_aligned
        assert len(seen) == 3
    finally:
        ctx.set_nearest_batch(0)
    # the yardstick on a part of it (the whole is compared above, batch against batch)
    assert_is(ctx, seqs[:4] + seqs[-2:], refs[:3], mm(), 7, 2, what="batches")


# ---- 8. guards -----------------------------------------------------------------------------------------------------------------------
def test_guards(ctx):
    import ctypes as C
    L = ctx._L
    seqs, refs = b"ACDEACD", b"ACDEKACD"
    off, roff = np.array([0, 4, 7], dtype=np.uint64), np.array([0, 5, 8], dtype=np.uint64)
    sub = mm()
    recs = np.full(2 * 9, 77, dtype=np.int32)
    scores = np.full(4, 77, dtype=np.int32)
    path = np.full(7 + 2 * 4096, 77, dtype=np.uint8)
    plen = np.full(2, 77, dtype=np.int32)
    stats = np.full(15, 77, dtype=np.int64)

    def call(seqs_p=seqs, off_p=off.ctypes.data, n=2, refs_p=refs, roff_p=roff.ctypes.data, n_ref=2, sub_p=sub.ctypes.data, go=6, ge=1, recs_p=recs.ctypes.data,
             path_p=path.ctypes.data, plen_p=plen.ctypes.data, h=None):
        return L.mgta_seqs_nearest(ctx.h if h is None else h[0], seqs_p, off_p, n, refs_p, roff_p, n_ref, sub_p, go, ge, recs_p, scores.ctypes.data, path_p, plen_p,
                                   stats.ctypes.data)

    def refused(word, **kw):
        assert call(**kw) == -1 and word in L.mgta_last_error(), (kw, L.mgta_last_error())

    refused(b"ctx", h=(None,))
    refused(b"n = -1", n=-1)
    refused(b"n_ref = -1", n_ref=-1)
    refused(b"offsets", off_p=None)
    refused(b"ref_offsets", roff_p=None)
    refused(b"recs", recs_p=None)
    refused(b"sub", sub_p=None)
    refused(b"seqs", seqs_p=None)
    refused(b"refs", refs_p=None)
    refused(b"path_len", plen_p=None)
    for go, ge in ((6, 7), (6, -1), (1025, 1), (-1, -1)):
        refused(b"gap_open", go=go, ge=ge)
    down = np.array([0, 5, 4], dtype=np.uint64)
    refused(b"ascend", off_p=down.ctypes.data)
    refused(b"ascend", roff_p=down.ctypes.data)
    long_off = np.array([0, 4097, 4098], dtype=np.uint64)
    refused(b"4096 residues per contig", off_p=long_off.ctypes.data)
    refused(b"4096 residues per reference", roff_p=long_off.ctypes.data)
    many = np.arange(0, (2 ** 19 + 1) * 4096, 4096, dtype=np.uint64)       # 2^19 references of 4096 residues: 2^31 columns
    refused(b"2^31 residues", roff_p=many.ctypes.data, n_ref=many.size - 1)
    refused(b"2^31 contigs", n=2 ** 31)
    refused(b"2^31 references", n_ref=2 ** 31)
    assert L.mgta_ctx_set_nearest_batch(ctx.h, -1) == -1 and b"cells" in L.mgta_last_error()
    assert L.mgta_ctx_set_nearest_batch(None, 7) == -1 and b"ctx" in L.mgta_last_error()
    # nothing was written by the refused calls
    assert (recs == 77).all() and (scores == 77).all() and (path == 77).all() and (plen == 77).all() and (stats == 77).all()
    # the same arguments with everything in place: a valid call
    assert call() == 0
    want_scores, near = restate_nearest([seqs[:4], seqs[4:]], [refs[:5], refs[5:]], sub, 6, 1)
    assert scores.reshape(2, 2).tolist() == [[NO_SCORE if v is None else v for v in row] for row in want_scores]
    assert recs.reshape(2, 9)[:, 1].tolist() == [t[0] for t in near] and plen.tolist() == [len(t[1]["path"]) for t in near]
    assert path[:4].tobytes() == b"MMMM" and path[4 + 4096:4 + 4096 + plen[1]].tobytes().decode() == near[1][1]["path"]
    assert stats[0] == 2 and stats[1] == 2 and stats[2] == 4
    # n = 0: MGTA_OK, stats all zero, whatever else is NULL
    assert L.mgta_seqs_nearest(ctx.h, None, None, 0, None, None, 0, None, 6, 1, None, None, None, None, stats.ctypes.data) == 0 and (stats[:13] == 0).all()


# ---- 9. files: one process per call and the worker -----------------------------------------------------------------------------------
MATRIX = """# four letters and the rest
   A  C  D  E  K  *
A  4 -1 -2 -1 -1 -4
C -1  6 -3 -2 -3 -4
D -2 -3  5  2 -1 -4
E -1 -2  2  5  1 -4
K -1 -3 -1  1  4 -4
* -4 -4 -4 -4 -4  1
"""


def fasta_case(seed):
    rng = np.random.default_rng(seed)
    base = random_seq(rng, 110)
    ref_names = [f"ref{j}" for j in range(7)]
    ref_lines = []
    for j in range(7):
        s = variant(rng, base, int(rng.integers(70, 110))).decode()
        at = int(rng.integers(5, 60))
        ref_lines.append(s[:at].lower() + "--." + s[at:at + 30] + "\n" + s[at + 30:] + "*")      # an alignment, on two lines
    seqs = [variant(rng, base, int(n)).decode() for n in rng.integers(25, 80, 40)] + ["", "AC*E"]
    headers = [f"c{j} len={len(s)}" if j % 3 else f"c{j}" for j, s in enumerate(seqs)]
    return headers, seqs, ref_names, ref_lines


def test_one_shot_and_worker_write_the_same_files(ctx, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    (tmp_path / "m.txt").write_text(MATRIX)
    cases = [fasta_case(4), fasta_case(5)]
    scoring = ["5,-4", str(tmp_path / "m.txt")]
    for i, (headers, seqs, ref_names, ref_lines) in enumerate(cases):
        open(tmp_path / f"p{i}.fa", "w").write("".join(f">{h}\n{s}\n" for h, s in zip(headers, seqs)))
        open(tmp_path / f"r{i}.faa", "w").write("".join(f">{h} some words\n{s}\n" for h, s in zip(ref_names, ref_lines)))
        subprocess.run([BIN, "nearest", str(tmp_path / f"r{i}.faa"), str(tmp_path / f"p{i}.fa"), str(tmp_path / f"one{i}"), "7", "2", scoring[i]],
                       check=True, capture_output=True, timeout=120)
    req = "".join(f"nearest\t{tmp_path}/r{i}.faa\t{tmp_path}/p{i}.fa\t{tmp_path}/w{i}\t7\t2\t{scoring[i]}\n" for i in range(2)) + "quit\n"
    r = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0", "DONE", "0"], r.stderr[-2000:]
    for i, (headers, seqs, ref_names, ref_lines) in enumerate(cases):
        names, ref_seqs = nr.read_refs(str(tmp_path / f"r{i}.faa"))
        assert names == ref_names and ref_seqs == [s.replace("-", "").replace(".", "").replace("*", "").replace("\n", "").upper() for s in ref_lines]
        sub = nr.parse_scoring(scoring[i])
        res = ctx.nearest(seqs, ref_seqs, sub, 7, 2)
        assert res["stats"]["n_unaligned"] == 1 and len(set(res["recs"]["ref"].tolist())) > 2
        nr.write_nearest(str(tmp_path / f"py{i}"), headers, seqs, names, ref_seqs, res)
        for tail in ("_nearest.txt", "_nearest_refs.txt"):
            text = open(f"{tmp_path}/py{i}{tail}").read()
            assert open(f"{tmp_path}/one{i}{tail}").read() == open(f"{tmp_path}/w{i}{tail}").read() == text and len(text) > 0, (i, tail)
        back = nr.read_nearest(f"{tmp_path}/one{i}_nearest.txt")
        first = nr.ref_index(names)
        assert [(-1 if x is None else first[x]) for x in back["ref_names"]] == res["recs"]["ref"].tolist()
        for f in nr.REC.names:
            assert f == "ref" or np.array_equal(back["recs"][f], res["recs"][f]), f
        table = nr.read_refs_table(f"{tmp_path}/one{i}_nearest_refs.txt")
        assert table["names"] == names and table["contigs"].sum() == len(seqs) - 1
        # a few records against the yardstick, the matrix's scores included
        _, near = restate_nearest([s.encode() for s in seqs[:3] + seqs[-2:]], [s.encode() for s in ref_seqs], sub, 7, 2)
        for j, t in zip((0, 1, 2, len(seqs) - 2, len(seqs) - 1), near):
            rec = res["recs"][j]
            assert (t is None and rec["status"] == 1) or (int(rec["ref"]), int(rec["score"]), int(rec["n_ident"])) == (t[0], t[1]["score"], t[1]["n_ident"]), j
    # a gap cost out of range, a matrix with a value outside int8: the step fails and leaves nothing
    (tmp_path / "bad.txt").write_text(MATRIX.replace(" 6 ", " 200 "))
    for j, tail in enumerate((["7", "8", "5,-4"], ["7", "2", str(tmp_path / "bad.txt")])):
        r = subprocess.run([BIN, "nearest", str(tmp_path / "r0.faa"), str(tmp_path / "p0.fa"), str(tmp_path / f"bad{j}")] + tail, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "nearest" in r.stderr
    assert [f for f in os.listdir(tmp_path) if f.startswith("bad") and f != "bad.txt"] == []


# ---- 10. driver end to end -----------------------------------------------------------------------------------------------------------
def check_driver_files(prefix, ref_path, scoring, go, ge):
    """PREFIX.fasta, PREFIX_nearest.txt and PREFIX_nearest_refs.txt: the files parse, and every record's line is what `restate` gives on the
    file's sequences"""
    with open(prefix + ".fasta", encoding="latin-1") as fh:
        records = nr.parse_fasta(fh.read())
    names, ref_seqs = nr.read_refs(ref_path)
    table = nr.read_nearest(prefix + "_nearest.txt")
    n = len(records)
    assert n > 0 and table["names"] == [nr.record_name(h) for h, _ in records] and table["lens"].tolist() == [len(s) for _, s in records]
    sub = nr.parse_scoring(scoring)
    seqs, refs = [s.encode("latin-1") for _, s in records], [s.encode() for s in ref_seqs]
    _, near = restate_nearest(seqs, refs, sub, go, ge)
    recs = np.zeros(n, dtype=nr.REC)
    for i, t in enumerate(near):
        recs[i] = (1, -1, 0, 0, 0, 0, 0, 0, 0) if t is None else (0, t[0], t[1]["score"], t[1]["ref_from"], t[1]["ref_to"], t[1]["n_match"], t[1]["n_ident"],
                                                                t[1]["n_insert"], t[1]["n_delete"])
    ref_lens = [len(s) for s in ref_seqs]
    assert open(prefix + "_nearest.txt", encoding="latin-1").read() == nr.nearest_text(table["names"], table["lens"], names, ref_lens, recs)
    assert open(prefix + "_nearest_refs.txt", encoding="latin-1").read() == nr.refs_text(names, ref_lens, recs)
    assert nr.read_refs_table(prefix + "_nearest_refs.txt")["contigs"].sum() == int((recs["status"] == 0).sum())
    return n


def test_driver_nearest_end_to_end(golden_dir, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    mg = synth.make_metagenome(6000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)    # the sample of test_driver_cluster_end_to_end
    synth.write_fasta(mg.reads, str(tmp_path / "reads.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "45", "-t", "4", "--min-contig-len", "150"]

    def nearest_files(out):
        return sorted(f for _, _, files in os.walk(out) for f in files if "_nearest" in f)

    # without the flag: no file of the step, and the checkpoints of a run without flags
    out = tmp_path / "out"
    r = subprocess.run(base + ["-o", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
    assert nearest_files(out) == [] and open(out / "tmp" / "cp.txt").read().splitlines() == [f"{i}\tdone" for i in range(6)]
    assert "nearest reference" not in open(out / "log").read()
    # the flag alone: the step reads every protein contig, and its checkpoint is the last
    out1 = tmp_path / "out1"
    r = subprocess.run(base + ["-o", str(out1), "--nearest"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out1 / "log").read()[-2000:]
    d = out1 / "contigs" / "rplB"
    assert nearest_files(out1) == ["prot_merged_nearest.txt", "prot_merged_nearest_refs.txt"]
    n_all = check_driver_files(str(d / "prot_merged"), f"{toy}/ref_aligned.faa", "5,-4", 10, 1)
    assert open(d / "prot_merged.fasta").read() == open(out / "contigs" / "rplB" / "prot_merged.fasta").read()      # the run is what it was
    assert open(out1 / "tmp" / "cp.txt").read().splitlines() == [f"{i}\tdone" for i in range(6 + 1)]
    log = open(out1 / "log").read()
    assert log.count("Finding the nearest reference of the contigs of rplB") == 1 and log.count("Searching contigs") == 1
    # with --derep, --align and --cluster, and parameters of its own: the step reads the representatives, and its checkpoint is the last
    out2 = tmp_path / "out2"
    r = subprocess.run(base + ["-o", str(out2), "--derep", "--align", "--cluster", "--nearest", "--nearest-scoring", "3,-2", "--nearest-gap-open", "5",
                               "--nearest-gap-extend", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out2 / "log").read()[-2000:]
    d = out2 / "contigs" / "rplB"
    assert nearest_files(out2) == ["prot_merged_rmdup_rep_seqs_nearest.txt", "prot_merged_rmdup_rep_seqs_nearest_refs.txt"]
    n_rep = check_driver_files(str(d / "prot_merged_rmdup_rep_seqs"), f"{toy}/ref_aligned.faa", "3,-2", 5, 2)
    assert 0 < n_rep <= n_all
    # the checkpoints: six of a run without flags, then derep, align, cluster, nearest (one gene each)
    assert open(out2 / "tmp" / "cp.txt").read().splitlines() == [f"{i}\tdone" for i in range(6 + 4)]
    log = open(out2 / "log").read()
    assert log.index("Clustering the aligned contigs") < log.index("Finding the nearest reference")
    print(f"driver: {n_all} contigs, {n_rep} representatives")
