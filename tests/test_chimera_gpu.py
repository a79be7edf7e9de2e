"""mgta_seqs_chimera on the device against `restate_chimera`, the rule of include/megagta_hip.h written out in Python:
the recurrence of 2l in nested loops over Python ints, None for undefined, every tie rule spelled out.  Every comparison is exact: the
top two of every row through `tops`, every field of every record, the files byte for byte.  `uchime` is not available; the rule is this
project's own and is not checked against it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from megagta_amd import chimera as ch
from megagta_amd import nearest as nr
from megagta_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
ABSENT = (-2 ** 31, -1)
gpu = pytest.mark.gpu


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------
def cls(b: int) -> int:
    if 65 <= b <= 90:
        return b - 64
    if 97 <= b <= 122:
        return b - 96
    return 0


def row_maxima(x: bytes, y: bytes, sub, go: int, ge: int) -> list:
    """[max_j M[i][j] for i = 1 .. L] of 2l's recurrence, None where no M[i][j] is defined: entry b - 1 is score(x[1..b], y), because
    the table of a prefix is the first rows of the table of the whole"""
    L, R = len(x), len(y)
    S = [[int(v) for v in row] for row in sub]
    cx, cy = [cls(b) for b in x], [cls(b) for b in y]
    out = []
    Mp = Xp = Yp = [None] * (R + 1)
    for i in range(1, L + 1):
        Mi, Xi, Yi, Si = [None] * (R + 1), [None] * (R + 1), [None] * (R + 1), S[cx[i - 1]]
        for j in range(1, R + 1):
            v = None
            if i == 1:
                v = 0
            elif j > 1:
                for c in (Mp[j - 1], Xp[j - 1], Yp[j - 1]):
                    if c is not None and (v is None or c > v):
                        v = c
            if v is not None:
                Mi[j] = Si[cy[j - 1]] + v
            if i > 1:
                v = None
                if Mp[j] is not None:
                    v = Mp[j] - go
                if Xp[j] is not None and (v is None or Xp[j] - ge > v):
                    v = Xp[j] - ge
                Xi[j] = v
            if j > 1:
                v = None
                if Mi[j - 1] is not None:
                    v = Mi[j - 1] - go
                if Yi[j - 1] is not None and (v is None or Yi[j - 1] - ge > v):
                    v = Yi[j - 1] - ge
                Yi[j] = v
        defined = [m for m in Mi[1:] if m is not None]
        out.append(max(defined) if defined else None)
        Mp, Xp, Yp = Mi, Xi, Yi
    return out


def score(x: bytes, y: bytes, sub, go, ge):
    """2l's score(x, y), or None"""
    return row_maxima(x, y, sub, go, ge)[-1] if len(x) and len(y) else None


def prefix_scores(x, y, sub, go, ge, rows=row_maxima) -> list:
    """P_r(b) for b = 1 .. L"""
    return rows(x, y, sub, go, ge) if len(y) else [None] * len(x)


def suffix_scores_literal(x, y, sub, go, ge, rows=row_maxima) -> list:
    """S_r(b) for b = 1 .. L, every suffix scored on its own"""
    return [rows(x[b - 1:], y, sub, go, ge)[-1] if len(y) else None for b in range(1, len(x) + 1)]


def suffix_scores_by_reversal(x, y, sub, go, ge, rows=row_maxima) -> list:
    """S_r(b) as the prefix score of the reversed contig against the reversed reference (tests/test_chimera_host.py ties it to the
    literal one, an asymmetric sub included)"""
    return prefix_scores(x[::-1], y[::-1], sub, go, ge, rows)[::-1]


def top_two(values) -> tuple:
    """values[r] or None -> ((score, r) of the highest, the lowest r on a tie; the same among the others), ABSENT where there is none"""
    first = second = None
    for r, v in enumerate(values):
        if v is not None and (first is None or v > values[first]):
            first = r
    for r, v in enumerate(values):
        if v is not None and r != first and (second is None or v > values[second]):
            second = r
    return (ABSENT if first is None else (values[first], first)), (ABSENT if second is None else (values[second], second))


def verdict(L, P, S, min_seg, min_gain):
    """steps 1 to 5 for one contig of L residues from P[r][b - 1] = P_r(b) and S[r][b - 1] = S_r(b) -> (the record as a tuple, tops as
    [L][8])"""
    n_ref = len(P)
    tops = []
    for b in range(1, L + 1):
        p1, p2 = top_two([P[r][b - 1] for r in range(n_ref)])
        s1, s2 = top_two([S[r][b - 1] for r in range(n_ref)])
        tops.append(p1 + p2 + s1 + s2)
    if L == 0:
        return ch.UNCHECKED, tops
    N = tops[L - 1][1]
    ref, sc = (N, tops[L - 1][0]) if N >= 0 else (-1, 0)
    best = None                                                          # (b, left ref, left score, right ref, right score)
    for b in range(min_seg, L - min_seg + 1):
        p1, p1r, p2, p2r = tops[b - 1][:4]
        s1, s1r, s2, s2r = tops[b][4:]                                    # the suffix that starts at b + 1
        pair = None
        if p1r >= 0 and s1r >= 0:
            if p1r != s1r:
                pair = (p1r, p1, s1r, s1)
            else:
                cands = []
                if s2r >= 0:
                    cands.append((p1r, p1, s2r, s2))
                if p2r >= 0:
                    cands.append((p2r, p2, s1r, s1))
                for c in cands:
                    if pair is None or c[1] + c[3] > pair[1] + pair[3]:   # the first wins a tie
                        pair = c
        if pair is not None and (best is None or pair[1] + pair[3] > best[2] + best[4]):   # the lowest b wins a tie
            best = (b,) + pair
    if best is None:
        return (2, ref, sc, 0, -1, 0, -1, 0, 0, 0, 0), tops
    b_star, A, a_score, B, b_score = best
    assert A != B
    two = a_score + b_score
    terms = [sc] if N >= 0 else []
    for r in {N, A, B} - {-1}:
        for b in range(min_seg, L - min_seg + 1):
            if P[r][b - 1] is not None and S[r][b] is not None:
                terms.append(P[r][b - 1] + S[r][b])
    one = max(terms)
    gain = two - one
    return (1 if gain >= min_gain else 0, ref, sc, b_star, A, a_score, B, b_score, two, one, gain), tops


def restate_chimera(seqs, refs, sub, go, ge, min_seg, min_gain, literal=False, rows=row_maxima):
    """-> (records as tuples, tops as a list of [L][8]); literal: every suffix scored on its own (small inputs), else by reversal; rows:
    the loops, or row_maxima_by_diagonals where they would take too long"""
    suffix = suffix_scores_literal if literal else suffix_scores_by_reversal
    recs, tops = [], []
    for x in seqs:
        P = [prefix_scores(x, y, sub, go, ge, rows) for y in refs]
        S = [suffix(x, y, sub, go, ge, rows) for y in refs]
        rec, t = verdict(len(x), P, S, min_seg, min_gain)
        recs.append(rec)
        tops.append(t)
    return recs, tops


def row_maxima_by_diagonals(x: bytes, y: bytes, sub, go: int, ge: int) -> list:
    """row_maxima of the same rule, one numpy step per anti-diagonal in int64 with a sentinel far below every value (for the sizes where
    the loops would take minutes; test_diagonals_agree_with_the_loops ties it to them)"""
    L, R = len(x), len(y)
    NEG = -(1 << 50)
    S = np.asarray(sub, dtype=np.int64)
    cx, cy = np.array([cls(b) for b in x]), np.array([cls(b) for b in y])
    new = lambda: np.full(L + 1, NEG, dtype=np.int64)                    # indexed by the row; a diagonal holds the cells with i + j = d
    M1, X1, Y1, D2 = new(), new(), new(), new()
    best = new()
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
        best = np.maximum(best, Md)
        D2 = np.maximum(np.maximum(M1, X1), Y1)
        M1, X1, Y1 = Md, Xd, Yd
    return [None if v < NEG // 2 else int(v) for v in best[1:]]


def mm(match=5, mismatch=-4):
    return nr.match_mismatch(match, mismatch)


def assert_is(ctx, seqs, refs, sub, go, ge, min_seg, min_gain, what="", literal=False, want=None):
    """tops and every record against the restatement; returns (result, wanted records)"""
    want_recs, want_tops = want if want is not None else restate_chimera(seqs, refs, sub, go, ge, min_seg, min_gain, literal=literal)
    res = ctx.chimera(seqs, refs, sub, go, ge, min_seg, min_gain, tops=True)
    assert len(res["tops"]) == len(seqs)
    for i, t in enumerate(want_tops):
        got = res["tops"][i]
        assert got.shape == (len(seqs[i]), 8)
        for b, row in enumerate(t):
            assert tuple(int(v) for v in got[b]) == tuple(row), (what, "tops", i, b + 1, got[b].tolist(), row)
    for i, w in enumerate(want_recs):
        assert tuple(int(v) for v in res["recs"][i]) == tuple(w), (what, "record", i, tuple(res["recs"][i]), w)
    st = res["stats"]
    assert st["n_seqs"] == len(seqs) and st["n_refs"] == len(refs)
    for k, name in enumerate(("n_clean", "n_chimeric", "n_unchecked")):
        assert st[name] == sum(w[0] == k for w in want_recs), (what, name)
    if sum(map(len, seqs)) and sum(map(len, refs)):
        assert st["n_cells"] == 2 * sum(map(len, seqs)) * sum(map(len, refs)) and st["lds_bytes"] == 27 * 32
    # the records do not depend on whether the top two are asked for
    plain = ctx.chimera(seqs, refs, sub, go, ge, min_seg, min_gain)
    assert np.array_equal(plain["recs"], res["recs"]) and "tops" not in plain, what
    return res, want_recs


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


def random_seq(rng, length: int, alphabet=ALPHABET) -> bytes:
    return bytes(alphabet[int(k)] for k in rng.integers(0, len(alphabet), length))


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


# ---- 0. the two restatements agree (no device) -----------------------------------------------------------------------------------------
def test_diagonals_agree_with_the_loops():
    rng = np.random.default_rng(7)
    sub = mm()
    sub[0, :] = sub[:, 0] = -2
    for trial in range(60):
        L, R = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        x, y = random_seq(rng, L), random_seq(rng, R)
        go = int(rng.integers(0, 9))
        ge = int(rng.integers(0, go + 1))
        assert row_maxima_by_diagonals(x, y, sub, go, ge) == row_maxima(x, y, sub, go, ge), (trial, x, y, go, ge)
    assert row_maxima(b"ACD", b"A", sub, 3, 1) == [5, None, None] == row_maxima_by_diagonals(b"ACD", b"A", sub, 3, 1)


# ---- 1. row-strip edges --------------------------------------------------------------------------------------------------------------
REF_LENS = {1: (1, 63, 130), 2: (2, 64, 65, 1), 3: (130, 2, 63), 63: (64, 1, 65, 2, 63), 64: (63, 130, 64), 65: (65, 2, 64, 1),
            127: (130, 63, 1, 65), 128: (64, 2, 130), 129: (1, 65, 63, 130, 64)}


@gpu
@pytest.mark.parametrize("L", sorted(REF_LENS))
def test_row_strip_edges(ctx, L):
    rng = np.random.default_rng(1000 + L)
    base = random_seq(rng, 160)
    refs = [variant(rng, base, R) for R in REF_LENS[L]]
    assert 3 <= len(refs) <= 5
    longest = max(refs, key=len)
    seqs = [variant(rng, base, L), variant(rng, longest, L, subs=0.05, indels=0.03), (refs[0] + refs[-1] + longest)[:L]]
    min_seg = max(1, min(10, L // 3))
    assert_is(ctx, seqs, refs, mm(), 6, 1, min_seg, 15, what=f"L={L}")
    if L <= 3:
        assert_is(ctx, seqs, refs, mm(), 6, 1, 1, 1, what=f"L={L} literal", literal=True)


@gpu
def test_small_inputs_with_every_suffix_scored_on_its_own(ctx):
    rng = np.random.default_rng(12)
    sub = rng.integers(-6, 7, (27, 27)).astype(np.int8)                   # not symmetric
    base = random_seq(rng, 40)
    refs = [variant(rng, base, int(n)) for n in (18, 22, 1, 25, 2)]
    seqs = [variant(rng, base, int(n)) for n in (20, 24, 7, 2, 1)] + [refs[0][:10] + refs[3][-11:]]
    res, want = assert_is(ctx, seqs, refs, sub, 5, 2, 3, 4, what="literal", literal=True)
    assert restate_chimera(seqs, refs, sub, 5, 2, 3, 4) == restate_chimera(seqs, refs, sub, 5, 2, 3, 4, literal=True)


# ---- 2. reference boundaries on every lane of a step -----------------------------------------------------------------------------------
@gpu
def test_reference_boundaries_on_every_lane(ctx):
    """many references of 1 to 5 residues: a boundary passes every one of a step's 64 lanes at every phase, in one segment and cut"""
    rng = np.random.default_rng(21)
    refs = [random_seq(rng, 1 + k % 5) for k in range(105)]
    starts = np.cumsum([0] + [len(r) for r in refs])
    assert {int(s) % 64 for s in starts} == set(range(64))                # a boundary at every residue of a step's lanes
    seqs = [random_seq(rng, n) for n in (5, 9, 66, 130)] + [refs[7] + refs[8], refs[104]]
    res, want = assert_is(ctx, seqs, refs, mm(), 4, 1, 2, 3, what="boundaries")
    assert res["stats"]["n_unchecked"] < len(seqs)
    try:
        ctx.set_chimera_segment(1)
        cut, _ = assert_is(ctx, seqs, refs, mm(), 4, 1, 2, 3, what="boundaries, one reference per segment")
        assert cut["stats"]["n_segments"] == len(refs)
    finally:
        ctx.set_chimera_segment(0)


# ---- 3. undefined pairs --------------------------------------------------------------------------------------------------------------
@gpu
def test_undefined_pairs(ctx):
    sub = mm()
    seqs = [b"ACDEKACD", b"", b"A", b"CC", b"ACDEKKEDCA"]
    for refs in ([], [b"ACDEK"], [b"ACDEK", b"KEDCA"], [b"ACDEK", b"", b"KEDCA"], [b"", b""], [b"A", b"C"], [b"A", b"ACDEKACD", b"C"]):
        res, want = assert_is(ctx, seqs, refs, sub, 3, 1, 2, 1, what=f"undefined {refs}", literal=True)
        if sum(len(r) >= 2 for r in refs) < 2:
            assert [w[0] for w in want] == [2] * len(seqs)               # fewer than two references that score a half of two residues
        assert tuple(res["recs"][1]) == ch.UNCHECKED                      # the empty contig
    # one reference: unchecked, and the nearest reference is kept
    res, want = assert_is(ctx, seqs, [b"ACDEK"], sub, 3, 1, 2, 1, what="one reference", literal=True)
    assert tuple(res["recs"][0])[:3] == (2, 0, score(seqs[0], b"ACDEK", sub, 3, 1)) and tuple(res["recs"][0])[3:] == ch.UNCHECKED[3:]
    # R = 1 < L: no score for the whole contig, and with min_seg 1 the two residues of a contig still find two parents
    res, want = assert_is(ctx, [b"AC", b"ACD"], [b"A", b"C"], sub, 3, 1, 1, 1, what="R = 1", literal=True)
    assert tuple(res["recs"][0]) == (1, -1, 0, 1, 0, 5, 1, 5, 10, 1, 9) and tuple(res["recs"][1]) == ch.UNCHECKED
    # every contig empty; no contig at all
    res = ctx.chimera([b"", b""], [b"ACD"], sub, 3, 1, 2, 1, tops=True)
    assert [tuple(r) for r in res["recs"]] == [ch.UNCHECKED] * 2 and [t.shape for t in res["tops"]] == [(0, 8)] * 2
    res = ctx.chimera([], [b"ACD"], sub, 3, 1, 2, 1, tops=True)
    assert len(res["recs"]) == 0 and all(v == 0 for v in res["stats"].values())
    res = ctx.chimera([b"ACD"], [], sub, 3, 1, 1, 1, tops=True)
    assert tuple(res["recs"][0]) == ch.UNCHECKED and res["tops"][0].tolist() == [list(ABSENT) * 4] * 3


# ---- 4. min_seg ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_min_seg(ctx):
    rng = np.random.default_rng(41)
    base = random_seq(rng, 80)
    refs = [variant(rng, base, 70) for _ in range(4)]
    L = 40
    seqs = [refs[0][:20] + refs[2][30:50], variant(rng, refs[1], L, subs=0.03, indels=0.02), refs[3][5:24] + refs[1][40:61]]
    assert [len(s) for s in seqs] == [40, 40, 40]
    sub = mm()
    P = [[prefix_scores(x, y, sub, 6, 1) for y in refs] for x in seqs]
    S = [[suffix_scores_by_reversal(x, y, sub, 6, 1) for y in refs] for x in seqs]
    status = {}
    for min_seg in (1, L // 2, L // 2 + 1, L + 1):
        want = [verdict(L, P[i], S[i], min_seg, 15) for i in range(3)]
        res, w = assert_is(ctx, seqs, refs, sub, 6, 1, min_seg, 15, what=f"min_seg {min_seg}", want=([r for r, _ in want], [t for _, t in want]))
        status[min_seg] = [r[0] for r in w]
        for rec in res["recs"]:
            assert rec["status"] == 2 or min_seg <= rec["brk"] <= L - min_seg
    assert status[L // 2 + 1] == status[L + 1] == [2, 2, 2]               # no b in range
    assert status[1][0] == 1 and status[L // 2][0] == 1 and 2 not in status[1] + status[L // 2]
    assert res["recs"]["ref"].tolist() == [verdict(L, P[i], S[i], 1, 15)[0][1] for i in range(3)]       # unchecked keeps ref and score


# ---- 5. ties -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_ties(ctx):
    rng = np.random.default_rng(51)
    letters = b"ACDEFGHIKLMNPQRSTVWY"
    p, q = random_seq(rng, 30, letters), random_seq(rng, 30, letters)
    # duplicate references: the lowest index wins in P1 and S1, and P2 is the copy
    refs = [q, p, p, q]
    res, want = assert_is(ctx, [p[:24], p[:12] + q[12:24]], refs, mm(), 6, 1, 5, 15, what="duplicates")
    t = res["tops"][0]
    assert t[-1].tolist()[:4] == [120, 1, 120, 2] and t[0].tolist()[4:] == [120, 1, 120, 2]
    # the pair of a contig that is one reference: P1 = S1, the candidates (P1, S2) and (P2, S1) tie, the first wins
    rec = res["recs"][0]
    assert (rec["status"], rec["ref"], rec["left_ref"], rec["right_ref"], rec["gain"]) == (0, 1, 1, 2, 0)
    # equal two at several b: the lowest b wins.  The halves share the residues 10 .. 13, so every break among them scores the same
    z = random_seq(rng, 4, letters)
    a, b = random_seq(rng, 20, letters), random_seq(rng, 20, letters)
    refs = [a[:10] + z + a[14:], b[:10] + z + b[14:]]
    x = a[:10] + z + b[14:]
    res, want = assert_is(ctx, [x], refs, mm(), 6, 1, 3, 15, what="equal two")
    rec = res["recs"][0]
    assert (rec["status"], rec["brk"], rec["left_ref"], rec["right_ref"], rec["two"]) == (1, 10, 0, 1, 100)
    # everything ties: sub all zero, gaps free
    zero = np.zeros((27, 27), dtype=np.int8)
    seqs = [random_seq(rng, n) for n in (2, 5, 64, 70)]
    refs = [random_seq(rng, n) for n in (1, 3, 66, 64)]
    res, want = assert_is(ctx, seqs, refs, zero, 0, 0, 1, 1, what="all zero")
    assert [w[0] for w in want] == [0, 0, 0, 0] and res["recs"]["brk"].tolist() == [1, 1, 1, 1] and res["recs"]["gain"].tolist() == [0] * 4


# ---- 6. range ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("value,gap", [(127, 1024), (127, 0), (-128, 1024), (-128, 0)])
def test_range_at_the_limits(ctx, value, gap):
    """a constant sub at the ends of int8 with L = R = 4096, one contig against three references.  With a constant sub a score depends
    on the lengths alone, so one sweep by diagonals per reference length gives P and S of every reference (S by reversal, which leaves
    the lengths as they are)"""
    sub = np.full((27, 27), value, dtype=np.int8)
    rng = np.random.default_rng(61)
    x = random_seq(rng, 4096)
    refs = [random_seq(rng, 4096), random_seq(rng, 4095), random_seq(rng, 4096)]
    by_len = {R: row_maxima_by_diagonals(x, refs[0][:R], sub, gap, gap) for R in (4095, 4096)}
    P = [by_len[len(y)] for y in refs]
    S = [by_len[len(y)][::-1] for y in refs]
    rec, tops = verdict(4096, P, S, 10, 15)
    res = ctx.chimera([x], refs, sub, gap, gap, 10, 15, tops=True)
    print(f"range {value} {gap}: record {tuple(res['recs'][0])}, wanted {rec}")
    assert np.array_equal(res["tops"][0], np.array(tops, dtype=np.int32))
    assert tuple(int(v) for v in res["recs"][0]) == rec
    assert rec[2] == (value * 4096 if value > 0 or gap else P[0][-1]) and res["stats"]["bound_bytes"] > 0


@gpu
def test_range_is_tied_to_the_loops_at_small_size(ctx):
    """the construction of test_range_at_the_limits at a size where the loops run: by lengths alone, by diagonals, by the loops"""
    rng = np.random.default_rng(62)
    for value, gap in ((127, 1024), (127, 0), (-128, 1024), (-128, 0)):
        sub = np.full((27, 27), value, dtype=np.int8)
        x = random_seq(rng, 70)
        refs = [random_seq(rng, 70), random_seq(rng, 69), random_seq(rng, 70)]
        by_len = {R: row_maxima_by_diagonals(x, refs[0][:R], sub, gap, gap) for R in (69, 70)}
        rec, tops = verdict(70, [by_len[len(y)] for y in refs], [by_len[len(y)][::-1] for y in refs], 10, 15)
        want = restate_chimera([x], refs, sub, gap, gap, 10, 15)
        assert want == ([rec], [tops]), (value, gap)
        assert_is(ctx, [x], refs, sub, gap, gap, 10, 15, what=f"range small {value} {gap}", want=want)


# ---- 7. the segment switch -----------------------------------------------------------------------------------------------------------
@gpu
def test_segment_switch_moves_no_output(ctx):
    rng = np.random.default_rng(71)
    base = random_seq(rng, 120)
    refs = [variant(rng, base, int(n)) for n in rng.integers(60, 120, 9)] + [b""]
    seqs = [variant(rng, base, int(n)) for n in rng.integers(20, 90, 12)] + [b"", b"*", refs[2][:40] + refs[6][-45:], variant(rng, base, 140)]
    try:
        ctx.set_chimera_segment(0)
        want = ctx.chimera(seqs, refs, mm(), 7, 2, 10, 15, tops=True)
        assert want["stats"]["n_segments"] == 1
        for columns in (1, 200):
            ctx.set_chimera_segment(columns)
            got = ctx.chimera(seqs, refs, mm(), 7, 2, 10, 15, tops=True)
            assert np.array_equal(got["recs"], want["recs"]), columns
            assert all(np.array_equal(a, b) for a, b in zip(got["tops"], want["tops"])), columns
            assert (got["stats"]["n_segments"] == 9 if columns == 1 else 1 < got["stats"]["n_segments"] < 9) and got["stats"]["n_groups"] > 1
    finally:
        ctx.set_chimera_segment(0)
    assert (want["recs"]["status"] == 1).sum() >= 1
    # the yardstick on a part of it (the whole is compared above, segment against segment)
    assert_is(ctx, seqs[:3] + seqs[-4:], refs, mm(), 7, 2, 10, 15, what="segments")


@gpu
def test_items_that_hold_several_segments(ctx):
    """what every input with many contigs and more than one segment of references takes: one work item walks several segments, carries
    a row's top two from one to the next through device memory, restarts its reference counter at each and uses the boundary buffer
    again.  set_chimera_groups forces it on an input a restatement can follow, whatever the device's size"""
    rng = np.random.default_rng(72)
    base = random_seq(rng, 150)
    refs = [variant(rng, base, int(n)) for n in rng.integers(60, 120, 4)] + [b""] + [variant(rng, base, int(n)) for n in rng.integers(60, 120, 5)]
    refs[7] = refs[1]                                                     # a tie across two segments: the lower index keeps it
    seqs = ([variant(rng, base, int(n)) for n in rng.integers(20, 64, 8)] + [variant(rng, base, int(n)) for n in (65, 70, 128, 129, 140)] +
            [b"", b"*", refs[2][:40] + refs[6][-45:], refs[8][:70] + refs[0][-60:], refs[1][5:60]])
    try:
        ctx.set_chimera_segment(0)
        ctx.set_chimera_groups(0)
        want = ctx.chimera(seqs, refs, mm(), 7, 2, 10, 15, tops=True)
        assert want["stats"]["n_segments"] == 1 and want["stats"]["n_groups"] == 1 and want["stats"]["bound_bytes"] > 0
        for columns, groups, n_seg, n_groups in ((1, 1, 9, 1), (1, 2, 9, 2), (1, 4, 9, 3), (200, 1, None, 1), (1, 100, 9, 9)):
            ctx.set_chimera_segment(columns)
            ctx.set_chimera_groups(groups)
            got = ctx.chimera(seqs, refs, mm(), 7, 2, 10, 15, tops=True)
            st = got["stats"]
            assert np.array_equal(got["recs"], want["recs"]), (columns, groups)
            assert all(np.array_equal(a, b) for a, b in zip(got["tops"], want["tops"])), (columns, groups)
            assert st["n_groups"] == n_groups and (st["n_segments"] == n_seg if n_seg else 1 < st["n_segments"] < 9), (columns, groups, st)
            assert st["n_items"] == 2 * len(seqs) * n_groups
            assert groups == 100 or 1 <= st["n_groups"] < st["n_segments"]                       # several segments in one item
        # the yardstick, with every item walking all nine segments
        ctx.set_chimera_segment(1)
        ctx.set_chimera_groups(1)
        some = [0, 3, 9, 11, 12, 13, 14, 15, 16, 17]
        res, w = assert_is(ctx, [seqs[i] for i in some], refs, mm(), 7, 2, 10, 15, what="several segments in one item")
        assert res["stats"]["n_segments"] == 9 and res["stats"]["n_groups"] == 1
        assert [r[0] for r in w][-3:-1] == [1, 1] and res["tops"][-1][-1].tolist()[:4] == [275, 1, 275, 7]
        # and the same path taken without the switch for groups: contigs enough that the library itself gives an item several segments
        ctx.set_chimera_groups(0)
        many = [variant(rng, base, int(n)) for n in rng.integers(20, 40, 1500)] + seqs
        ctx.set_chimera_segment(0)
        whole = ctx.chimera(many, refs, mm(), 7, 2, 10, 15, tops=True)
        ctx.set_chimera_segment(1)
        cut = ctx.chimera(many, refs, mm(), 7, 2, 10, 15, tops=True)
        print("many contigs:", {k: cut["stats"][k] for k in ("n_segments", "n_groups", "n_items", "grid_blocks")})
        assert np.array_equal(cut["recs"], whole["recs"]) and all(np.array_equal(a, b) for a, b in zip(cut["tops"], whole["tops"]))
        assert np.array_equal(cut["recs"][-len(seqs):], want["recs"]) and cut["stats"]["n_segments"] == 9
    finally:
        ctx.set_chimera_segment(0)
        ctx.set_chimera_groups(0)


# ---- 8. agreement with nearest -------------------------------------------------------------------------------------------------------
@gpu
def test_ref_and_score_are_those_of_nearest(ctx):
    rng = np.random.default_rng(81)
    base = random_seq(rng, 150)
    refs = [variant(rng, base, int(n)) for n in rng.integers(90, 150, 12)] + [b"A", b""]
    seqs = [variant(rng, base, int(n)) for n in rng.integers(1, 140, 40)] + [b"", b"AC"]
    got = ctx.chimera(seqs, refs, mm(), 10, 1, 10, 15)
    near = ctx.nearest(seqs, refs, mm(), 10, 1)
    assert np.array_equal(got["recs"]["ref"], near["recs"]["ref"]) and np.array_equal(got["recs"]["score"], near["recs"]["score"])
    assert (near["recs"]["status"] == 1).sum() >= 1 and len(set(near["recs"]["ref"].tolist())) > 3


# ---- 9. planted cases ----------------------------------------------------------------------------------------------------------------
AMINO = b"ACDEFGHIKLMNPQRSTVWY"


def planted(seed=5):
    """six references at 15 % divergence from one ancestor of 120 residues; contigs of 45 + 45 residues of two references with and
    without 3 % noise (the parents are known), and pieces of one reference: clean, 5 % noise, a 12-residue deletion, an 8-residue
    insertion"""
    rng = np.random.default_rng(seed)

    def noisy(s, rate):
        return bytes(AMINO[int(rng.integers(20))] if rng.random() < rate else c for c in s)

    ancestor = random_seq(rng, 120, AMINO)
    refs = [noisy(ancestor, 0.15) for _ in range(6)]
    chimeras, parents, clean = [], [], []
    for a, b in ((0, 1), (4, 3)):
        for rate in (0.0, 0.03):
            at = int(rng.integers(10, 20))
            chimeras.append(noisy(refs[a][at:at + 45] + refs[b][at + 45:at + 90], rate))
            parents.append((a, b))
    for r in (5,):
        piece = refs[r][12:102]
        clean += [piece, noisy(piece, 0.05), piece[:40] + piece[52:], piece[:45] + random_seq(rng, 8, AMINO) + piece[45:]]
    return refs, chimeras, parents, clean


@gpu
def test_planted_cases(ctx):
    refs, chimeras, parents, clean = planted()
    seqs = chimeras + clean
    res, want = assert_is(ctx, seqs, refs, mm(), 10, 1, 10, 15, what="planted")
    n = len(chimeras)
    recs = res["recs"]
    print("planted: gains of the chimeras", recs["gain"][:n].tolist(), "of the clean contigs", recs["gain"][n:].tolist())
    assert recs["status"][:n].tolist() == [1] * n and recs["status"][n:].tolist() == [0] * len(clean)
    assert list(zip(recs["left_ref"][:n].tolist(), recs["right_ref"][:n].tolist())) == parents
    assert all(35 <= b <= 55 for b in recs["brk"][:n].tolist())


# ---- 10. files: one process per call and the worker ----------------------------------------------------------------------------------
@gpu
def test_one_shot_and_worker_write_the_same_files(ctx, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    refs, chimeras, parents, clean = planted(6)
    seqs = [s.decode() for s in chimeras[:3] + clean] + ["", "AC*E"] + [chimeras[3].decode().lower()]
    headers = [f"c{j} len={len(s)}" if j % 3 else f"c{j}" for j, s in enumerate(seqs)]
    nucl = ["ACGT" * (j + 1) for j in range(len(seqs))]
    ref_names = [f"ref{j}" for j in range(len(refs))]
    open(tmp_path / "p.fa", "w").write("".join(f">{h}\n{s}\n" for h, s in zip(headers, seqs)))
    open(tmp_path / "n.fa", "w").write("".join(f">{h} nucl\n{s}\n" for h, s in zip(headers, nucl)))
    open(tmp_path / "r.faa", "w").write("".join(f">{h} some words\n{s.decode()[:50].lower()}--.\n{s.decode()[50:]}*\n" for h, s in zip(ref_names, refs)))
    args = [str(tmp_path / "r.faa"), str(tmp_path / "p.fa"), "PREFIX", "10", "1", "5,-4", "10", "15", str(tmp_path / "n.fa"), "NPREFIX"]

    def with_prefix(tag):
        return [a.replace("NPREFIX", str(tmp_path / f"{tag}_n")).replace("PREFIX", str(tmp_path / tag)) for a in args]

    subprocess.run([BIN, "chimera"] + with_prefix("one"), check=True, capture_output=True, timeout=120)
    subprocess.run([BIN, "chimera"] + with_prefix("short")[:8], check=True, capture_output=True, timeout=120)
    req = "\t".join(["chimera"] + with_prefix("w")) + "\nquit\n"
    r = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0"], r.stderr[-2000:]
    names, ref_seqs = nr.read_refs(str(tmp_path / "r.faa"))
    assert names == ref_names and ref_seqs == [s.decode() for s in refs]
    res = ctx.chimera(seqs, ref_seqs, mm(), 10, 1, 10, 15)
    assert sorted(set(res["recs"]["status"].tolist())) == [0, 1, 2] and res["recs"]["status"][-1] == 1
    ch.write_chimera(str(tmp_path / "py"), headers, seqs, names, res)
    for tail in ("_chimera.txt", "_nochim.fasta"):
        text = open(f"{tmp_path}/py{tail}").read()
        assert open(f"{tmp_path}/one{tail}").read() == open(f"{tmp_path}/w{tail}").read() == open(f"{tmp_path}/short{tail}").read() == text and text, tail
    kept = [j for j in range(len(seqs)) if res["recs"]["status"][j] != 1]
    want_nucl = "".join(f">{headers[j]} nucl\n{nucl[j]}\n" for j in kept)
    assert open(tmp_path / "one_n_nochim.fasta").read() == open(tmp_path / "w_n_nochim.fasta").read() == want_nucl
    assert not os.path.exists(tmp_path / "short_n_nochim.fasta")
    assert open(tmp_path / "one_nochim.fasta").read() == "".join(f">{headers[j]}\n{seqs[j]}\n" for j in kept)
    back = ch.read_chimera(f"{tmp_path}/one_chimera.txt")
    first = nr.ref_index(names)
    for f, col in (("ref", "ref_names"), ("left_ref", "left_names"), ("right_ref", "right_names")):
        assert [(-1 if x is None else first[x]) for x in back[col]] == res["recs"][f].tolist()
    for f in ch.REC.names:
        assert f.endswith("ref") or np.array_equal(back["recs"][f], res["recs"][f]), f
    # the files against the yardstick
    some = [0, 4, len(seqs) - 2, len(seqs) - 1]
    want, _ = restate_chimera([seqs[j].encode() for j in some], refs, mm(), 10, 1, 10, 15)
    assert [tuple(int(v) for v in res["recs"][j]) for j in some] == want
    # nucleotide records under other names, parameters out of range: the step fails and leaves nothing
    open(tmp_path / "other.fa", "w").write("".join(f">x{j}\n{s}\n" for j, s in enumerate(nucl)))
    bad = with_prefix("bad")
    for k, v in ((8, str(tmp_path / "other.fa")), (6, "0"), (7, "0"), (3, "1025")):
        a = list(bad)
        a[k] = v
        r = subprocess.run([BIN, "chimera"] + a, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "chimera" in r.stderr and "nothing written" in r.stderr, (k, r.stderr)
    assert [f for f in os.listdir(tmp_path) if f.startswith("bad")] == []


# ---- 11. driver end to end -----------------------------------------------------------------------------------------------------------
def check_driver_files(ctx, d, tail, ref_path, scoring, go, ge, min_seg, min_gain):
    """prot<tail>.fasta, prot<tail>_chimera.txt and the two _nochim files: every line of the table is what Context.chimera gives on the
    file's sequences, and the _nochim files hold exactly the names that are not chimeric"""
    with open(f"{d}/prot{tail}.fasta", encoding="latin-1") as fh:
        records = nr.parse_fasta(fh.read())
    with open(f"{d}/nucl{tail}.fasta", encoding="latin-1") as fh:
        nrecords = nr.parse_fasta(fh.read())
    names, ref_seqs = nr.read_refs(ref_path)
    seqs = [s for _, s in records]
    res = ctx.chimera(seqs, ref_seqs, nr.parse_scoring(scoring), go, ge, min_seg, min_gain)
    rec_names = [nr.record_name(h) for h, _ in records]
    assert len(records) > 0 and [nr.record_name(h) for h, _ in nrecords] == rec_names
    assert open(f"{d}/prot{tail}_chimera.txt", encoding="latin-1").read() == ch.chimera_text(rec_names, [len(s) for s in seqs], names, res["recs"])
    kept = [i for i in range(len(records)) if res["recs"]["status"][i] != 1]
    assert open(f"{d}/prot{tail}_nochim.fasta", encoding="latin-1").read() == "".join(f">{records[i][0]}\n{records[i][1]}\n" for i in kept)
    assert open(f"{d}/nucl{tail}_nochim.fasta", encoding="latin-1").read() == "".join(f">{nrecords[i][0]}\n{nrecords[i][1]}\n" for i in kept)
    return res["recs"]["status"].tolist()


@gpu
def test_driver_chimera_end_to_end(ctx, golden_dir, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    mg = synth.make_metagenome(6000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)    # the sample of test_driver_nearest_end_to_end
    synth.write_fasta(mg.reads, str(tmp_path / "reads.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "45", "-t", "4", "--min-contig-len", "150"]

    def step_files(out):
        return sorted(f for _, _, files in os.walk(out) for f in files if "chim" in f)

    def all_files(out):
        return sorted(os.path.relpath(os.path.join(d, f), out) for d, _, files in os.walk(out) for f in files)

    # without the flag: no file of the step, and the checkpoints of a run without flags
    out = tmp_path / "out"
    r = subprocess.run(base + ["-o", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
    assert step_files(out) == [] and open(out / "tmp" / "cp.txt").read().splitlines() == [f"{i}\tdone" for i in range(6)]
    assert "for chimeras" not in open(out / "log").read()
    # the flag alone: the step reads every protein contig, and its checkpoint is the last
    out1 = tmp_path / "out1"
    r = subprocess.run(base + ["-o", str(out1), "--chimera"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out1 / "log").read()[-2000:]
    d = out1 / "contigs" / "rplB"
    assert step_files(out1) == ["nucl_merged_nochim.fasta", "prot_merged_chimera.txt", "prot_merged_nochim.fasta"]
    status = check_driver_files(ctx, d, "_merged", f"{toy}/ref_aligned.faa", "5,-4", 10, 1, 10, 15)
    assert [f for f in all_files(out1) if "chim" not in f] == all_files(out)                                       # the run is what it was
    for f in ("prot_merged.fasta", "nucl_merged.fasta"):
        assert open(d / f).read() == open(out / "contigs" / "rplB" / f).read()
    assert open(out1 / "tmp" / "cp.txt").read().splitlines() == [f"{i}\tdone" for i in range(6 + 1)]
    log = open(out1 / "log").read()
    assert log.count("Checking the contigs of rplB for chimeras") == 1 and log.count("Searching contigs") == 1
    # with --derep and --nearest, and parameters of its own: the step reads what --derep kept, behind --nearest
    out2 = tmp_path / "out2"
    r = subprocess.run(base + ["-o", str(out2), "--derep", "--nearest", "--chimera", "--nearest-scoring", "3,-2", "--nearest-gap-open", "5", "--nearest-gap-extend", "2",
                               "--chimera-min-seg", "5", "--chimera-min-gain", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out2 / "log").read()[-2000:]
    d = out2 / "contigs" / "rplB"
    assert step_files(out2) == ["nucl_merged_rmdup_nochim.fasta", "prot_merged_rmdup_chimera.txt", "prot_merged_rmdup_nochim.fasta"]
    status2 = check_driver_files(ctx, d, "_merged_rmdup", f"{toy}/ref_aligned.faa", "3,-2", 5, 2, 5, 1)
    assert 0 < len(status2) <= len(status)
    assert open(out2 / "tmp" / "cp.txt").read().splitlines() == [f"{i}\tdone" for i in range(6 + 3)]
    log = open(out2 / "log").read()
    assert log.index("Finding the nearest reference") < log.index("Checking the contigs of rplB for chimeras")
    print(f"driver: statuses {status} and {status2}")
