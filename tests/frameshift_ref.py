"""The rule of mgta_seqs_frameshift (include/megagta_hip.h) restated in plain Python, cell by cell, for the tests to compare the device
with.  test_frameshift_host.py checks it against an enumeration of every state path before any kernel is compared with it."""
import numpy as np

from megagta_amd.frameshift import REC, codon_residue
from megagta_amd.nearest import residue_class

INT32_MIN = -(1 << 31)
CLASS_X = residue_class(ord("X"))


def _s(v) -> str:
    return v.decode("latin-1") if isinstance(v, (bytes, bytearray)) else str(v)


def codon_classes(x: str) -> list:
    """[i] = c(a(i)) for i >= 3 (1-based), None below"""
    return [None, None, None] + [residue_class(ord(codon_residue(x[i - 3:i]))) for i in range(3, len(x) + 1)]


def fill(x, y, sub, go, ge, fs):
    """the three tables of one pair, [L + 1][R + 1], None = undefined, and P with the state it came from"""
    x, y = _s(x), _s(y)
    L, R = len(x), len(y)
    ca = codon_classes(x)
    cy = [0] + [residue_class(ord(c)) for c in y]
    M = [[None] * (R + 1) for _ in range(L + 1)]
    X = [[None] * (R + 1) for _ in range(L + 1)]
    Y = [[None] * (R + 1) for _ in range(L + 1)]
    P = [[None] * (R + 1) for _ in range(L + 1)]

    def prev(i, j):
        if i == 0:
            return 0
        return P[i][j] if i >= 1 and j >= 1 else None

    for i in range(1, L + 1):
        Mi, Xi, Yi, Pi = M[i], X[i], Y[i], P[i]
        for j in range(1, R + 1):
            best = None
            if i >= 3:
                p = prev(i - 3, j - 1)
                if p is not None:
                    best = int(sub[ca[i]][cy[j]]) + p
            if i >= 2:
                p = prev(i - 2, j - 1)
                if p is not None:
                    v = int(sub[CLASS_X][cy[j]]) - fs + p
                    if best is None or v > best:
                        best = v
            if i >= 4:
                p = prev(i - 4, j - 1)
                if p is not None:
                    v = int(sub[ca[i]][cy[j]]) - fs + p
                    if best is None or v > best:
                        best = v
            Mi[j] = best
            if i >= 4:
                a, b = M[i - 3][j], X[i - 3][j]
                a = None if a is None else a - go
                b = None if b is None else b - ge
                Xi[j] = a if b is None or (a is not None and a >= b) else b
            if j >= 2:
                a, b = Mi[j - 1], Yi[j - 1]
                a = None if a is None else a - go
                b = None if b is None else b - ge
                Yi[j] = a if b is None or (a is not None and a >= b) else b
            p = Mi[j]
            if Xi[j] is not None and (p is None or Xi[j] > p):
                p = Xi[j]
            if Yi[j] is not None and (p is None or Yi[j] > p):
                p = Yi[j]
            Pi[j] = p
    return dict(L=L, R=R, ca=ca, cy=cy, M=M, X=X, Y=Y, P=P)


def _state_of(t, i, j):
    """the state P[i][j] came from: preference M, X, Y"""
    p = t["P"][i][j]
    for name in ("M", "X", "Y"):
        if t[name][i][j] is not None and t[name][i][j] == p:
            return name
    raise AssertionError("P is undefined")


def pair(x, y, sub, go, ge, fs):
    """one pair -> None when it has no score, else dict(score, jend, path, ref_from, n_match, n_ident, n_insert, n_delete, n_short, n_long)"""
    x, y = _s(x), _s(y)
    t = fill(x, y, sub, go, ge, fs)
    L, R, M, X, Y, P, ca, cy = t["L"], t["R"], t["M"], t["X"], t["Y"], t["P"], t["ca"], t["cy"]
    if L == 0 or R == 0:
        return None
    last = [v for v in M[L][1:] if v is not None]
    if not last:
        return None
    score = max(last)
    jend = M[L].index(score, 1)
    out = dict(score=score, jend=jend, ref_from=0, n_match=0, n_ident=0, n_insert=0, n_delete=0, n_short=0, n_long=0)
    path = []
    i, j, state = L, jend, "M"
    while True:
        if state == "M":
            v = M[i][j]
            cands = []
            for kind, back, need in (("M", 3, 3), ("<", 2, 2), (">", 4, 4)):
                if i < need:
                    continue
                p = 0 if i - back == 0 else (P[i - back][j - 1] if j - 1 >= 1 else None)
                if p is None:
                    continue
                e = int(sub[CLASS_X][cy[j]]) - fs if kind == "<" else int(sub[ca[i]][cy[j]]) - (fs if kind == ">" else 0)
                cands.append((kind, back, e + p))
            kind, back = next((k, b) for k, b, val in cands if val == v)
            path.append(kind)
            out["n_match" if kind == "M" else "n_short" if kind == "<" else "n_long"] += 1
            if kind != "<" and ca[i] == cy[j] and ca[i] != 0:
                out["n_ident"] += 1
            out["ref_from"] = j
            i, j = i - back, j - 1
            if i == 0:
                break
            state = _state_of(t, i, j)
        elif state == "X":
            path.append("I")
            out["n_insert"] += 1
            a, b = M[i - 3][j], X[i - 3][j]
            state = "M" if a is not None and a - go == X[i][j] else "X"
            assert state == "M" or b - ge == X[i][j]
            i -= 3
        else:
            path.append("D")
            out["n_delete"] += 1
            a, b = M[i][j - 1], Y[i][j - 1]
            state = "M" if a is not None and a - go == Y[i][j] else "Y"
            assert state == "M" or b - ge == Y[i][j]
            j -= 1
    out["path"] = "".join(reversed(path))
    return out


def frameshift(nucl, refs, sub, go, ge, fs):
    """what Context.frameshift(nucl, refs, sub, go, ge, fs, scores=True, paths=True) must give: dict(recs, scores, paths)"""
    n, n_ref = len(nucl), len(refs)
    recs = np.zeros(n, dtype=REC)
    scores = np.full((n, n_ref), INT32_MIN, dtype=np.int32)
    paths = []
    for i, x in enumerate(nucl):
        best = None
        for r, y in enumerate(refs):
            p = pair(x, y, sub, go, ge, fs)
            if p is not None:
                scores[i, r] = p["score"]
                if best is None or p["score"] > best[1]["score"]:
                    best = (r, p)
        if best is None:
            recs[i] = (1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0)
            paths.append("")
        else:
            r, p = best
            recs[i] = (0, r, p["score"], p["ref_from"], p["jend"], p["n_match"], p["n_ident"], p["n_insert"], p["n_delete"], p["n_short"], p["n_long"])
            paths.append(p["path"])
    return dict(recs=recs, scores=scores, paths=paths)


def enumerate_best(x, y, sub, go, ge, fs):
    """The same answer with no table: every state path of the pair is written out and scored on its own, the best taken.  Among the
    paths of the highest score the one with the lowest end column wins, then, read from its END, the one whose choices come first:
    a match state before an insert before a delete state, a codon before a short before a long codon.
    -> None or (score, jend, path)"""
    x, y = _s(x), _s(y)
    L, R = len(x), len(y)
    ca = codon_classes(x)
    cy = [0] + [residue_class(ord(c)) for c in y]
    rank = {"M": (0, 0), "<": (0, 1), ">": (0, 2), "I": (1, 0), "D": (2, 0)}
    found = []

    def grow(ops, i, j, score):
        """ops end at nucleotide i and column j"""
        last = ops[-1]
        if i == L and last in "M<>":
            found.append((-score, j, [rank[o] for o in reversed(ops)], "".join(ops)))
        for op, take in (("M", 3), ("<", 2), (">", 4)):
            if i + take <= L and j + 1 <= R:
                e = int(sub[CLASS_X][cy[j + 1]]) - fs if op == "<" else int(sub[ca[i + take]][cy[j + 1]]) - (fs if op == ">" else 0)
                grow(ops + [op], i + take, j + 1, score + e)
        if last != "D" and i + 3 <= L:
            grow(ops + ["I"], i + 3, j, score - (ge if last == "I" else go))
        if last != "I" and j + 1 <= R:
            grow(ops + ["D"], i, j + 1, score - (ge if last == "D" else go))

    for j0 in range(1, R + 1):
        for op, take in (("M", 3), ("<", 2), (">", 4)):
            if take <= L:
                e = int(sub[CLASS_X][cy[j0]]) - fs if op == "<" else int(sub[ca[take]][cy[j0]]) - (fs if op == ">" else 0)
                grow([op], take, j0, e)
    if not found:
        return None
    neg, jend, _, path = min(found)
    return -neg, jend, path
