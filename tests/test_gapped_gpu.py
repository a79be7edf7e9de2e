"""Gapped pileup (mgta_reads_pileup_gapped, Graph.pileup_gapped) on the device.

Expected values never come from the library.  restate() does the rule of include/megagta_hip.h in Python over strings: a dict of the
contigs' windows gives the occurrences, a dict per (contig, orientation, diagonal) the anchor windows (the sets P1 / P2 of the rule), the
breakpoint is found by trying every legal b, placements are sorted().  The graph is the `-m 1` graph of the call's reads built on the
device, so every read window has an edge.  Every designed read is looked up in the restatement first (design()): the test asserts that
the inputs hold what they were made to hold before it asks the library anything.

Shapes: k = 21 and k = 31, a 3 000-letter genome, 13 contigs, about 1 000 reads of k + 1 .. 120 letters in both orientations; the reads
of case 8 are longer, 148 letters at k = 31: both orders of its pair of diagonals need k + 1 letters on either side of either breakpoint
inside the repeat (2 (k + 1) + 2 units), and the read an anchored flank of k + 1 letters on either side of that."""
import ctypes as C
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from megagta_amd import readlib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
DNA = "ACGT"
COMP = str.maketrans("ACGTacgt", "TGCAtgca")
CONTIG_FIELDS = ("len", "n_covered", "min_depth", "max_depth", "n_placed", "n_unique", "depth_sum", "mismatch_sum")
PLACE_FIELDS = ("score", "contig", "diag", "orient", "n_placed", "n_mismatch", "diag2", "brk")
GAP_FIELDS = ("read", "contig", "pos", "len", "brk", "orient", "unique")
STAT_FIELDS = ("n_contigs", "n_contig_letters", "n_contig_windows", "n_keys", "n_occurrences", "n_reads", "n_read_windows", "n_hit_windows",
               "n_reads_with_candidate", "n_candidates", "n_verified", "n_reads_placed", "n_reads_multi", "n_placements", "n_bases_piled",
               "n_gap_candidates", "n_gap_passing", "n_reads_gapped", "n_gap_placements", "n_inserted", "n_deleted", "diag_list_entries")
VOLATILE = ("groups_per_cu", "peak_bytes", "n_read_walked", "n_read_index_searches")
G = 32                                                                       # the default max_gap


def rc(s):
    return s.translate(COMP)[::-1]


def codes(s):
    return np.array([DNA.index(c) for c in s], dtype=np.uint8)


def rand_dna(rng, n):
    return "".join(DNA[c] for c in rng.integers(0, 4, n))


def other(ch, step=1):
    return DNA[(DNA.index(ch) + step) % 4]


def subst(s, at):
    s = list(s)
    for p in at:
        s[p] = other(s[p])
    return "".join(s)


def make_inputs(k, seed=5):
    """-> dict(strs = the reads as sequenced, seqs = the contigs, genome, named = name -> read number of the designed reads,
    clean = the numbers of the error-free genome reads with origin = their (start, end) on the genome)"""
    rng = np.random.default_rng(seed + k)
    w = k + 1
    genome = rand_dna(rng, 3000)
    strs, named, clean, origin = [], {}, [], {}

    def add(name, s, flip=False):
        named[name] = len(strs)
        strs.append(rc(s) if flip else s)

    for i in range(880):
        n = int(rng.integers(w, 121))
        p = int(rng.integers(0, 3000 - n + 1))
        s = genome[p:p + n]
        kind = i % 10
        if kind == 3:
            s = subst(s, [int(rng.integers(0, n))])
        elif kind == 5 and n > 2 * w + 8:                                    # a deletion of 1 .. 5 letters somewhere with k + 1 letters on either side
            at, m = int(rng.integers(w, n - w - 5)), int(rng.integers(1, 6))
            s = s[:at] + s[at + m:]
        elif kind == 7 and n > 2 * w + 8 and n < 116:                        # an insertion of 1 .. 4 letters
            at = int(rng.integers(w, n - w))
            s = s[:at] + rand_dna(rng, int(rng.integers(1, 5))) + s[at:]
        elif kind not in (3, 5, 7):
            clean.append(len(strs))
            origin[len(strs)] = (p, p + n)
        strs.append(rc(s) if i % 2 else s)
    a = genome[400:1000]
    b = subst(a, [100, 300, 301, 450])
    # ---- the contigs of the designed reads
    unit = "ACGTTGCAAG"
    tandem = genome[2700:2760] + "A" * 12 + genome[2760:2830] + "CAG" * 6 + genome[2830:2900]
    rep_n = (2 * w + 2 * len(unit) + 4) // len(unit) + 1                      # copies of the unit in the contig of case 8
    rep = genome[2150:2200] + unit * rep_n + genome[2200:2250]
    e0 = genome[2400:2700]
    e = e0[:50] + e0[50:120].lower() + e0[120:150] + "N" + e0[151:]
    runs = "A" * (w // 4) + "C" * (w // 4) + "G" * (w // 4) + "T" * (w + 1 - 3 * (w // 4))          # k + 2 letters in four runs
    tie = genome[2900:2980] + runs + "T"
    c2 = genome[950:1500]
    t4 = rc(genome[1600:2140])                                                # the contig is its letters from 40 on: the read starts before it
    seqs = [a, b, c2, a, t4[40:], rep, e, tandem, tie, genome[20:20 + w], "", rand_dna(rng, 200), genome[10:10 + k]]

    def firm(src, at, dele):
        """the first position from `at` on where a deletion of `dele` letters cannot be moved left or right without a mismatch"""
        while src[at - 1] == src[at + dele - 1] or src[at] == src[at + dele]:
            at += 1
        return at

    def ins_of(src, at, m):
        """m letters to go in front of src[at] that cannot be moved left either"""
        x = rand_dna(rng, m)
        return x[:-1] + (other(src[at - 1]) if x[-1] == src[at - 1] else x[-1])

    def gap(src, at, left, right, dele=0, m=0):
        at = firm(src, at, dele) if dele else at
        return src[at - left:at] + (ins_of(src, at, m) if m else "") + src[at + dele:at + dele + right]

    # 1. deletions and insertions of 1, 3, G and G + 1 letters in mid-read
    for m in (1, 3, G, G + 1):
        add("del%d" % m, gap(c2, 150, w + 8, w + 12, dele=m), flip=m == 3)
        add("ins%d" % m, gap(c2, 250, w + 5, w + 7, m=m), flip=m == 1)
    # 2. / 3. the breakpoint exactly k + 1 letters from the start (the end) of the read, and one letter nearer
    add("left_edge", gap(c2, 330, w, 50, dele=2))
    add("left_short", gap(c2, 330, k, 50, dele=2))
    add("right_edge", gap(c2, 390, 50, w, dele=2), flip=True)
    add("right_short", gap(c2, 390, 50, k, dele=2))
    add("right_edge_ins", gap(c2, 390, 50, w, m=2))
    add("right_short_ins", gap(c2, 390, 50, k, m=2))
    # 4. a gap in a homopolymer and in a tandem repeat of unit 3
    add("homo_del", tandem[60 - w - 3:60] + tandem[61:72 + w + 2])
    add("homo_ins", tandem[60 - w - 3:60] + "A" + tandem[60:72 + w + 2], flip=True)
    add("tandem_del", tandem[142 - w - 1:142] + tandem[145:160 + w + 4])
    add("tandem_ins", tandem[142 - w - 1:145] + "CAG" + tandem[145:160 + w + 4])
    # 5. a substitution 1 and 2 letters beside the gap, on either side
    for j, off in enumerate((-2, -1, 0, 1)):
        add("sub_del%d" % off, subst(gap(c2, 440, w + 12, w + 14, dele=4), [w + 12 + off]), flip=bool(j & 1))
        add("sub_ins%d" % off, subst(gap(c2, 480, w + 12, w + 5, m=3), [w + 12 + off if off < 0 else w + 12 + 3 + off]))
    # 6. breakpoints b mod 8 = 0 .. 7, lengths that are no multiple of 8, insertions that move the right side across a step of 8
    for j in range(8):
        add("mod_del%d" % j, gap(genome, 1050 + 3 * j, w + 8 + j, w + 9 + 2 * j, dele=1 + j % 3), flip=bool(j & 1))
        add("mod_ins%d" % j, gap(genome, 1150 + 5 * j, w + 8 + j, w + 2 + j, m=(5, 8, 11, 7)[j % 4]))
    # 7. a gapped read on two equal contigs
    add("twice", gap(a, 200, w + 9, w + 11, dele=5))
    # 8. a read with a unit less inside the internal repeat: both orders of its two diagonals have a legal breakpoint
    add("repeat", genome[2200 - w - 2:2200] + unit * (rep_n - 1) + genome[2200:2200 + w + 2])
    # 9. the right side running over the contig's end, the left side before its start
    at = firm(genome, 1500 - w - 10, 3)
    add("over_end", genome[at - w - 14:at] + genome[at + 3:1515])
    add("before_start", gap(t4, 40 + w + 7, w + 7 + 12, w + 13, m=2))
    # 10. two gaps
    add("two_gaps", c2[20:20 + w + 4] + c2[20 + w + 6:20 + 2 * w + 10] + c2[20 + 2 * w + 13:20 + 3 * w + 17])
    # 11. the ungapped and the gapped candidate score the same: an A more in front of the runs, whose letters shifted by one differ in 3 places
    add("same_score", tie[20:80] + "A" + runs[:w])
    # 12. a gapped candidate that fails max_mismatch_permille (7 of about 115), and a short one for the call with min_overlap = 80
    add("permille", subst(gap(c2, 350, 50 + w, w + 8, dele=3), [2, 9, 15, 22, 30, 38, 45]))
    add("short", gap(c2, 290, w + 2, w + 2, dele=2))
    # 13. lower-case letters on the left side and an N beside the gap
    m = next(m for m in range(3, 9) if e0[150] != e0[150 + m])               # (the letter on the N finds no equal letter across the gap either)
    add("n_beside", e0[150 - w - 14:151] + e0[151 + m:151 + m + w + 10])
    add("lower", gap(e0, 40 + w + 20, w + 20, w + 19, dele=1), flip=True)
    strs += ["", genome[5:5 + k], rand_dna(rng, 80)]
    return dict(strs=strs, seqs=seqs, genome=genome, named=named, clean=clean, origin=origin)


def read_windows(strs, k):
    out = set()
    for s in dict.fromkeys(strs):
        for t in (s, rc(s)):
            out.update(t[p:p + k + 1] for p in range(len(t) - k))
    return out


def restate(strs, seqs, k, in_graph, min_anchors=0, min_overlap=0, permille=0, max_gap=0, gap_open=0, gap_extend=0):
    """the whole result of Graph.pileup_gapped(reads, seqs, per_read=True) by comparing strings, in Python integers; info[r] = what the
    rule saw of read r, for design()"""
    min_anchors, min_overlap, permille = min_anchors or 1, min_overlap or k + 1, permille or 50
    max_gap, gap_open, gap_extend = max_gap or 32, gap_open or 4, gap_extend or 1
    up = [s.upper() for s in seqs]
    occ = {}
    for i, c in enumerate(up):
        for q in range(len(c) - k):
            w = c[q:q + k + 1]
            if set(w) <= set(DNA) and w in in_graph:
                occ.setdefault(w, []).append((i, q))
    keys = set(occ) | {rc(w) for w in occ if rc(w) in in_graph}
    n_occ = sum(len(v) * (1 + (rc(w) in in_graph)) for w, v in occ.items())
    most_occ = max((len(occ.get(w, ())) + len(occ.get(rc(w), ())) for w in keys), default=0)
    counts = [[[0, 0, 0, 0] for _ in c] for c in up]
    uniq = [[0] * len(c) for c in up]
    ctg = [dict(n_placed=0, n_unique=0, mismatch_sum=0) for _ in up]
    reads, gaps, info = [], [], []
    st = Counter()
    for r, s in enumerate(strs):
        anchors, n_start = {}, 0
        st["n_read_windows"] += max(0, len(s) - k)
        st["n_hit_windows"] += sum(s[p:p + k + 1] in keys for p in range(len(s) - k))
        for o, t in enumerate((s, rc(s))):
            edge = [t[p:p + k + 1] in in_graph for p in range(len(t) - k)]
            for p in range(len(t) - k):
                if edge[p]:
                    for i, q in occ.get(t[p:p + k + 1], ()):
                        anchors.setdefault((i, o, q - p), set()).add(p)
                        n_start += not (p > 0 and q > 0 and edge[p - 1] and up[i][q - 1] == t[p - 1])
        L = len(s)
        passing, seen = [], dict(gap_cands=[], n_b_tied={})                   # passing: (score, i, o, d1, d2, b, n_mm, pairs)
        for (i, o, d), P in anchors.items():
            t = rc(s) if o else s
            pairs = [(p, p + d) for p in range(L) if 0 <= p + d < len(up[i])]
            n_mm = sum(up[i][x] != t[p] for p, x in pairs)
            if len(P) >= min_anchors and len(pairs) >= min_overlap and n_mm * 1000 <= permille * len(pairs):
                passing.append((len(pairs) - 2 * n_mm, i, o, d, d, 0, n_mm, pairs))
        for (i, o, d1), P1 in anchors.items():
            for (i2, o2, d2), P2 in anchors.items():
                g = abs(d2 - d1)
                if (i2, o2) != (i, o) or g == 0 or g > max_gap:
                    continue
                ins = max(0, d1 - d2)
                legal = range(min(P1) + k + 1, max(P2) - ins + 1)
                if not legal:
                    continue
                t = rc(s) if o else s
                c = up[i]
                tried = []
                for b in legal:
                    pairs = [(p, p + d1) for p in range(b) if 0 <= p + d1 < len(c)] + [(p, p + d2) for p in range(b + ins, L) if 0 <= p + d2 < len(c)]
                    n_mm = sum(c[x] != t[p] for p, x in pairs)
                    tried.append((len(pairs) - 2 * n_mm - (gap_open + gap_extend * g), -b, n_mm, pairs))
                assert len({len(x[3]) for x in tried}) == 1                  # n_ov is the same for every legal b
                score, b, n_mm, pairs = max(tried)[0], -max(tried)[1], max(tried)[2], max(tried)[3]
                votes = sum(p + k + 1 <= b for p in P1) + sum(p >= b + ins for p in P2)
                ok = votes >= min_anchors and len(pairs) >= min_overlap and n_mm * 1000 <= permille * len(pairs)
                seen["gap_cands"].append(dict(i=i, o=o, d1=d1, d2=d2, b=b, n_mm=n_mm, n_ov=len(pairs), ok=ok, score=score,
                                              n_tied=sum(x[0] == score for x in tried), clipped=len(pairs) < L - ins))
                st["n_gap_candidates"] += 1
                st["n_gap_passing"] += ok
                if ok:
                    passing.append((score, i, o, d1, d2, b, n_mm, pairs))
        st["n_reads_with_candidate"] += bool(anchors)
        st["n_candidates"] += len(anchors)
        st["n_verified"] += n_start
        best = max((p[0] for p in passing), default=None)
        placed = sorted(p[1:] for p in passing if p[0] == best)
        for i, o, d1, d2, b, n_mm, pairs in placed:
            t = rc(s) if o else s
            for p, x in pairs:
                counts[i][x][DNA.index(t[p])] += 1
                uniq[i][x] += len(placed) == 1
            st["n_bases_piled"] += len(pairs)
            ctg[i]["n_placed"] += 1
            ctg[i]["n_unique"] += len(placed) == 1
            ctg[i]["mismatch_sum"] += n_mm
            if d2 != d1:
                gaps.append((i, b + d1, d2 - d1, r, o, d1, b, int(len(placed) == 1)))
                st["n_gap_placements"] += 1
                st["n_inserted"] += max(0, d1 - d2)
                st["n_deleted"] += max(0, d2 - d1)
        st["n_reads_placed"] += bool(placed)
        st["n_reads_multi"] += len(placed) > 1
        st["n_placements"] += len(placed)
        if placed:
            i, o, d1, d2, b, n_mm, _ = placed[0]
            st["n_reads_gapped"] += d2 != d1
            reads.append(dict(score=best, contig=i, diag=d1, orient=o, n_placed=len(placed), n_mismatch=n_mm, diag2=d2, brk=b))
        else:
            reads.append(dict(score=0, contig=-1, diag=0, orient=0, n_placed=0, n_mismatch=0, diag2=0, brk=0))
        seen["placed"] = [p[:6] for p in placed]
        seen["score"] = best
        info.append(seen)
    rows = []
    for i, c in enumerate(up):
        depth = [sum(x) for x in counts[i]]
        rows.append(dict(len=len(c), n_covered=sum(x > 0 for x in depth), min_depth=min(depth, default=0), max_depth=max(depth, default=0),
                         depth_sum=sum(depth), **ctg[i]))
    longest = max((len(s) for s in strs), default=0)
    st.update(n_contigs=len(up), n_contig_letters=sum(map(len, up)), n_contig_windows=sum(max(0, len(c) - k) for c in up), n_keys=len(keys),
              n_occurrences=n_occ, n_reads=len(strs), diag_list_entries=max(1, max(0, longest - k) * most_occ))
    gaps = [dict(read=g[3], contig=g[0], pos=g[1], len=g[2], brk=g[6], orient=g[4], unique=g[7]) for g in sorted(gaps)]
    return dict(counts=[x for c in counts for x in c], uniq=[x for u in uniq for x in u], rows=rows, reads=reads, gaps=gaps,
                stats={f: int(st[f]) for f in STAT_FIELDS}, info=info)


def design(d, want, k):
    """the designed reads are what they were made to be, by the restatement alone"""
    w = k + 1
    info, named, strs = want["info"], d["named"], d["strs"]

    def gapped(name):                                                        # the gapped placements of the read: (i, o, d1, d2, b)
        return [p for p in info[named[name]]["placed"] if p[2] != p[3]]

    def cands(name):
        return info[named[name]]["gap_cands"]
    for m in (1, 3, G):                                                       # 1
        (p,) = gapped("del%d" % m)
        assert p[3] - p[2] == m and p[0] == 2 and p[1] == (m == 3), (m, p)
        (p,) = gapped("ins%d" % m)
        assert p[2] - p[3] == m and p[1] == (m == 1), (m, p)
    for name in ("del%d" % (G + 1), "ins%d" % (G + 1)):
        assert not cands(name) and not gapped(name), name
    (p,) = gapped("left_edge")                                                # 2, 3
    assert p[4] == w, p
    assert not cands("left_short") and not gapped("left_short")
    for name, ins in (("right_edge", 0), ("right_edge_ins", 2)):
        (p,) = gapped(name)
        assert p[4] + ins == len(strs[named[name]]) - w, (name, p)
    assert not gapped("right_short") and not gapped("right_short_ins")
    for name, pos, ln in (("homo_del", 60, 1), ("homo_ins", 60, -1), ("tandem_del", 130 + 12, 3), ("tandem_ins", 130 + 12, -3)):   # 4
        (p,) = gapped(name)
        c = [x for x in cands(name) if (x["d1"], x["d2"]) == (p[2], p[3])][0]
        assert c["n_tied"] > 1 and p[4] + p[2] == pos and p[3] - p[2] == ln and p[0] == 7, (name, p, c)
    for off in (-2, -1, 0, 1):                                                # 5
        for name in ("sub_del%d" % off, "sub_ins%d" % off):
            (p,) = gapped(name)
            c = [x for x in cands(name) if (x["d1"], x["d2"]) == (p[2], p[3])][0]
            assert c["n_mm"] <= 1 and abs(p[4] - (w + 12)) <= 2, (name, p, c)     # (b minimises the mismatches: it may step over the substitution)
    assert sum([x for x in cands(n) if x["ok"]][0]["n_mm"] for n in named if n.startswith("sub_")) >= 4
    for j in range(8):                                                        # 6
        (p,) = gapped("mod_del%d" % j)
        assert p[4] % 8 == (w + 8 + j) % 8, (j, p)
        (p,) = gapped("mod_ins%d" % j)
        assert p[4] % 8 == (w + 8 + j) % 8, (j, p)
    assert len({x % 8 for x in range(w + 8, w + 16)}) == 8 and any(len(strs[named["mod_del%d" % j]]) % 8 for j in range(8))
    assert any((gapped("mod_ins%d" % j)[0][4] // 8) != ((gapped("mod_ins%d" % j)[0][4] + gapped("mod_ins%d" % j)[0][2] - gapped("mod_ins%d" % j)[0][3]) // 8) for j in range(8))
    assert len(gapped("twice")) >= 2 and {p[0] for p in gapped("twice")} >= {0, 3}                        # 7
    assert [g["unique"] for g in want["gaps"] if g["read"] == named["twice"]] == [0] * len(gapped("twice"))
    pairs = {(x["d1"], x["d2"]) for x in cands("repeat") if x["i"] == 5}                                 # 8
    assert gapped("repeat") and any((b, a) in pairs for a, b in pairs), pairs
    for name in ("over_end", "before_start"):                                 # 9
        (p,) = gapped(name)
        assert [x for x in cands(name) if (x["d1"], x["d2"]) == (p[2], p[3])][0]["clipped"], name
    assert gapped("before_start")[0][2] < 0 and gapped("before_start")[0][0] == 4
    assert cands("two_gaps") and not gapped("two_gaps")                       # 10
    both = info[named["same_score"]]["placed"]                                # 11
    assert len(both) == 2 and {p[2] == p[3] for p in both} == {True, False}, both
    assert cands("permille") and not any(x["ok"] for x in cands("permille")) and not gapped("permille")     # 12
    assert all(x["n_mm"] * 1000 > 50 * x["n_ov"] for x in cands("permille"))
    (p,) = gapped("n_beside")                                                 # 13
    assert p[0] == 6 and [x for x in cands("n_beside") if (x["d1"], x["d2"]) == (p[2], p[3])][0]["n_mm"] >= 1
    (p,) = gapped("lower")
    assert p[0] == 6 and p[1] == 1 and p[4] + p[2] < 120
    st = want["stats"]
    assert st["n_gap_candidates"] > st["n_gap_passing"] > st["n_gap_placements"] > 50 and st["n_inserted"] and st["n_deleted"]
    assert 0 < st["n_reads_gapped"] < st["n_reads_placed"] and st["n_reads_multi"]


def check_result(res, want, what=""):
    assert res["counts"].tolist() == want["counts"], what
    assert res["uniq"].tolist() == want["uniq"], what
    got = [{f: int(c[f]) for f in CONTIG_FIELDS} for c in res["contigs"]]
    assert len(got) == len(want["rows"])
    for i, (g, w) in enumerate(zip(got, want["rows"])):
        assert g == w, (what, i, g, w)
    got = [{f: int(r[f]) for f in PLACE_FIELDS} for r in res["reads"]]
    assert len(got) == len(want["reads"])
    for i, (g, w) in enumerate(zip(got, want["reads"])):
        assert g == w, (what, i, g, w)
    got = [{f: int(r[f]) for f in GAP_FIELDS} for r in res["gaps"]]
    assert got == want["gaps"], what
    assert {f: res["stats"][f] for f in STAT_FIELDS} == want["stats"], what


def stable(stats):
    return {n: v for n, v in stats.items() if not n.startswith("ms_") and n not in VOLATILE}


def same(a, b, what=""):
    for key in ("counts", "uniq", "contigs", "reads", "gaps"):
        assert a[key].tobytes() == b[key].tobytes(), (what, key)
    assert stable(a["stats"]) == stable(b["stats"]), what


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(ctx):
    """k = 21 and k = 31: reads, upload, the -m 1 graph built on the device, the contigs and the restatement (computed once, never changed)"""
    from megagta_amd import api
    out = {}
    for k in (21, 31):
        d = make_inputs(k)
        reads = [codes(s) for s in d["strs"]]
        rd = ctx.upload_reads(*readlib.pack_for_build(reads))
        g = api.Graph(ctx, ctx.build_sdbg(rd, k))
        in_graph = read_windows(d["strs"], k)
        out[k] = dict(d, k=k, g=g, rd=rd, reads=reads, in_graph=in_graph, want=restate(d["strs"], d["seqs"], k, in_graph))
    return out


# ---- 1. every output against the restatement, the designed reads first ----------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31])
def test_every_output_equals_the_restatement(cases, k):
    c = cases[k]
    design(c, c["want"], k)
    assert 900 < len(c["strs"]) < 1100 and len(c["seqs"]) == 13 and len({len(s) % 8 for s in c["strs"]}) == 8
    res = c["g"].pileup_gapped(c["rd"], c["seqs"], per_read=True)
    check_result(res, c["want"])
    # the optionals left out: the same counts and records
    r1 = c["g"].pileup_gapped(c["rd"], c["seqs"])
    assert r1["reads"] is None and r1["counts"].tobytes() == res["counts"].tobytes() and r1["gaps"].tobytes() == res["gaps"].tobytes()


@pytest.mark.parametrize("k", [21, 31])
def test_parameters_change_the_result_as_the_restatement_says(cases, k):
    c = cases[k]
    base = c["want"]
    short = c["named"]["short"]
    assert any(p[2] != p[3] for p in base["info"][short]["placed"])
    for par in (dict(min_overlap=80), dict(max_gap=2, gap_open=9, gap_extend=3), dict(gap_open=1, gap_extend=1, max_mismatch_permille=80, min_anchors=2)):
        want = restate(c["strs"], c["seqs"], k, c["in_graph"], par.get("min_anchors", 0), par.get("min_overlap", 0), par.get("max_mismatch_permille", 0),
                       par.get("max_gap", 0), par.get("gap_open", 0), par.get("gap_extend", 0))
        assert want["reads"] != base["reads"] and want["gaps"] != base["gaps"], par
        if "min_overlap" in par:                                              # case 12: a gapped candidate of fewer than 80 pairs
            cs = want["info"][short]["gap_cands"]
            assert cs and all(x["n_ov"] < 80 and not x["ok"] for x in cs)
        check_result(c["g"].pileup_gapped(c["rd"], c["seqs"], params=par, per_read=True), want, str(par))


# ---- 2. what must not move the outputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31])
def test_what_must_not_move_the_outputs(cases, ctx, k):
    c = cases[k]
    g, rd, seqs = c["g"], c["rd"], c["seqs"]
    a = g.pileup_gapped(rd, seqs, per_read=True)
    ctx.set_pileup_chunk(1)
    try:
        one = g.pileup_gapped(rd, seqs, per_read=True)
    finally:
        ctx.set_pileup_chunk(0)
    same(a, one, "chunk 1")
    ctx.set_share_hash_bits(4)
    try:
        few = g.pileup_gapped(rd, seqs, per_read=True)
    finally:
        ctx.set_share_hash_bits(64)
    same(a, few, "4 hash bits")
    order = np.random.default_rng(k).permutation(len(c["reads"]))
    rd2 = ctx.upload_reads(*readlib.pack_for_build([c["reads"][i] for i in order]))
    r = g.pileup_gapped(rd2, seqs, per_read=True)
    rd2.free()
    back = np.empty_like(r["reads"])
    back[order] = r["reads"]
    gaps = r["gaps"].copy()
    gaps["read"] = order[r["gaps"]["read"].astype(np.int64)]
    key = np.lexsort((gaps["pos"].astype(np.int64) - gaps["brk"].astype(np.int64), gaps["orient"], gaps["read"], gaps["len"], gaps["pos"], gaps["contig"]))
    same(a, dict(r, reads=back, gaps=gaps[key]), "reads in another order")


# ---- 3. the witness without the restatement: reads without an indel --------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31])
def test_reads_without_indels_are_placed_as_pileup_places_them(cases, ctx, k):
    c = cases[k]
    keep = c["clean"]
    assert len(keep) > 500
    rd = ctx.upload_reads(*readlib.pack_for_build([c["reads"][i] for i in keep]))
    contigs = [c["genome"], c["genome"][100:900], rc(c["genome"][2000:2600])]
    a = c["g"].pileup(rd, contigs, per_read=True)
    b = c["g"].pileup_gapped(rd, contigs, per_read=True)
    rd.free()
    for key in ("counts", "uniq", "contigs"):
        assert a[key].tobytes() == b[key].tobytes(), key
    for f in a["reads"].dtype.names:
        assert a["reads"][f].tolist() == b["reads"][f].tolist(), f
    assert b["gaps"].size == 0 and (b["reads"]["diag2"] == b["reads"]["diag"]).all() and not b["reads"]["brk"].any()
    assert all(a["stats"][f] == b["stats"][f] for f in a["stats"] if not f.startswith("ms_") and f not in VOLATILE)
    assert b["stats"]["n_gap_placements"] == b["stats"]["n_gap_passing"] == b["stats"]["n_reads_gapped"] == 0
    assert int((a["reads"]["n_placed"] > 0).sum()) == len(keep)


# ---- 4. limits and errors ---------------------------------------------------------------------------------------------------------------
def test_limits_and_errors_leave_the_outputs_untouched(cases, ctx):
    from megagta_amd import _lib
    from megagta_amd.gapped import GAP_DTYPE, PLACE_DTYPE
    c = cases[21]
    g, rd = c["g"], c["rd"]
    L = _lib.load()
    seq = c["seqs"][2].encode()
    off = np.array([0, len(seq)], dtype=np.uint64)
    ns = len(c["strs"])

    def call(par=None, cap=64, n=1, nsr=ns, expect_untouched=True):
        cnt = np.full((len(seq), 4), 7, dtype=np.uint32)
        un = np.full(len(seq), 7, dtype=np.uint32)
        rec = np.full(6, 7, dtype=np.uint64)
        pr = np.full(nsr * 8 + 8, 7, dtype=np.uint32)
        gaps = np.full(cap * 4 + 4, 7, dtype=np.uint64)
        st = _lib.GappedStats()
        st.n_reads = 7
        p = _lib.GappedParams(*par) if par else None
        code = L.mgta_reads_pileup_gapped(g.h, rd.h, 1, nsr, seq, off.ctypes.data, n, C.byref(p) if p else None, cnt.ctypes.data, un.ctypes.data, rec.ctypes.data,
                                          pr.ctypes.data, gaps.ctypes.data, cap, C.byref(st))
        if expect_untouched:
            assert (cnt == 7).all() and (un == 7).all() and (rec == 7).all() and (pr == 7).all() and (gaps == 7).all() and st.n_reads == 7
        return code, L.mgta_last_error(), st, cnt

    assert GAP_DTYPE.itemsize == 32 and PLACE_DTYPE.itemsize == 32
    for par, word in (((0, 0, 0, 256, 0, 0), b"max_gap"), ((0, 0, 0, -1, 0, 0), b"max_gap"), ((0, 0, 0, 0, 256, 0), b"gap_open"), ((0, 0, 0, 0, -2, 0), b"gap_open"),
                      ((0, 0, 0, 0, 3, 4), b"gap_extend"), ((0, 0, 0, 0, 0, -1), b"gap_extend"), ((-1, 0, 0, 0, 0, 0), b"negative"), ((0, 0, 1001, 0, 0, 0), b"permille")):
        code, msg, _, _ = call(par=par)
        assert code == -1 and word in msg, (par, msg)
    code, msg, _, _ = call(nsr=ns + 1)
    assert code == -1 and b"n_short_reads" in msg
    # too small a gap_cap: the count is named and filled in, nothing else is written
    code, msg, st, _ = call(cap=1)
    need = int(st.n_gap_placements)
    assert code == -1 and need > 1 and str(need).encode() in msg and b"gap_cap" in msg
    code, msg, st, cnt = call(cap=need, expect_untouched=False)
    assert code == 0 and int(st.n_gap_placements) == need and not (cnt == 7).all()
    # n = 0 and n_short_reads = 0
    r0 = g.pileup_gapped(rd, [], per_read=True)
    assert r0["counts"].size == 0 and r0["gaps"].size == 0 and all(v == 0 for v in r0["stats"].values()) and (r0["reads"]["contig"] == -1).all()
    r0 = g.pileup_gapped(rd, c["seqs"], n_short_reads=0, per_read=True)
    assert not r0["counts"].any() and not r0["uniq"].any() and r0["reads"].size == 0 and r0["gaps"].size == 0 and all(v == 0 for v in r0["stats"].values())
    assert r0["contigs"]["len"].tolist() == [len(s) for s in c["seqs"]] and not r0["contigs"]["n_placed"].any()


# ---- 5. the command, the worker and the driver ------------------------------------------------------------------------------------------
def tree(root):
    return {os.path.relpath(os.path.join(dp, f), root): open(os.path.join(dp, f), "rb").read() for dp, _, fs in os.walk(root) for f in fs}


def test_driver_command_and_worker(ctx, golden_dir, tmp_path):
    from megagta_amd import api, gapped as gp, phase as ph, pileup as pl, synth
    mg = synth.make_metagenome(2000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)
    strs = ["".join(DNA[c] for c in r) for r in mg.reads]
    for i in range(1000, 2000):                                               # the second library: every other read loses or gains letters in its middle
        if i % 4 == 0:
            strs[i] = strs[i][:70] + strs[i][72:]
        elif i % 4 == 2:
            strs[i] = strs[i][:80] + "GAT" + strs[i][80:]
    for name, part in (("a.fa", strs[:1000]), ("b.fa", strs[1000:])):
        (tmp_path / name).write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(part)))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    out = tmp_path / "run"
    cmd = [sys.executable, DRIVER, "-r", str(tmp_path / "a.fa"), "-r", str(tmp_path / "b.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "21", "-t", "4",
           "--min-contig-len", "100", "--derep", "--pileup", "--min-depth", "2", "--gapped", "--max-gap", "8", "--phase", "--min-link", "1", "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
    ta = tree(str(out))
    stem = "contigs/rplB/nucl_merged_rmdup"
    assert {stem + s for s in ("_pileup.txt", "_pileup_variants.txt", "_pileup_indels.txt", "_phase_links.txt", "_phase_blocks.txt")} <= set(ta)
    assert "--gapped --max-gap 8" in ta["log"].decode()
    cp = ta["tmp/cp.txt"].decode().splitlines()
    assert cp == [f"{i}\tdone" for i in range(len(cp))]
    # the files: the API's arrays on the run's graph and library, in the bytes of the Python writers
    lib = str(out / "tmp" / "reads.lib")
    fa = str(out / "contigs" / "rplB" / "nucl_merged_rmdup.fasta")
    prefix = str(out / "k20" / "20")
    names, seqs = pl.read_fasta(fa)
    g = api.Graph.from_files(ctx, prefix)
    lib_reads = readlib.load_lib_bin(lib)
    rd = ctx.upload_reads(*readlib.pack_for_build(lib_reads))
    res = g.pileup_gapped(rd, seqs, params=dict(max_gap=8), per_read=True)
    assert res["gaps"].size > 0 and set(res["gaps"]["len"].tolist()) <= {2, -3}       # (which reads reach the gene's contigs is the assembly's business)
    texts = gp.format_gapped(names, seqs, res, lib_reads, min_depth=2)
    for key, suffix in (("summary", "_pileup.txt"), ("variants", "_pileup_variants.txt"), ("indels", "_pileup_indels.txt")):
        assert texts[key].encode() == ta[stem + suffix], suffix
    rows = gp.parse_indels(texts["indels"])
    assert rows and sum(x["reads"] for x in rows) == res["gaps"].size and all(x["seq"] in ("GAT", rc("GAT")) for x in rows if x["type"] == "ins")
    # ... and by comparing strings
    as_seq = ["".join(DNA[c] for c in x) for x in lib_reads]
    want = restate(as_seq, seqs, 20, read_windows(as_seq, 20), max_gap=8)
    check_result(res, want, "the run's contigs")
    # the phase files: as_read_place() records fed to Context.phase
    libs = [(to + 1, pe) for _, _, to, _, pe in readlib.read_lib_table(lib)]
    assert len(libs) == 2
    place = gp.as_read_place(res["reads"])
    assert int((place["n_placed"] == 0).sum()) > int((res["reads"]["n_placed"] == 0).sum())
    sites = ph.sites_from_pileup(seqs, res, min_depth=2)
    ptxt = ph.format_phase(names, ctx.phase(rd, place, libs, seqs, sites), min_link=1)
    assert ptxt["links"].encode() == ta[stem + "_phase_links.txt"] and ptxt["blocks"].encode() == ta[stem + "_phase_blocks.txt"]
    # the command alone with other options, and the same argv as a request to the worker
    res2 = g.pileup_gapped(rd, seqs, params=dict(min_overlap=40, max_gap=3, gap_open=2, gap_extend=2))
    rd.free()
    g.free()
    t2 = gp.format_gapped(names, seqs, res2, lib_reads, min_depth=1, min_alt_permille=1, per_base=True)
    one, w = str(tmp_path / "one"), str(tmp_path / "w")
    argv = [prefix, lib, fa, None, "--min-overlap", "40", "--min-depth", "1", "--min-alt-permille", "1", "--per-base", "--gapped", "--max-gap", "3", "--gap-open", "2",
            "--gap-extend", "2"]
    subprocess.run([BIN, "pileup"] + [a or one for a in argv], check=True, capture_output=True, timeout=120)
    for key, suffix in (("summary", "_pileup.txt"), ("variants", "_pileup_variants.txt"), ("depth", "_pileup_depth.txt"), ("indels", "_pileup_indels.txt")):
        assert open(one + suffix).read() == t2[key], suffix
    assert not any(x["len"] > 3 for x in gp.parse_indels(t2["indels"]))
    req = "pileup\t" + "\t".join(a or w for a in argv) + "\nquit\n"
    r = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0"], r.stderr[-2000:]
    for suffix in ("_pileup.txt", "_pileup_variants.txt", "_pileup_depth.txt", "_pileup_indels.txt"):
        assert open(one + suffix, "rb").read() == open(w + suffix, "rb").read(), suffix
    # usage errors: a gap option without --gapped
    for flag in ("--max-gap", "--gap-open", "--gap-extend"):
        r = subprocess.run([BIN, "pileup", prefix, lib, fa, one, flag, "3"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "options of --gapped" in r.stderr and "Usage: megagta pileup" in r.stderr
    r = subprocess.run([BIN, "pileup", prefix, lib, fa, one, "--gapped", "--max-gap", "x"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "is not a count" in r.stderr
