"""Pileup (mgta_reads_pileup, Graph.pileup) on the device.

Expected values never come from the code under test.  restate() does the rule of include/megagta_hip.h in Python over strings: a dict
of the contigs' windows gives the occurrences, a Counter per (contig, orientation, diagonal) holds the votes, verification compares
letters, placements are sorted().  The graph is the `-m 1` graph of the call's reads built on the device (its md5 checked against the
oracle's), so a read window always has an edge; test 4 uses the graph of a part of the reads and gives the restatement that set.
The second witness counts no windows: one contig equal to the genome and the error-free reads, whose origin is known.

`max_mismatch_permille = 0` takes the default like every parameter given as 0 (the header's `0 = the default of each`), so the test of
the parameters asks for exact matches with 1 permille as well (no overlap here reaches 1000 letters)."""
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
READ_FIELDS = ("score", "contig", "diag", "orient", "n_placed", "n_mismatch")
STAT_FIELDS = ("n_contigs", "n_contig_letters", "n_contig_windows", "n_keys", "n_occurrences", "n_reads", "n_read_windows", "n_hit_windows",
               "n_reads_with_candidate", "n_candidates", "n_verified", "n_reads_placed", "n_reads_multi", "n_placements", "n_bases_piled")
VOLATILE = ("groups_per_cu", "peak_bytes", "n_read_walked", "n_read_index_searches")


def rc(s):
    return s.translate(COMP)[::-1]


def codes(s):
    return np.array([DNA.index(c) for c in s], dtype=np.uint8)


def rand_dna(rng, n):
    return "".join(DNA[c] for c in rng.integers(0, 4, n))


def subst(s, at):
    s = list(s)
    for p in at:
        s[p] = DNA[(DNA.index(s[p]) + 1) % 4]
    return "".join(s)


def make_inputs(k, seed=3):
    """-> dict(strs = the reads as sequenced, origin = per read (start, end) on the genome for the error-free genome reads else None,
    seqs = the contigs, genome)"""
    rng = np.random.default_rng(seed + k)
    genome = rand_dna(rng, 3000)
    strs, origin = [], []
    for i in range(900):
        n = int(rng.integers(k + 1, 101))
        p = int(rng.integers(0, 3000 - n + 1))
        s = genome[p:p + n]
        n_sub = {3: 1, 5: 3, 7: 9}.get(i % 10, 0)
        if n_sub:
            s = subst(s, sorted(set(int(x) for x in rng.integers(0, n, n_sub))))
        strs.append(rc(s) if i % 2 else s)
        origin.append(None if n_sub else (p, p + n))
    a = genome[400:1000]
    b = subst(a, [100, 300, 301, 450])                                      # a variant of A: four substitutions, two of them adjacent
    for i, p in enumerate((30, 60, 90, 230, 260, 280, 295, 380, 400, 420) * 3):
        s = b[p:p + 70 + i]
        strs.append(rc(s) if i % 3 == 0 else s)
        origin.append(None)
    x = genome[2200:2200 + k + 40]                                           # the unit of an internal repeat longer than k + 1
    rep = genome[2150:2200] + x + x + genome[2200 + k + 40:2200 + k + 80]
    hot = rc(genome[1700:1790])
    extra = [genome[5:5 + k], "", rand_dna(rng, 80),                          # length k, length 0, foreign
             genome[10:20 + k + 1 + 10],                                      # overhangs both ends of the contig of k + 1 letters
             genome[380:460], genome[940:1030],                               # over A's start; over A's end, inside the adjacent piece
             subst(genome[500:560], [50, 53, 56, 58]),                        # a candidate that does not pass: 4 of 60
             subst(genome[600:700], [48]),                                    # two runs on one diagonal
             x[2:k + 12], rc(x[5:k + 30]), x[:k + 1]]                         # inside the repeat unit: two diagonals of one contig
    late = rand_dna(rng, 150)                                                # seen by the last reads only: test 4 builds the graph without them
    strs += extra[:6] + [hot] * 40 + extra[6:] + [late[:90], rc(late[40:140])]
    origin += [None] * (len(extra) + 42)
    e = genome[2400:2700]
    e = e[:50] + e[50:120].lower() + e[120:150] + "N" + e[151:]
    seqs = [a, b, genome[950:1500], a, rc(genome[1600:2100]), rep, e, genome[10:10 + k], genome[20:20 + k + 1], "", rand_dna(rng, 200), late]
    return dict(strs=strs, origin=origin, seqs=seqs, genome=genome)


def read_windows(strs, k):
    """the (k+1)-mers of the reads on either strand: the edges of their `-m 1` graph"""
    out = set()
    for s in dict.fromkeys(strs):
        for t in (s, rc(s)):
            out.update(t[p:p + k + 1] for p in range(len(t) - k))
    return out


def restate(strs, seqs, k, in_graph, min_anchors=0, min_overlap=0, permille=0):
    """the whole result of Graph.pileup(reads, seqs, per_read=True) by comparing strings, in Python integers"""
    min_anchors = min_anchors or 1
    min_overlap = min_overlap or k + 1
    permille = permille or 50
    up = [s.upper() for s in seqs]
    occ = {}
    for i, c in enumerate(up):
        for q in range(len(c) - k):
            w = c[q:q + k + 1]
            if set(w) <= set(DNA) and w in in_graph:
                occ.setdefault(w, []).append((i, q))
    keys = set(occ) | {rc(w) for w in occ if rc(w) in in_graph}
    n_occ = sum(len(v) * (1 + (rc(w) in in_graph)) for w, v in occ.items())
    counts = [[[0, 0, 0, 0] for _ in c] for c in up]
    uniq = [[0] * len(c) for c in up]
    ctg = [dict(n_placed=0, n_unique=0, mismatch_sum=0) for _ in up]
    reads, census = [], Counter()
    st = Counter()
    for s in strs:
        votes, first, n_start = Counter(), {}, 0
        st["n_read_windows"] += max(0, len(s) - k)
        st["n_hit_windows"] += sum(s[p:p + k + 1] in keys for p in range(len(s) - k))
        for o, t in enumerate((s, rc(s))):
            edge = [t[p:p + k + 1] in in_graph for p in range(len(t) - k)]
            for p in range(len(t) - k):
                if not edge[p]:
                    continue
                for i, q in occ.get(t[p:p + k + 1], ()):
                    votes[(i, o, q - p)] += 1
                    first.setdefault((i, o, q - p), []).append(p)
                    n_start += not (p > 0 and q > 0 and edge[p - 1] and up[i][q - 1] == t[p - 1])
        passing = []
        for (i, o, d), v in votes.items():
            t = rc(s) if o else s
            x0, x1 = max(0, d), min(len(up[i]), d + len(t))
            n_mm = sum(up[i][x] != t[x - d] for x in range(x0, x1))
            ps = first[(i, o, d)]
            census["two_runs"] += any(b - a > 1 for a, b in zip(ps, ps[1:]))
            census["negative"] += d < 0
            census["past_end"] += d + len(t) > len(up[i])
            if v >= min_anchors and x1 - x0 >= min_overlap and n_mm * 1000 <= permille * (x1 - x0):
                passing.append((x1 - x0 - 2 * n_mm, i, o, d, n_mm))
        st["n_reads_with_candidate"] += bool(votes)
        st["n_candidates"] += len(votes)
        st["n_verified"] += n_start
        best = max((p[0] for p in passing), default=None)
        placed = sorted(p[1:] for p in passing if p[0] == best)
        census["placed_%d" % min(len(placed), 3)] += 1
        census["none_passes"] += bool(votes) and not passing
        census["loser"] += len(passing) > len(placed)
        census["same_contig_twice"] += len({p[0] for p in placed}) < len(placed)
        for i, o, d, n_mm in placed:
            t = rc(s) if o else s
            for x in range(max(0, d), min(len(up[i]), d + len(t))):
                counts[i][x][DNA.index(t[x - d])] += 1
                uniq[i][x] += len(placed) == 1
                st["n_bases_piled"] += 1
            ctg[i]["n_placed"] += 1
            ctg[i]["n_unique"] += len(placed) == 1
            ctg[i]["mismatch_sum"] += n_mm
        st["n_reads_placed"] += bool(placed)
        st["n_reads_multi"] += len(placed) > 1
        st["n_placements"] += len(placed)
        if placed:
            i, o, d, n_mm = placed[0]
            reads.append(dict(score=best, contig=i, diag=d, orient=o, n_placed=len(placed), n_mismatch=n_mm))
        else:
            reads.append(dict(score=0, contig=-1, diag=0, orient=0, n_placed=0, n_mismatch=0))
    rows = []
    for i, c in enumerate(up):
        depth = [sum(x) for x in counts[i]]
        rows.append(dict(len=len(c), n_covered=sum(x > 0 for x in depth), min_depth=min(depth, default=0), max_depth=max(depth, default=0),
                         depth_sum=sum(depth), **ctg[i]))
    st.update(n_contigs=len(up), n_contig_letters=sum(map(len, up)), n_contig_windows=sum(max(0, len(c) - k) for c in up), n_keys=len(keys),
              n_occurrences=n_occ, n_reads=len(strs))
    return dict(counts=[x for c in counts for x in c], uniq=[x for u in uniq for x in u], rows=rows, reads=reads,
                stats={f: int(st[f]) for f in STAT_FIELDS}, census=census)


def check_result(res, want, what=""):
    assert res["counts"].tolist() == want["counts"], what
    assert res["uniq"].tolist() == want["uniq"], what
    got = [{f: int(c[f]) for f in CONTIG_FIELDS} for c in res["contigs"]]
    assert len(got) == len(want["rows"])
    for i, (g, w) in enumerate(zip(got, want["rows"])):
        assert g == w, (what, i, g, w)
    if res["reads"] is not None:
        got = [{f: int(r[f]) for f in READ_FIELDS} for r in res["reads"]]
        assert len(got) == len(want["reads"])
        for i, (g, w) in enumerate(zip(got, want["reads"])):
            assert g == w, (what, i, g, w)
    assert {f: res["stats"][f] for f in STAT_FIELDS} == want["stats"], what


def stable(stats):
    return {n: v for n, v in stats.items() if not n.startswith("ms_") and n not in VOLATILE}


def same(a, b, what=""):
    for key in ("counts", "uniq", "contigs", "reads"):
        assert a[key].tobytes() == b[key].tobytes(), (what, key)
    assert stable(a["stats"]) == stable(b["stats"]), what


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(ctx, oracle):
    """k = 20 and k = 45: reads, upload, the -m 1 graph built on the device, the contigs and the restatement (computed once, never changed)"""
    from megagta_amd import api
    out = {}
    for k in (20, 45):
        d = make_inputs(k)
        reads = [codes(s) for s in d["strs"]]
        packed, start = readlib.pack_for_build(reads)
        rd = ctx.upload_reads(packed, start)
        stream = ctx.build_sdbg(rd, k)
        assert stream.md5() == oracle.Stream.build(packed, start, k, threads=4).edges().md5()
        g = api.Graph(ctx, stream, keep_multiplicity=True)
        in_graph = read_windows(d["strs"], k)
        out[k] = dict(d, k=k, g=g, rd=rd, reads=reads, in_graph=in_graph, want=restate(d["strs"], d["seqs"], k, in_graph))
    return out


# ---- 1. every output against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 45])
def test_every_output_equals_the_restatement(cases, k):
    c = cases[k]
    want, seqs = c["want"], c["seqs"]
    cen = want["census"]
    # the inputs hold what they were made to hold
    assert all(cen["placed_%d" % i] > 0 for i in range(4)), cen
    assert cen["negative"] and cen["past_end"] and cen["none_passes"] and cen["loser"] and cen["two_runs"] and cen["same_contig_twice"], cen
    assert {len(s) for s in seqs} >= {0, k, k + 1} and {len(s) for s in c["strs"]} >= {0, k}
    assert any(r["n_mismatch"] for r in want["reads"]) and want["stats"]["n_verified"] > want["stats"]["n_candidates"]
    res = c["g"].pileup(c["rd"], seqs, per_read=True)
    check_result(res, want)
    # the optionals left out: the same counts (uniq, per_contig and per_read NULL)
    from megagta_amd import _lib
    raw = b"".join(s.encode() for s in seqs)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    counts = np.zeros((len(raw), 4), dtype=np.uint32)
    L = _lib.load()
    assert L.mgta_reads_pileup(c["g"].h, c["rd"].h, 1, len(c["strs"]), raw, off.ctypes.data, len(seqs), None, counts.ctypes.data, None, None, None, None) == 0
    assert counts.tobytes() == res["counts"].tobytes()
    r1 = c["g"].pileup(c["rd"], seqs)
    assert r1["reads"] is None and r1["counts"].tobytes() == res["counts"].tobytes() and r1["contigs"].tobytes() == res["contigs"].tobytes()
    # n = 0 and n_short_reads = 0
    r0 = c["g"].pileup(c["rd"], [], per_read=True)
    assert r0["counts"].size == 0 and all(v == 0 for v in r0["stats"].values()) and (r0["reads"]["contig"] == -1).all() and not r0["reads"]["n_placed"].any()
    r0 = c["g"].pileup(c["rd"], seqs, n_short_reads=0, per_read=True)
    assert not r0["counts"].any() and not r0["uniq"].any() and r0["reads"].size == 0 and all(v == 0 for v in r0["stats"].values())
    assert r0["contigs"]["len"].tolist() == [len(s) for s in seqs] and not r0["contigs"]["n_placed"].any() and not r0["contigs"]["depth_sum"].any()


# ---- 2. the witness that counts no windows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 45])
def test_depth_on_the_genome_is_the_number_of_reads_from_there(cases, ctx, k):
    c = cases[k]
    keep = [i for i, o in enumerate(c["origin"]) if o is not None]
    assert len(keep) > 500
    rd = ctx.upload_reads(*readlib.pack_for_build([c["reads"][i] for i in keep]))
    res = c["g"].pileup(rd, [c["genome"]], per_read=True)
    rd.free()
    depth = np.zeros(3000, dtype=np.int64)
    for i in keep:
        depth[c["origin"][i][0]:c["origin"][i][1]] += 1
    assert res["counts"].sum(axis=1).tolist() == depth.tolist()
    own = res["counts"][np.arange(3000), codes(c["genome"])]
    assert own.tolist() == depth.tolist()                                    # all of it on the genome's own letter
    assert res["uniq"].tolist() == depth.tolist() and int(res["contigs"]["mismatch_sum"][0]) == 0
    assert int(res["contigs"]["n_placed"][0]) == int(res["contigs"]["n_unique"][0]) == len(keep) == int((res["reads"]["n_placed"] == 1).sum())
    for j, i in enumerate(keep):
        p, e = c["origin"][i]
        r = res["reads"][j]
        assert (int(r["diag"]), int(r["orient"]), int(r["score"])) == (p, i % 2, e - p), (i, r)


# ---- 3. what must not move the outputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 45])
def test_what_must_not_move_the_outputs(cases, ctx, k):
    c = cases[k]
    g, rd, seqs = c["g"], c["rd"], c["seqs"]
    a = g.pileup(rd, seqs, per_read=True)
    same(a, g.pileup(rd, seqs, per_read=True), "the call twice")
    g.match_reads(rd, seqs[:3])
    g.contig_sample_coverage(rd, [len(c["strs"])], seqs[2:5])
    g.contig_coverage(seqs[:2])
    same(a, g.pileup(rd, seqs, per_read=True), "after other calls")
    ctx.set_pileup_chunk(1)
    try:
        one = g.pileup(rd, seqs, per_read=True)
        ctx.set_pileup_chunk(7)
        seven = g.pileup(rd, seqs, per_read=True)
    finally:
        ctx.set_pileup_chunk(0)
    same(a, one, "chunk 1")
    same(a, seven, "chunk 7")
    ctx.set_share_hash_bits(4)
    try:
        few = g.pileup(rd, seqs, per_read=True)
    finally:
        ctx.set_share_hash_bits(64)
    same(a, few, "4 hash bits")
    # the reads in another order, per_read permuted back
    order = np.random.default_rng(k).permutation(len(c["reads"]))
    rd2 = ctx.upload_reads(*readlib.pack_for_build([c["reads"][i] for i in order]))
    r = g.pileup(rd2, seqs, per_read=True)
    rd2.free()
    back = np.empty_like(r["reads"])
    back[order] = r["reads"]
    same(a, dict(r, reads=back), "reads in another order")
    # the reads uploaded as sequenced
    lens = np.array([x.size for x in c["reads"]], dtype=np.uint64)
    start = np.zeros(lens.size + 1, dtype=np.uint64)
    np.cumsum(lens, out=start[1:])
    rd3 = ctx.upload_reads(readlib.pack_codes(np.concatenate(c["reads"])), start)
    f = g.pileup(rd3, seqs, per_read=True, reads_reversed=False)
    rd3.free()
    same(a, f, "reads not reversed")
    # the contigs in another order, the records permuted back
    perm = [5, 0, 9, 3, 11, 10, 1, 8, 2, 7, 4, 6]
    assert sorted(perm) == list(range(len(seqs)))
    s = g.pileup(rd, [seqs[i] for i in perm], per_read=True)
    off_a, off_s = a["offsets"], s["offsets"]
    for j, i in enumerate(perm):
        assert s["contigs"][j].tobytes() == a["contigs"][i].tobytes(), (j, i)
        assert s["counts"][off_s[j]:off_s[j + 1]].tobytes() == a["counts"][off_a[i]:off_a[i + 1]].tobytes(), (j, i)
        assert s["uniq"][off_s[j]:off_s[j + 1]].tobytes() == a["uniq"][off_a[i]:off_a[i + 1]].tobytes(), (j, i)
    for f_ in ("score", "n_placed", "n_mismatch"):
        assert s["reads"][f_].tolist() == a["reads"][f_].tolist(), f_
    assert stable(s["stats"]) == stable(a["stats"])


# ---- 4. a graph that lacks edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 45])
def test_a_graph_that_lacks_edges(cases, ctx, k):
    from megagta_amd import api
    c = cases[k]
    rd600 = ctx.upload_reads(*readlib.pack_for_build(c["reads"][:600]))
    g = api.Graph(ctx, ctx.build_sdbg(rd600, k))
    rd600.free()
    in_graph = read_windows(c["strs"][:600], k)
    assert len(in_graph) < len(c["in_graph"])
    want = restate(c["strs"], c["seqs"], k, in_graph)
    res = g.pileup(c["rd"], c["seqs"], per_read=True)
    g.free()
    check_result(res, want, "graph of 600 reads")
    full = c["want"]["reads"]
    assert any(a["n_placed"] and not b["n_placed"] for a, b in zip(full, want["reads"]))
    assert want["stats"]["n_read_windows"] > sum(sum(s[p:p + k + 1] in in_graph for p in range(len(s) - k)) for s in c["strs"])   # windows without an edge


# ---- 5. parameters, limits, errors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 45])
def test_parameters_change_the_result_as_the_restatement_says(cases, k):
    c = cases[k]
    base = c["want"]
    for par in (dict(min_anchors=3), dict(min_overlap=60), dict(max_mismatch_permille=1), dict(max_mismatch_permille=0),
                dict(min_anchors=2, min_overlap=70, max_mismatch_permille=20)):
        want = restate(c["strs"], c["seqs"], k, c["in_graph"], par.get("min_anchors", 0), par.get("min_overlap", 0), par.get("max_mismatch_permille", 0))
        if par != dict(max_mismatch_permille=0):                              # (0 = the default)
            assert want["reads"] != base["reads"] and want["counts"] != base["counts"], par
        else:
            assert want["reads"] == base["reads"]
        check_result(c["g"].pileup(c["rd"], c["seqs"], params=par, per_read=True), want, str(par))


def test_limits_and_errors_leave_the_outputs_untouched(cases, ctx):
    from megagta_amd import _lib, api
    c = cases[20]
    g, rd = c["g"], c["rd"]
    L = _lib.load()
    seq = c["seqs"][0].encode()
    off = np.array([0, len(seq)], dtype=np.uint64)

    def call(gh, rh, ns=10, par=None, n=1, offsets=off, counts=True):
        cnt = np.full((len(seq), 4), 7, dtype=np.uint32)
        un = np.full(len(seq), 7, dtype=np.uint32)
        rec = np.full(1, 7, dtype=np.uint64).repeat(6)
        pr = np.full(ns * 6, 7, dtype=np.uint32)
        st = _lib.PileupStats()
        st.n_reads = 7
        p = _lib.PileupParams(*par) if par else None
        rcode = L.mgta_reads_pileup(gh, rh, 1, ns, seq, offsets.ctypes.data if offsets is not None else None, n, C.byref(p) if p else None,
                                    cnt.ctypes.data if counts else None, un.ctypes.data, rec.ctypes.data, pr.ctypes.data, C.byref(st))
        assert (cnt == 7).all() and (un == 7).all() and (rec == 7).all() and (pr == 7).all() and st.n_reads == 7
        return rcode, L.mgta_last_error()

    for par, word in (((-1, 0, 0), b"negative"), ((0, -5, 0), b"negative"), ((0, 0, -1), b"negative"), ((0, 0, 1001), b"permille")):
        code, msg = call(g.h, rd.h, par=par)
        assert code == -1 and word in msg, (par, msg)
    assert call(None, rd.h)[0] == -1 and call(g.h, None)[0] == -1
    assert call(g.h, rd.h, counts=False)[0] == -1
    code, msg = call(g.h, rd.h, ns=len(c["strs"]) + 1)
    assert code == -1 and b"n_short_reads" in msg
    code, msg = call(g.h, rd.h, n=1 << 31)
    assert code == -1 and b"2^31" in msg
    code, msg = call(g.h, rd.h, offsets=np.array([0, 1 << 32], dtype=np.uint64))
    assert code == -1 and b"2^32" in msg
    code, msg = call(g.h, rd.h, n=-1)
    assert code == -1
    # a read of 65 536 bases
    long_rd = ctx.upload_reads(*readlib.pack_for_build([codes(c["strs"][0]), np.zeros(65536, dtype=np.uint8)]))
    code, msg = call(g.h, long_rd.h, ns=2)
    long_rd.free()
    assert code == -1 and b"65535" in msg
    # (k + 1 <= 128 holds for every graph the build or a load accepts: k <= 127)
    other = api.Context(0)
    try:
        rd2 = other.upload_reads(*readlib.pack_for_build(c["reads"][:50]))
        with pytest.raises(api.MegaGtaError, match=r"\(-1\).*different contexts"):
            g.pileup(rd2, ["A" * 40])
        rd2.free()
    finally:
        other.close()


# ---- 6. the command, the worker and the driver ----------------------------------------------------------------------------------------
def tree(root):
    return {os.path.relpath(os.path.join(dp, f), root): open(os.path.join(dp, f), "rb").read() for dp, _, fs in os.walk(root) for f in fs}


def test_driver_pileup_command_and_worker(ctx, golden_dir, tmp_path):
    from megagta_amd import api, pileup as pl, synth
    mg = synth.make_metagenome(2000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)
    synth.write_fasta(mg.reads, str(tmp_path / "a.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "a.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "21", "-t", "4", "--min-contig-len", "100", "--derep"]
    out, plain = tmp_path / "with", tmp_path / "plain"
    for o, extra in ((out, ["--pileup", "--min-depth", "2"]), (plain, [])):
        r = subprocess.run(base + ["-o", str(o)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + open(o / "log").read()[-2000:]
    ta, tb = tree(str(out)), tree(str(plain))
    new = {"contigs/rplB/nucl_merged_rmdup_pileup.txt", "contigs/rplB/nucl_merged_rmdup_pileup_variants.txt"}
    assert set(ta) - set(tb) == new and set(tb) <= set(ta)
    for f in set(tb) - {"log", "opts.txt", "tmp/cp.txt"}:
        assert ta[f] == tb[f], f
    cp_a, cp_b = ta["tmp/cp.txt"].decode().splitlines(), tb["tmp/cp.txt"].decode().splitlines()
    assert cp_b == [f"{i}\tdone" for i in range(len(cp_b))] and cp_a == cp_b + [f"{len(cp_b)}\tdone"]      # its checkpoint is the last
    assert "Placing the reads" not in tb["log"].decode() and " pileup " not in tb["log"].decode() and "Placing the reads on the contigs of rplB" in ta["log"].decode()
    # the files: the API's arrays on the run's graph and library, in pileup.py's bytes
    lib = str(out / "tmp" / "reads.lib")
    fa = str(out / "contigs" / "rplB" / "nucl_merged_rmdup.fasta")
    prefix = str(out / "k20" / "20")
    names, seqs = pl.read_fasta(fa)
    assert len(names) >= 1
    g = api.Graph.from_files(ctx, prefix)
    rd = ctx.upload_reads(*readlib.load_for_build(lib))
    res = g.pileup(rd, seqs)
    texts = pl.format_pileup(names, seqs, res, min_depth=2)
    assert texts["summary"].encode() == ta["contigs/rplB/nucl_merged_rmdup_pileup.txt"]
    assert texts["variants"].encode() == ta["contigs/rplB/nucl_merged_rmdup_pileup_variants.txt"]
    rows = pl.parse_summary(texts["summary"])
    assert all(r["reads"] > 0 and r["covered"] > 0 for r in rows)           # the contigs of the search are paths of the reads' graph
    # ... and by comparing strings
    strs = ["".join(DNA[c] for c in r) for r in mg.reads]
    check_result(res, restate(strs, seqs, 20, read_windows(strs, 20)), "the run's contigs")
    # the command alone with other options, and as requests to the worker by matchreads' rules for what it keeps
    res2 = g.pileup(rd, seqs, params=dict(min_anchors=2, min_overlap=40, max_mismatch_permille=10))
    rd.free()
    g.free()
    t2 = pl.format_pileup(names, seqs, res2, min_depth=1, min_alt_permille=1, per_base=True)
    one = str(tmp_path / "one")
    subprocess.run([BIN, "pileup", prefix, lib, fa, one, "--min-anchors", "2", "--min-overlap", "40", "--max-mismatch-permille", "10", "--min-depth", "1",
                    "--min-alt-permille", "1", "--per-base"], check=True, capture_output=True, timeout=120)
    for key, suffix in (("summary", "_pileup.txt"), ("variants", "_pileup_variants.txt"), ("depth", "_pileup_depth.txt")):
        assert open(one + suffix).read() == t2[key], suffix
    assert len(pl.parse_bases(t2["depth"])) == sum(map(len, seqs))
    req = f"matchreads\t{prefix}\t{lib}\t{fa}\t{tmp_path}/w\npileup\t{prefix}\t{lib}\t{fa}\t{tmp_path}/w\t--min-depth\t2\nquit\n"
    r = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0"] * 2, r.stderr[-2000:]
    assert r.stderr.count(f"graph {prefix}: still on the device") == 1 and r.stderr.count("library: still in memory") == 1
    assert open(tmp_path / "w_pileup.txt").read() == texts["summary"] and open(tmp_path / "w_pileup_variants.txt").read() == texts["variants"]
    assert not os.path.exists(tmp_path / "w_pileup_depth.txt")
    r = subprocess.run([BIN, "pileup", prefix, lib, fa], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage: megagta pileup" in r.stderr
    r = subprocess.run([BIN, "pileup", prefix, lib, fa, one, "--min-depth", "x"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "is not a count" in r.stderr
