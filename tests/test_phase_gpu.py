"""Phase (mgta_reads_phase, Context.phase) on the device.

Expected values never come from the code under test.  restate() does the rule of include/megagta_hip.h in Python over strings: per
usable read a dict site -> letter, per fragment the merge of one or two such dicts, Counters for the outputs.  Test 1 gives it
hand-made placements (no graph is needed: the placements are an input), test 2 takes the placements of Graph.pileup on a `-m 1` graph
and compares with that call's own `uniq`, a number another kernel counted."""
import ctypes as C
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from megagta_amd import phase as ph
from megagta_amd import pileup as pl
from megagta_amd import readlib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
DNA = "ACGT"
COMP = str.maketrans("ACGT", "TGCA")
STAT_FIELDS = ("n_reads", "n_usable", "n_fragments", "n_mate_fragments", "n_fragments_allele", "n_fragments_linked", "n_alleles", "n_conflicts",
               "n_pair_adds", "n_sites", "n_pairs")


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


def pair_offsets(sites, span):
    per_site = []
    for pos in sites:
        for u in range(len(pos)):
            per_site.append(sum(1 for v in range(u + 1, len(pos)) if pos[v] - pos[u] < span))
    return [0] + np.cumsum(per_site, dtype=np.int64).tolist() if per_site else [0]


def restate(strs, place, libs, lens, sites, max_span=0):
    """the whole result of Context.phase by comparing strings, in Python integers.  place = list of (contig, diag, orient, n_placed)"""
    span = max_span or 1000
    base = [0]
    for s in sites:
        base.append(base[-1] + len(s))
    pair_off = pair_offsets(sites, span)
    counts, joint, st, census = Counter(), Counter(), Counter(), Counter()

    def letters(r):
        i, d, o, _ = place[r]
        t = rc(strs[r]) if o else strs[r]
        census["negative_diag"] += d < 0
        census["overhang"] += d + len(t) > lens[i]
        census["empty_read_usable"] += len(t) == 0
        return {base[i] + j: t[x - d] for j, x in enumerate(sites[i]) if max(0, d) <= x < min(lens[i], d + len(t))}

    def fragment(reads):
        st["n_fragments"] += 1
        st["n_mate_fragments"] += len(reads) == 2
        maps = [letters(r) for r in reads]
        allele = {}
        for u in sorted(set().union(*maps)):
            seen = {m[u] for m in maps if u in m}
            census["overlap_agree"] += len(maps) == 2 and u in maps[0] and u in maps[1] and len(seen) == 1
            if len(seen) == 1:
                allele[u] = seen.pop()
            else:
                st["n_conflicts"] += 1
        if len(maps) == 2 and maps[0] and maps[1]:
            lo, hi = sorted((min(maps[0]), max(maps[0]), min(maps[1]), max(maps[1])))[1:3]
            census["gap_sites"] += any(lo < u < hi and u not in maps[0] and u not in maps[1] for u in range(lo, hi))
        census["more_than_8"] += len(allele) > 8
        census["more_than_64"] += len(allele) > 64
        st["n_fragments_allele"] += len(allele) >= 1
        st["n_fragments_linked"] += len(allele) >= 2
        st["n_alleles"] += len(allele)
        us = sorted(allele)
        for u in us:
            counts[(u, DNA.index(allele[u]))] += 1
        for a, u in enumerate(us):
            for v in us[a + 1:]:
                if v - u - 1 < pair_off[u + 1] - pair_off[u]:                  # (u, v) is tabled
                    joint[(pair_off[u] + v - u - 1, DNA.index(allele[u]) * 4 + DNA.index(allele[v]))] += 1
                    st["n_pair_adds"] += 1

    first = 0
    for end, paired in libs:
        census["odd_paired_library"] += bool(paired) and (end - first) % 2 == 1
        r = first
        while r < end:
            group = [r, r + 1] if paired and r + 1 < end else [r]
            ok = [q for q in group if place[q][3] == 1]
            st["n_usable"] += len(ok)
            if len(group) == 2:
                census["mate_placed_twice"] += any(place[q][3] > 1 for q in group)
                if len(ok) == 2:
                    census["other_contig"] += place[group[0]][0] != place[group[1]][0]
                    census["same_orient"] += place[group[0]][0] == place[group[1]][0] and place[group[0]][2] == place[group[1]][2]
            if len(ok) == 2 and place[ok[0]][0] == place[ok[1]][0] and place[ok[0]][2] != place[ok[1]][2]:
                fragment(ok)
            else:
                for q in ok:
                    fragment([q])
            r += len(group)
        first = end
    S = base[-1]
    covered = {u for u, _ in counts}
    census["site_uncovered"] = S - len(covered)
    st.update(n_reads=libs[-1][0] if libs else 0, n_sites=S, n_pairs=pair_off[-1])
    sc = np.zeros((S, 4), dtype=np.uint32)
    for (u, b), c in counts.items():
        sc[u, b] = c
    jt = np.zeros((pair_off[-1], 16), dtype=np.uint32)
    for (p, cell), c in joint.items():
        jt[p, cell] = c
    return dict(site_counts=sc, pair_off=np.array(pair_off, dtype=np.uint64), joint=jt, stats={f: int(st[f]) for f in STAT_FIELDS}, census=census)


def place_array(place):
    a = np.zeros(len(place), dtype=pl.READ_DTYPE)
    for r, (i, d, o, n) in enumerate(place):
        a[r] = (7 if n else 0, i, d, o, n, 0)
    return a


def make_inputs(seed=2):
    """Contig 0 (700 letters): eight sites, six of which tell three strains apart: A (the contig), B (all six differ) and R, a
    recombinant with A's letters at the first three and B's at the last three.  Contig 1 (200 letters): 80 sites on adjacent positions,
    two strains.  Contig 2 (120 letters): sites at 0, 60 and 119, the last covered by no read.  Contig 3: no site.  Library 0: paired,
    odd-sized; 1: single-end; 2: empty; 3: paired, on contig 1."""
    rng = np.random.default_rng(seed)
    c0, c1, c2, c3 = rand_dna(rng, 700), rand_dna(rng, 200), rand_dna(rng, 120), rand_dna(rng, 90)
    var = [100, 180, 300, 350, 420, 560]
    strains0 = [c0, subst(c0, var), subst(c0, var[3:])]
    strains1 = [c1, subst(c1, range(20, 100, 3))]
    sites = [[0] + var + [699], list(range(20, 100)), [0, 60, 119], []]
    lens = [700, 200, 120, 90]
    strs, place = [], []

    def add(contig, segment, diag, orient, n_placed=1, junk_left=0, junk_right=0):
        t = rand_dna(rng, junk_left) + segment + rand_dna(rng, junk_right)       # the read in orientation `orient`
        strs.append(rc(t) if orient else t)
        place.append((contig, diag - junk_left, orient, n_placed) if n_placed else (-1, 0, 0, 0))

    def add_pair(contig, s_a, s_b, p, insert, length=80, flip=False, **kw):
        first = (contig, s_a[p:p + length], p, 0)
        second = (contig, s_b[p + insert - length:p + insert], p + insert - length, 1)
        for m in ((second, first) if flip else (first, second)):
            add(*m, **kw)

    for j in range(120):                                                          # 120 pairs, inserts of 250 to 400
        s = strains0[int(rng.choice(3, p=[0.4, 0.35, 0.25]))]
        insert = int(rng.integers(250, 401))
        add_pair(0, s, s, int(rng.integers(0, 700 - insert + 1)), insert, flip=bool(j % 2))
    add_pair(0, strains0[0], strains0[0], 60, 400)                               # 100 | a gap that holds 180, 300, 350 | 420
    add_pair(0, strains0[1], strains0[1], 280, 90)                               # [280, 360) and [290, 370): both mates cover 300 and 350 and agree
    add_pair(0, strains0[0], strains0[1], 280, 90)                               # ... and disagree at both
    add(0, strains0[1][280:360], 280, 0); add(2, c2[0:70], 0, 1)                 # mates on different contigs
    add(0, strains0[1][80:160], 80, 0); add(0, strains0[1][330:410], 330, 0)     # mates in the same orientation
    add(0, strains0[2][90:170], 90, 0); add(0, strains0[2][400:480], 400, 1, n_placed=2)   # a mate placed twice
    add(0, strains0[0][300:380], 300, 1, n_placed=0); add(0, strains0[0][90:190], 90, 0)   # a mate without a placement
    add(0, strains0[1][0:75], 0, 0, junk_left=5); add(0, strains0[1][640:700], 640, 1, junk_right=9)   # a negative diag, an overhang
    add(0, "", 10, 0); add(0, strains0[0][330:430], 330, 1)                      # a read of length 0 that is usable
    add(0, strains0[1][540:620], 540, 0)                                         # the odd last read of the library
    lib0 = len(strs)
    assert lib0 % 2 == 1
    for j in range(150):                                                          # 150 single reads
        s = strains0[int(rng.choice(3, p=[0.4, 0.35, 0.25]))]
        p = int(rng.integers(0, 621))
        add(0, s[p:p + 80], p, j % 2)
    add(2, c2[30:100], 30, 0)
    add(3, c3[5:80], 5, 1)
    add(1, strains1[1][25:55], 25, 1)                                            # 30 adjacent sites on one read
    add(0, "", 0, 0, n_placed=0)
    lib1 = len(strs)
    for j in range(12):                                                           # contig 1: mates that together cover all 80 sites, and shorter ones
        s = strains1[j % 2]
        add_pair(1, s, s, 10, 130, length=80, flip=bool(j % 3 == 0))
        add_pair(1, s, strains1[(j + j // 4) % 2], 5 + j, 100 + 3 * j, length=40)
    add_pair(1, strains1[0], strains1[1], 10, 130)                               # the mates overlap on 30 sites and disagree at every third
    libs = [(lib0, True), (lib1, False), (lib1, True), (len(strs), True)]
    return dict(strs=strs, place=place, libs=libs, lens=lens, sites=sites)


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hand(ctx):
    """the hand-made inputs, their upload and the restatement at the default span and at 150 (computed once, never changed)"""
    d = make_inputs()
    reads = [codes(s) for s in d["strs"]]
    rd = ctx.upload_reads(*readlib.pack_for_build(reads))
    return dict(d, reads=reads, rd=rd, parr=place_array(d["place"]), want=restate(d["strs"], d["place"], d["libs"], d["lens"], d["sites"]),
                want150=restate(d["strs"], d["place"], d["libs"], d["lens"], d["sites"], 150))


def check_result(res, want, what=""):
    assert res["pair_off"].tolist() == want["pair_off"].tolist(), what
    assert res["site_counts"].tolist() == want["site_counts"].tolist(), what
    assert res["joint"].shape == want["joint"].shape and np.array_equal(res["joint"], want["joint"]), what
    assert {f: res["stats"][f] for f in STAT_FIELDS} == want["stats"], what


def stable(stats):
    return {n: v for n, v in stats.items() if not n.startswith("ms_") and n != "peak_bytes"}


def same(a, b, what=""):
    for key in ("site_counts", "pair_off", "joint"):
        assert a[key].tobytes() == b[key].tobytes(), (what, key)
    assert stable(a["stats"]) == stable(b["stats"]), what


# ---- 1. hand-made placements against the restatement --------------------------------------------------------------------------------
def test_hand_made_placements_equal_the_restatement(hand, ctx):
    h = hand
    want, cen = h["want"], h["want"]["census"]
    # the inputs hold what they were made to hold
    assert want["stats"]["n_mate_fragments"] > 100 and want["stats"]["n_fragments"] > want["stats"]["n_mate_fragments"] + 150
    for case in ("overlap_agree", "other_contig", "same_orient", "mate_placed_twice", "odd_paired_library", "negative_diag", "overhang", "empty_read_usable",
                 "more_than_8", "more_than_64", "gap_sites", "site_uncovered"):
        assert cen[case] > 0, (case, cen)
    assert want["stats"]["n_conflicts"] > 0
    assert h["sites"][0][0] == 0 and h["sites"][0][-1] == h["lens"][0] - 1 and want["site_counts"][0].sum() > 0 and want["site_counts"][7].sum() > 0
    assert any(len(s) == 0 for s in h["strs"]) and want["stats"]["n_usable"] < want["stats"]["n_reads"]
    names = ["c0", "c1", "c2", "c3"]
    shape = dict(want, site_off=np.cumsum([0] + [len(s) for s in h["sites"]]), site_pos=np.concatenate([np.array(s, dtype=np.uint32) for s in h["sites"]]))
    rows = [r for r in ph.parse_links(ph.format_phase(names, shape)["links"]) if r["contig"] == "c0"]
    assert {r["phased"] for r in rows} == {0, 1}, rows                         # links both phased and not phased
    alone = restate(h["strs"], h["place"], [(e, False) for e, _ in h["libs"]], h["lens"], h["sites"])
    rows_alone = [r for r in ph.parse_links(ph.format_phase(names, dict(shape, joint=alone["joint"]))["links"]) if r["contig"] == "c0"]
    assert len(rows_alone) < len(rows)                                          # the pairing is what links distant sites
    # the call, reversed as the build uploads the reads and as sequenced
    res = ctx.phase(h["rd"], h["parr"], h["libs"], h["lens"], h["sites"])
    check_result(res, want, "reversed")
    lens = np.array([x.size for x in h["reads"]], dtype=np.uint64)
    start = np.zeros(lens.size + 1, dtype=np.uint64)
    np.cumsum(lens, out=start[1:])
    rd_f = ctx.upload_reads(readlib.pack_codes(np.concatenate(h["reads"])), start)
    res_f = ctx.phase(rd_f, h["parr"], h["libs"], h["lens"], h["sites"], reads_reversed=False)
    rd_f.free()
    check_result(res_f, want, "as sequenced")
    check_result(ctx.phase(h["rd"], h["parr"], h["libs"], h["lens"], h["sites"], params=dict(max_span=150)), h["want150"], "span 150")
    assert h["want150"]["stats"]["n_pairs"] < want["stats"]["n_pairs"] and h["want150"]["stats"]["n_alleles"] == want["stats"]["n_alleles"]
    check_result(ctx.phase(h["rd"], h["parr"], h["libs"], h["lens"], h["sites"], params=dict(max_span=0)), want, "span 0 is the default")
    # the letters may be given in place of the lengths; with n = 0 or no site all outputs are zero
    r0 = ctx.phase(h["rd"], h["parr"], h["libs"], ["A" * n for n in h["lens"]], [[], [], [], []])
    assert r0["site_counts"].size == 0 and r0["joint"].size == 0 and r0["pair_off"].tolist() == [0] and all(v == 0 for v in r0["stats"].values())
    r0 = ctx.phase(h["rd"], h["parr"][:0], [(0, True)], [], [])
    assert r0["pair_off"].tolist() == [0] and all(v == 0 for v in r0["stats"].values())


# ---- 2. against another code path ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph_case(ctx, oracle):
    """about 900 reads of a genome, some with substitutions, every other one as its reverse complement; their -m 1 graph at k = 20"""
    from megagta_amd import api
    k = 20
    rng = np.random.default_rng(23)
    genome = rand_dna(rng, 3000)
    strs = []
    for i in range(900):
        n = int(rng.integers(k + 1, 101))
        p = int(rng.integers(0, 3000 - n + 1))
        s = genome[p:p + n]
        if i % 10 in (3, 5):
            s = subst(s, sorted(set(int(x) for x in rng.integers(0, n, 2))))
        strs.append(rc(s) if i % 2 else s)
    a = genome[400:1000]
    seqs = [a, subst(a, [100, 300, 301, 450]), genome[950:1500]]
    packed, start = readlib.pack_for_build([codes(s) for s in strs])
    rd = ctx.upload_reads(packed, start)
    stream = ctx.build_sdbg(rd, k)
    assert stream.md5() == oracle.Stream.build(packed, start, k, threads=4).edges().md5()
    g = api.Graph(ctx, stream)
    return dict(strs=strs, seqs=seqs, rd=rd, g=g)


def test_row_sums_equal_the_unique_depth_of_pileup(graph_case, ctx):
    c = graph_case
    res = c["g"].pileup(c["rd"], c["seqs"], per_read=True)
    place = res["reads"]
    assert int((place["n_placed"] == 1).sum()) > 100 and int((place["n_placed"] > 1).sum()) > 50      # (about 900 * 550 / 3000 reads lie on the third contig alone)
    sites = [np.arange(len(c["seqs"][0])), [], np.arange(len(c["seqs"][2]))]   # every position of two contigs
    out = ctx.phase(c["rd"], place, [(400, False), (900, False)], c["seqs"], sites, params=dict(max_span=3))
    off = res["offsets"]
    uniq = np.concatenate([res["uniq"][off[0]:off[1]], res["uniq"][off[2]:off[3]]])
    assert uniq.sum() > 3000
    assert out["site_counts"].sum(axis=1).tolist() == uniq.tolist()
    st = out["stats"]
    assert st["n_usable"] == int((place["n_placed"] == 1).sum()) == st["n_fragments"] and st["n_mate_fragments"] == 0 and st["n_conflicts"] == 0
    assert st["n_alleles"] == int(uniq.sum())
    # pairs at distance 1 and 2: the reads placed once that cover both positions, counted from the placements alone
    L = np.array([len(s) for s in c["strs"]])
    n_sites = [len(s) for s in sites]
    want = np.zeros(int(out["pair_off"][-1]), dtype=np.int64)
    base = 0
    for i in (0, 2):
        m = len(c["seqs"][i])
        sel = (place["n_placed"] == 1) & (place["contig"] == i)
        x0 = np.maximum(0, place["diag"][sel].astype(np.int64))
        x1 = np.minimum(m, place["diag"][sel].astype(np.int64) + L[sel])
        for u in range(m):
            for dist in (1, 2):
                if u + dist < m:
                    want[int(out["pair_off"][base + u]) + dist - 1] = int(((x0 <= u) & (u + dist < x1)).sum())
        base += n_sites[i]
    assert out["joint"].sum(axis=1).tolist() == want.tolist()


# ---- 3. what must not move the outputs -----------------------------------------------------------------------------------------------
def test_what_must_not_move_the_outputs(hand, ctx):
    h = hand
    args = (h["libs"], h["lens"], h["sites"])
    a = ctx.phase(h["rd"], h["parr"], *args)
    same(a, ctx.phase(h["rd"], h["parr"], *args), "the call twice")
    ctx.set_phase_chunk(1)
    try:
        one = ctx.phase(h["rd"], h["parr"], *args)
        ctx.set_phase_chunk(7)
        seven = ctx.phase(h["rd"], h["parr"], *args)
    finally:
        ctx.set_phase_chunk(0)
    same(a, one, "chunk 1")
    same(a, seven, "chunk 7")
    # the single-end reads in another order, place permuted the same way
    lib0, lib1 = h["libs"][0][0], h["libs"][1][0]
    order = np.arange(len(h["reads"]))
    order[lib0:lib1] = lib0 + np.random.default_rng(4).permutation(lib1 - lib0)
    assert (order != np.arange(order.size)).sum() > 100
    rd2 = ctx.upload_reads(*readlib.pack_for_build([h["reads"][i] for i in order]))
    r = ctx.phase(rd2, h["parr"][order], *args)
    rd2.free()
    same(a, r, "single-end reads in another order")
    # the contigs in another order: the sites and the pairs of a contig move with it
    perm = [2, 0, 3, 1]
    new_of = {old: new for new, old in enumerate(perm)}
    p2 = h["parr"].copy()
    usable = p2["contig"] >= 0
    p2["contig"][usable] = [new_of[int(i)] for i in p2["contig"][usable]]
    s = ctx.phase(h["rd"], p2, h["libs"], [h["lens"][i] for i in perm], [h["sites"][i] for i in perm])
    assert stable(s["stats"]) == stable(a["stats"])
    for new, old in enumerate(perm):
        ua, ub = int(a["site_off"][old]), int(a["site_off"][old + 1])
        va, vb = int(s["site_off"][new]), int(s["site_off"][new + 1])
        assert s["site_counts"][va:vb].tobytes() == a["site_counts"][ua:ub].tobytes(), (new, old)
        assert s["joint"][int(s["pair_off"][va]):int(s["pair_off"][vb])].tobytes() == a["joint"][int(a["pair_off"][ua]):int(a["pair_off"][ub])].tobytes(), (new, old)
    # a larger max_span: the pairs tabled under both keep their cells
    narrow = ctx.phase(h["rd"], h["parr"], *args, params=dict(max_span=150))
    assert narrow["site_counts"].tobytes() == a["site_counts"].tobytes()
    n_both = 0
    for u in range(len(a["site_pos"])):
        for j in range(int(narrow["pair_off"][u + 1] - narrow["pair_off"][u])):
            assert narrow["joint"][int(narrow["pair_off"][u]) + j].tobytes() == a["joint"][int(a["pair_off"][u]) + j].tobytes(), (u, j)
            n_both += 1
    assert n_both == int(narrow["pair_off"][-1]) > 0 and n_both < int(a["pair_off"][-1])


# ---- 4. limits and errors ------------------------------------------------------------------------------------------------------------
def test_limits_and_errors_leave_the_outputs_untouched(hand, ctx):
    from megagta_amd import _lib, api
    h = hand
    L = _lib.load()
    n_reads = len(h["strs"])
    need = int(h["want"]["pair_off"][-1])

    def call(rh=h["rd"].h, place=h["parr"], ends=(n_reads,), paired=(0,), n_libs=None, lens=h["lens"], sites=h["sites"], cap=need, span=0):
        offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
        np.cumsum(lens, out=offsets[1:])
        site_off = np.zeros(len(sites) + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in sites], out=site_off[1:])
        site_pos = np.concatenate([np.array(s, dtype=np.uint32) for s in sites])
        ends_a, paired_a = np.array(ends, dtype=np.uint64), np.array(paired, dtype=np.uint8)
        counts = np.full((site_pos.size, 4), 7, dtype=np.uint32)
        pair_off = np.full(site_pos.size + 1, 7, dtype=np.uint64)
        joint = np.full((max(1, cap), 16), 7, dtype=np.uint32)
        st = _lib.PhaseStats()
        st.n_reads = 7
        par = _lib.PhaseParams(span)
        place = np.ascontiguousarray(place)
        code = L.mgta_reads_phase(rh, 1, place.ctypes.data, ends_a.ctypes.data, paired_a.ctypes.data, len(ends) if n_libs is None else n_libs, offsets.ctypes.data,
                                  len(lens), site_off.ctypes.data, site_pos.ctypes.data, C.byref(par), counts.ctypes.data, pair_off.ctypes.data, joint.ctypes.data, cap,
                                  C.byref(st))
        untouched = bool((counts == 7).all() and (pair_off == 7).all() and (joint == 7).all() and st.n_reads == 7)
        return code, L.mgta_last_error(), untouched

    assert call()[0] == 0 and not call()[2]                                    # the call as the cases below change it
    bad = [list(s) for s in h["sites"]]
    bad[0][2], bad[0][3] = bad[0][3], bad[0][2]
    cases = [(dict(sites=bad), b"ascend"),
             (dict(sites=[h["sites"][0][:-1] + [700]] + h["sites"][1:]), b"below the contig's length"),
             (dict(sites=h["sites"][:3] + [[90]]), b"below the contig's length"),
             (dict(ends=(10, 5), paired=(0, 0)), b"lib_end"),
             (dict(ends=(n_reads + 1,)), b"the library holds"),
             (dict(n_libs=0), b"n_libs"),
             (dict(ends=(n_reads,) * 257, paired=(0,) * 257), b"n_libs"),
             (dict(cap=need - 1), b"joint_cap >= %d is needed" % need),
             (dict(span=-1), b"max_span"),
             (dict(rh=None), b"NULL")]
    for field, value in (("contig", 4), ("contig", -1)):
        p = h["parr"].copy()
        r = int(np.flatnonzero(p["n_placed"] == 1)[5])
        p[field][r] = value
        cases.append((dict(place=p), b"contig < n"))
    for kw, word in cases:
        code, msg, untouched = call(**kw)
        assert code == -1 and word in msg and untouched, (kw.keys(), msg)
    p = h["parr"].copy()
    p["contig"][np.flatnonzero(p["n_placed"] != 1)] = 99                       # a record that is not usable is not looked at
    assert call(place=p)[0] == 0
    # a read of 65 536 bases
    long_rd = ctx.upload_reads(*readlib.pack_for_build([codes(h["strs"][0]), np.zeros(65536, dtype=np.uint8)]))
    code, msg, untouched = call(rh=long_rd.h, place=h["parr"][:2], ends=(2,))
    long_rd.free()
    assert code == -1 and b"65535" in msg and untouched
    # a handle of another context
    other = api.Context(0)
    try:
        rd2 = other.upload_reads(*readlib.pack_for_build(h["reads"][:50]))
        with pytest.raises(api.MegaGtaError, match="another context"):
            ctx.phase(rd2, h["parr"][:50], [(50, False)], h["lens"], h["sites"])
        rd2.free()
    finally:
        other.close()
    with pytest.raises(api.MegaGtaError, match=r"\(-1\).*joint_cap"):
        ctx.phase(h["rd"], h["parr"], h["libs"], h["lens"], h["sites"], joint_cap=need - 1)


# ---- 5. the command, the worker and the driver ----------------------------------------------------------------------------------------
def tree(root):
    return {os.path.relpath(os.path.join(dp, f), root): open(os.path.join(dp, f), "rb").read() for dp, _, fs in os.walk(root) for f in fs}


def test_driver_phase_command_and_worker(ctx, golden_dir, tmp_path):
    from megagta_amd import api, synth
    mg = synth.make_metagenome(2000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)
    synth.write_fasta(mg.reads, str(tmp_path / "a.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    common = ["-g", str(tmp_path / "gene_list.txt"), "-k", "21", "-t", "4", "--min-contig-len", "100", "--derep", "--pileup", "--min-depth", "2"]
    single, inter = ["-r", str(tmp_path / "a.fa")], ["--12", str(tmp_path / "a.fa")]
    runs = dict(plain=(single, []), se=(single, ["--phase", "--min-link", "1"]), pe=(inter, ["--phase", "--min-link", "1"]))
    trees = {}
    for name, (reads, extra) in runs.items():
        o = tmp_path / name
        r = subprocess.run([sys.executable, DRIVER] + reads + common + ["-o", str(o)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + open(o / "log").read()[-2000:]
        trees[name] = tree(str(o))
    new = {"contigs/rplB/nucl_merged_rmdup_phase_links.txt", "contigs/rplB/nucl_merged_rmdup_phase_blocks.txt"}
    varies = {"log", "opts.txt"}
    names_lib = {"tmp/reads.lib", "tmp/reads.lib.lib_info"}                     # what says how the reads were given
    for name in ("se", "pe"):
        ta, tb = trees[name], trees["plain"]
        assert set(ta) - set(tb) == new and set(tb) <= set(ta), name
        for f in set(tb) - varies - (names_lib if name == "pe" else set()):
            assert ta[f] == tb[f], (name, f)                                    # tmp/cp.txt too: the files belong to the pileup step
    assert b" pe" in trees["pe"]["tmp/reads.lib.lib_info"] and b" se" in trees["se"]["tmp/reads.lib.lib_info"]
    assert "--phase" not in trees["plain"]["log"].decode() and "--phase" in trees["se"]["log"].decode()
    # the files: the API's arrays on the run's graph and library with the run's .lib_info, in phase.py's bytes
    fa = str(tmp_path / "se" / "contigs" / "rplB" / "nucl_merged_rmdup.fasta")
    names, seqs = pl.read_fasta(fa)
    texts, libdirs = {}, {}
    for name in ("se", "pe"):
        lib = str(tmp_path / name / "tmp" / "reads.lib")
        prefix = str(tmp_path / name / "k20" / "20")
        g = api.Graph.from_files(ctx, prefix)
        rd = ctx.upload_reads(*readlib.load_for_build(lib))
        res = g.pileup(rd, seqs, per_read=True)
        libs = [(to + 1, pe) for _, _, to, _, pe in readlib.read_lib_table(lib)]
        assert [p for _, p in libs] == [name == "pe"]
        sites = ph.sites_from_pileup(seqs, res, min_depth=2)
        out = ctx.phase(rd, res["reads"], libs, seqs, sites)
        rd.free()
        g.free()
        texts[name] = ph.format_phase(names, out, min_link=1)
        libdirs[name] = (prefix, lib)
        assert texts[name]["links"].encode() == trees[name]["contigs/rplB/nucl_merged_rmdup_phase_links.txt"], name
        assert texts[name]["blocks"].encode() == trees[name]["contigs/rplB/nucl_merged_rmdup_phase_blocks.txt"], name
        assert sum(map(len, sites)) == len(pl.parse_bases(trees[name]["contigs/rplB/nucl_merged_rmdup_pileup_variants.txt"].decode()))
        # the mates of the interleaved file are consecutive reads: those that form one fragment, counted from the placements
        a, b = res["reads"][0::2], res["reads"][1::2]
        joined = int(((a["n_placed"] == 1) & (b["n_placed"] == 1) & (a["contig"] == b["contig"]) & (a["orient"] != b["orient"])).sum())
        assert out["stats"]["n_mate_fragments"] == (joined if name == "pe" else 0)
        assert out["stats"]["n_fragments"] == int((res["reads"]["n_placed"] == 1).sum()) - out["stats"]["n_mate_fragments"]
    assert len(ph.parse_links(texts["se"]["links"])) > 0
    # the command alone with other options, and the same argv as a request to the worker
    prefix, lib = libdirs["pe"]
    one, w = str(tmp_path / "one"), str(tmp_path / "w")
    argv = [prefix, lib, fa, None, "--min-depth", "2", "--phase", "--max-span", "40", "--min-link", "2", "--min-hap-permille", "200"]
    subprocess.run([BIN, "pileup"] + [a or one for a in argv], check=True, capture_output=True, timeout=120)
    req = "pileup\t" + "\t".join(a or w for a in argv) + "\nquit\n"
    r = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0"], r.stderr[-2000:]
    for suffix in ("_pileup.txt", "_pileup_variants.txt", "_phase_links.txt", "_phase_blocks.txt"):
        assert open(one + suffix, "rb").read() == open(w + suffix, "rb").read(), suffix
    links40 = ph.parse_links(open(one + "_phase_links.txt").read())
    assert all(r["pos2"] - r["pos1"] < 40 and r["fragments"] >= 2 for r in links40)
    r = subprocess.run([BIN, "pileup", prefix, lib, fa, one, "--max-span", "40"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage: megagta pileup" in r.stderr
