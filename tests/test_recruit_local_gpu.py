"""Local read recruitment (Context.recruit(params=dict(local=True)) / `megagta recruit --local` / `megagta.py --recruit --recruit-local`).

The device against the yardstick in plain Python (tests/recruit_local_ref.py) on every read and every field: the score in its 8 bytes,
the hit bits, the column depth and the stats that are functions of the input.  On the small cases the score, model_to and the end of the
span are also checked against the device's own Context.align over every substring of every stretch (stretches of at most 40
residues).  Every test of mode 1 fails on a library that ignores the mode: it would return the global rule's records."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from megagta_amd import hmm as H
from megagta_amd import synth
from megagta_amd import recruit as rc
from tests import helpers
from tests import recruit_local_ref as lref
from tests import recruit_ref as ref
from tests import rich_models as R
from tests import test_recruit_gpu as TR
from tests.test_recruit_gpu import BIN, BITS20, DRIVER, NEG, SENSE, VOLATILE, assert_is, codons, coding, eight, gene_read, protein, revcomp, upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def models(ctx, tmp_path_factory):
    return TR.Models(ctx, str(tmp_path_factory.mktemp("recruit_local_models")))


def sense(rng, n):
    """base codes of n codons at random, none of them a stop"""
    return np.array([[c >> 4, (c >> 2) & 3, c & 3] for c in rng.choice(SENSE, n)], dtype=np.uint8).reshape(-1)


def with_tables(ctx, hm, msc=None, tsc=None):
    """a model with these tables in place of the parsed ones, and its copy on the device"""
    from megagta_amd import api
    hm = copy.copy(hm)
    if msc is not None:
        hm.msc = np.array(msc, dtype=np.float64)
    if tsc is not None:
        hm.tsc = np.array(tsc, dtype=np.float64)
    return hm, api.DeviceHmm(ctx, hm), None


def run_local(ctx, model, reads, min_aa=20, min_score=BITS20, what="", reversed_storage=True, n_short=None, want=None):
    """the device in local mode against the yardstick on every read -> (device, yardstick)"""
    hm, dev, _ = model
    rd, _, _ = upload(ctx, reads, reversed_storage)
    try:
        got = ctx.recruit(dev, rd, n_short_reads=n_short, params=dict(min_aa=min_aa, min_score=min_score, local=True), reads_reversed=reversed_storage)
    finally:
        rd.free()
    if want is None:
        want = lref.recruit(hm, reads if n_short is None else reads[:n_short], min_aa, min_score)
    assert_is(got, want, what + " (local)")
    return got, want


def run_global(ctx, model, reads, min_aa=20, min_score=BITS20):
    hm, dev, _ = model
    rd, _, _ = upload(ctx, reads)
    try:
        return ctx.recruit(dev, rd, params=dict(min_aa=min_aa, min_score=min_score))
    finally:
        rd.free()


def check_against_align(ctx, model, got, want, what=""):
    """score, model_to and the end of the span of every placed read against the device's own mgta_seqs_align over every substring of
    every stretch of the read: the highest score; then the earlier stretch, the lowest end column, the lowest end row.  A read with a
    stretch of more than 40 residues is left out (its substrings are too many) -> the reads that were checked"""
    hm, dev, _ = model
    too_long = {s[0] for s in want["stretches"] if s[3] > 40}
    seqs, owner = [], []
    for k, (r, f, a, n, res) in enumerate(want["stretches"]):
        if r in too_long:
            continue
        for b in range(1, n + 1):
            for a0 in range(b):
                seqs.append(res[a0:b])
                owner.append((r, k, a + b))
    recs = ctx.align(dev, seqs, cols=False, paths=False)["recs"]
    best = {}
    for (r, k, end), rec in zip(owner, recs):
        if int(rec["status"]) != 0:
            continue
        key = (-float(rec["score"]), k, int(rec["model_to"]), end)
        if r not in best or key < best[r]:
            best[r] = key
    n = 0
    for i, rec in enumerate(got["recs"]):
        if i in too_long:
            continue
        if int(rec["status"]) == 0:
            score, _, m_to, end = best[i]
            assert eight(rec["score"]) == eight(-score) and int(rec["model_to"]) == m_to and int(rec["aa_from"]) + int(rec["aa_len"]) == end, (what, i)
            n += 1
        else:
            assert i not in best, (what, i)
    return n


# ---- 1. overhangs ----------------------------------------------------------------------------------------------------------------------
def overhang_case():
    """-> (gene of 120 residues, gene of 9, reads over the long gene's ends, reads over the short gene, what each must give): frame 0 of
    every read is the designed one; 40 residues at most between two stops"""
    rng = np.random.default_rng(5)
    prot = protein(rng, 120)
    short = protein(rng, 9)
    stop = codons("TAA")
    long_reads = [np.concatenate([sense(rng, 30), coding(rng, prot[:10])]),                          # 5' flank without a stop, 10 residues of the gene
                  np.concatenate([sense(rng, 28), coding(rng, prot[:12])]),                          # ... 12
                  np.concatenate([coding(rng, prot[110:]), stop, sense(rng, 25)]),                   # 3' end, the gene's stop, a longer run behind it
                  np.concatenate([coding(rng, prot[108:]), codons("TGA"), sense(rng, 27)])]
    long_want = [(1, 10, 30, 10), (1, 12, 28, 12), (111, 120, 0, 10), (109, 120, 0, 12)]     # model_from, model_to, aa_from, aa_len
    short_reads = [np.concatenate([sense(rng, 20), coding(rng, short), stop, sense(rng, 10)]),       # both ends: a flank, the gene, its stop, a run behind it
                   np.concatenate([sense(rng, 12), coding(rng, short), stop, sense(rng, 18)]),       # ... the run behind it the longer one
                   np.concatenate([sense(rng, 15), coding(rng, short), sense(rng, 16)]),             # a gene shorter than the read, no stop at all
                   np.concatenate([codons("TAG"), sense(rng, 12), coding(rng, short), sense(rng, 18)])]
    short_want = [(1, 9, 20, 9), (1, 9, 12, 9), (1, 9, 15, 9), (1, 9, 13, 9)]
    return prot, short, long_reads, long_want, short_reads, short_want


def test_overhangs_are_recruited_locally_and_not_globally(ctx, models):
    prot, short, long_reads, long_want, short_reads, short_want = overhang_case()
    for name, gene, reads, wants in (("over120", prot, long_reads, long_want), ("over9", short, short_reads, short_want)):
        model = models.of_protein(gene, name)
        hm = model[0]
        reads = reads + [revcomp(r) for r in reads]                          # and each on the other strand: frame 3
        glob_ref = ref.recruit(hm, reads, 8, BITS20)
        assert not glob_ref["bits"].any(), name                              # by the global yardstick none reaches 20 bits
        got, want = run_local(ctx, model, reads, min_aa=8, what=name)
        assert want["bits"].all() and got["bits"].all(), name                # by the local one, and on the device, all do
        for i, (m_from, m_to, a, n) in enumerate(wants + wants):
            r = got["recs"][i]
            assert (int(r["frame"]), int(r["model_from"]), int(r["model_to"]), int(r["aa_from"]), int(r["aa_len"])) == (0 if i < len(wants) else 3, m_from, m_to, a, n), (name, i)
            assert float(r["score"]) / ref.LN2 >= 30.0, (name, i)
        glob = run_global(ctx, model, reads, min_aa=8)
        assert not glob["bits"].any() and glob["stats"]["n_recruited"] == 0, name
        for g, l in zip(glob["recs"], got["recs"]):                          # per read the local score is at least the global one
            assert float(l["score"]) >= float(g["score"])
        assert check_against_align(ctx, model, got, want, name) == len(reads)
        print(name, "bits global", [round(float(s) / ref.LN2, 1) for s in glob["recs"]["score"]], "local", [round(float(s) / ref.LN2, 1) for s in got["recs"]["score"]])


# ---- 2. strip edges --------------------------------------------------------------------------------------------------------------------
def width_reads(rng, prot):
    reads = [gene_read(rng, prot, int(rng.integers(60, 153))) for _ in range(30)] + [rng.integers(0, 4, int(rng.integers(60, 153)), dtype=np.uint8) for _ in range(8)]
    M = len(prot)
    if M > 64:                                                               # entry in one strip of 64 columns, end in a later one, flanks on both sides
        reads += [np.concatenate([sense(rng, 6), coding(rng, prot[50:min(M, 90)]), sense(rng, 5)]), revcomp(np.concatenate([sense(rng, 3), coding(rng, prot[40:M])]))]
    if M > 128:
        reads.append(np.concatenate([sense(rng, 4), coding(rng, prot[55:M]), codons("TAA"), sense(rng, 30)]))
    return reads


@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 128, 129])
def test_model_widths(ctx, models, M):
    rng = np.random.default_rng(700 + M)
    prot = protein(rng, M)
    model = models.of_protein(prot, f"lwidth{M}")
    if M <= 2:
        reads = [coding(rng, prot), np.concatenate([codons("TAA"), coding(rng, prot), codons("TGA")]), revcomp(coding(rng, prot)), codons("AAAAAC"), codons("A" * 27),
                 np.concatenate([sense(rng, 5), coding(rng, prot), sense(rng, 6)]), rng.integers(0, 4, 40, dtype=np.uint8)]
        got, want = run_local(ctx, model, reads, min_aa=1, min_score=NEG, what=f"M={M}")
        assert want["recs"][0]["status"] == 0 and (want["recs"][5]["model_from"], want["recs"][5]["model_to"]) == (1, M)
        assert all(w["status"] == 0 for w in want["recs"])                   # one column takes one residue of any stretch: nothing is unaligned
        if M == 1:
            assert all(w["aa_len"] == 1 for w in want["recs"])
        check_against_align(ctx, model, got, want, f"M={M}")
    else:
        got, want = run_local(ctx, model, width_reads(rng, prot), what=f"M={M}")
        assert want["stats"]["n_recruited"] >= 10 and want["stats"]["n_recruited"] < len(want["recs"])
        assert any(w["model_from"] > 1 for w in want["recs"]) and any(0 < w["model_to"] < M for w in want["recs"])
        if M > 64:
            assert any(w["status"] == 0 and w["model_from"] <= 64 < w["model_to"] for w in want["recs"][-3:])
        if M > 128:
            assert want["recs"][-1]["model_from"] <= 64 and want["recs"][-1]["model_to"] == 129
    assert got["stats"]["msc_in_lds"] == 1 and got["stats"]["waves_per_block"] == 4


# ---- 3. stretches per frame, slot flushes ----------------------------------------------------------------------------------------------
def test_stretches_per_frame_and_equal_peptides(ctx, models):
    rng = np.random.default_rng(83)
    prot = "K" * 30 + protein(rng, 34)
    model = models.of_protein(prot, "lties64")
    gene = lambda a, n: coding(rng, prot[a:a + n])
    pep = gene(34, 22)
    reads = [codons(*["TAA"] * 25),                                                          # 0: no stretch in frame 0
             np.concatenate([codons("TAA"), gene(33, 30)]),                                  # 1: one
             np.concatenate([gene(30, 22), codons("TAG"), gene(40, 23)]),                    # 2: two, the second better by a residue
             np.concatenate([gene(30, 21), codons("TAG"), gene(35, 25), codons("TGA"), gene(31, 20)]),   # 3: three, the middle one the best
             np.concatenate([pep, codons("TAA"), pep]),                                      # 4: two equal peptides in one frame
             np.concatenate([gene(30, 19), codons("TAA"), gene(38, 19), codons("TAA"), gene(44, 20)]),   # 5: two below min_aa, the last alone scored
             codons("A" * 62), revcomp(codons("A" * 62))]                                    # 6, 7: the same peptide in frames 0 .. 2, 3 .. 5
    got, want = run_local(ctx, model, reads, min_score=NEG, what="stretches")
    per_f0 = [[s[2:4] for s in want["stretches"] if s[0] == i and s[1] == 0] for i in range(6)]
    assert [len(x) for x in per_f0] == [0, 1, 2, 3, 2, 1] and per_f0[5] == [(40, 20)] and per_f0[3] == [(0, 21), (22, 25), (48, 20)]
    w = want["recs"]
    assert (w[2]["frame"], w[2]["aa_from"], w[2]["aa_len"]) == (0, 23, 23) and (w[3]["frame"], w[3]["aa_from"], w[3]["aa_len"]) == (0, 22, 25)
    assert eight(want["scores"][[s[:3] for s in want["stretches"]].index((4, 0, 0))][0]) == eight(want["scores"][[s[:3] for s in want["stretches"]].index((4, 0, 23))][0])
    assert (w[4]["frame"], w[4]["aa_from"], w[4]["aa_len"]) == (0, 0, 22)                     # the lower aa_from
    assert ref.frames(reads[6])[:3] == ["K" * 20] * 3 and w[6]["frame"] == 0 and w[7]["frame"] == 3   # the lower frame
    assert check_against_align(ctx, model, got, want, "stretches") >= 4   # (the reads without a stretch of more than 40 residues in any frame)


def test_slot_flushes_long_stretches_and_the_longest_read(ctx, models):
    rng = np.random.default_rng(84)
    prot = protein(rng, 5)
    model = models.of_protein(prot, "lfive")
    hm, dev, _ = model
    every_other = codons(*["AAA", "TAA"] * 40)                               # frame 0: K * K * ...: 40 stretches of one residue
    assert ref.frames(every_other)[0] == "K*" * 40
    many = [np.concatenate([coding(rng, prot), codons("TAA")] * 6) for _ in range(70)]      # six stretches and more per read: a grab of 64 reads fills the 64 slots several times
    reads = many[:3] + [every_other, revcomp(every_other)] + many[3:]
    ctx.set_recruit_chunk(64)
    try:
        got, want = run_local(ctx, model, reads, min_aa=1, min_score=NEG, what="flushes")
    finally:
        ctx.set_recruit_chunk(0)
    assert got["stats"]["chunk"] == 64 and sum(s[0] < 64 for s in want["stretches"]) > 5 * 64
    assert sum(s[0] == 3 and s[1] == 0 for s in want["stretches"]) == 40 and want["recs"][3]["status"] == 0
    # a stretch longer than the 256 rows, the gene in its middle; the longest read there is: 4096 residues in frame 2
    body = sense(rng, 4096)
    body[3 * 2000:3 * 2005] = coding(rng, prot)
    longest = np.concatenate([codons("TA"), body])
    mid = sense(rng, 300)
    mid[3 * 140:3 * 145] = coding(rng, prot)
    assert len(longest) == ref.MAX_BASES
    reads = [gene_read(rng, prot, 150), mid, np.concatenate([codons("TAA"), coding(rng, prot), codons("TAA")]), longest]
    got3, want3 = run_local(ctx, model, reads[:3], min_aa=4, what="long stretch")
    assert (1, 0, 0, 300) in [s[:4] for s in want3["stretches"]] and got3["stats"]["rows_per_wave"] == 304
    got4, want4 = run_local(ctx, model, reads, min_aa=4, what="longest")
    assert (3, 2, 0, 4096) in [s[:4] for s in want4["stretches"]] and got4["stats"]["rows_per_wave"] == 4096 and got4["stats"]["waves_per_block"] == 1
    assert want4["recs"][3]["status"] == 0 and got4["recs"][:3].tobytes() == got3["recs"].tobytes()
    # one base more: refused with the read's number, nothing written
    from megagta_amd import api
    L = ctx._L
    rd, _, _ = upload(ctx, [reads[0], np.concatenate([longest, codons("A")])])
    try:
        bits, recs, depth = np.full(1, 77, dtype=np.uint64), np.zeros(2, dtype=rc.REC), np.full(hm.M, 77, dtype=np.uint64)
        recs.view(np.uint8)[:] = 77
        par = api._lib.RecruitParams()
        par.min_aa, par.mode, par.min_score = 4, 1, BITS20
        assert L.mgta_reads_recruit(ctx.h, dev.h, rd.h, 1, 2, C.byref(par), bits.ctypes.data, recs.ctypes.data, depth.ctypes.data, None) == -1
        assert b"read 1 " in L.mgta_last_error() and str(ref.MAX_BASES).encode() in L.mgta_last_error()
        assert (bits == 77).all() and (recs.view(np.uint8) == 77).all() and (depth == 77).all()
    finally:
        rd.free()


# ---- 4. ties, 5. -inf ------------------------------------------------------------------------------------------------------------------
def test_ties_lowest_column_then_lowest_row_and_b_wins(ctx, models):
    rng = np.random.default_rng(85)
    base = models.of_protein("K" * 6, "lsix")[0]
    k = int(base.alpha[ord("K")])
    # every column emits 1 for K and -3 for anything else, every transition costs nothing: a run of K reaches any score in many cells
    msc = np.full_like(base.msc, -3.0)
    msc[:, k] = 1.0
    msc[0] = 0.0
    flat = with_tables(ctx, base, msc, np.zeros_like(base.tsc))
    reads = [codons("AAA" * 3, "TAA", "AAA" * 8), codons("AAA" * 9), codons("ACG", "AAA" * 7, "ACG", "AAA" * 7), codons("A" * 25), revcomp(codons("A" * 25))]
    got, want = run_local(ctx, flat, reads, min_aa=1, min_score=NEG, what="flat")
    # nine K over six columns: 6 = the six columns in a row, first reached in row 6 of column 6 by the path that entered at row 1
    assert want["scores"][[s[:3] for s in want["stretches"]].index((1, 0, 0))] == (6.0, 1, 6, 0, 6)
    assert (want["recs"][0]["aa_from"], want["recs"][0]["aa_len"], want["recs"][0]["model_from"], want["recs"][0]["model_to"]) == (4, 6, 1, 6)
    assert (want["recs"][3]["frame"], want["recs"][4]["frame"]) == (0, 3)
    assert check_against_align(ctx, flat, got, want, "flat") == len(reads)
    # a continuing candidate of exactly 0.0: column 1 emits 0 for K, so VM[2][2] may continue from (1, 1) with 0 + 0 or enter: B wins,
    # and the span is one residue in column 2 (the lowest column that reaches 1, its lowest row)
    msc0 = msc.copy()
    msc0[1, k] = 0.0
    zero = with_tables(ctx, base, msc0, np.zeros_like(base.tsc))
    got0, want0 = run_local(ctx, zero, [codons("AAA", "AAA")], min_aa=2, min_score=NEG, what="zero")
    assert want0["scores"][0] == (2.0, 2, 3, 0, 2)
    check_against_align(ctx, zero, got0, want0, "zero")
    # the same on two columns and the residues N K, where it shows in the record: column 1 emits 0 for N, column 2 emits 1 for K, so
    # VM[2][2] = 1 either way -- entered there (span K alone, model_from 2) or continued from (1, 1) (span N K, model_from 1)
    base2 = models.of_protein("NK", "ltwo")[0]
    n2, k2 = int(base2.alpha[ord("N")]), int(base2.alpha[ord("K")])
    m2 = np.full_like(base2.msc, -3.0)
    m2[0], m2[1, n2], m2[2, n2], m2[2, k2] = 0.0, 0.0, -1.0, 1.0
    for e11, rec in ((0.0, (1.0, 2, 2, 1, 1)), (0.5, (1.5, 1, 2, 0, 2))):   # a candidate of 0.5 does continue
        m2[1, n2] = e11
        model = with_tables(ctx, base2, m2, np.zeros_like(base2.tsc))
        got2, want2 = run_local(ctx, model, [codons("AAC", "AAA")], min_aa=2, min_score=NEG, what=f"B against {e11}")
        w = want2["recs"][0]
        assert (w["score"], w["model_from"], w["model_to"], w["aa_from"], w["aa_len"], w["frame"]) == rec + (0,)
        check_against_align(ctx, model, got2, want2, f"B against {e11}")
    # whole-number tables at random, with stars: ties of every kind, -inf in match and transition tables
    for t in range(3):
        m = rng.integers(-2, 3, base.msc.shape).astype(np.float64)
        tr = rng.integers(-2, 1, base.tsc.shape).astype(np.float64)
        m[rng.random(m.shape) < 0.15] = NEG
        tr[rng.random(tr.shape) < 0.2] = NEG
        m[0] = 0.0
        model = with_tables(ctx, base, m, tr)
        reads = [rng.integers(0, 4, int(n), dtype=np.uint8) for n in rng.integers(3, 100, 40)]
        got, want = run_local(ctx, model, reads, min_aa=1, min_score=NEG, what=f"whole {t}")
        assert check_against_align(ctx, model, got, want, f"whole {t}") > 30
        assert not any(np.isnan(got["recs"]["score"]))


def test_minus_infinity(ctx, models):
    rng = np.random.default_rng(86)
    prot = protein(rng, 40)
    stars = [(j, x) for j in range(1, 41) for x in (ref.MI, ref.MD)] + [(20, ref.MM)]       # no gaps, and no way from column 20 to 21
    model = models.from_text("lstar40", TR.with_stars(synth.hmm_text("s", prot), match_stars=[(j, prot[j - 1]) for j in (5, 30)], trans_stars=stars))
    hm = model[0]
    assert hm.tsc[ref.MM, 20] == NEG and hm.msc[5][hm.alpha[ord(prot[4])]] == NEG
    reads = [coding(rng, prot), coding(rng, prot[10:35]), np.concatenate([sense(rng, 8), coding(rng, prot[15:26]), sense(rng, 8)]), revcomp(coding(rng, prot[0:21])),
             coding(rng, prot[0:12]), np.concatenate([codons("TAA"), coding(rng, prot[18:40])])]
    got, want = run_local(ctx, model, reads, min_aa=8, min_score=NEG, what="stars")
    assert all(w["status"] == 0 and not w["model_from"] <= 20 < w["model_to"] for w in want["recs"])
    assert [(w["model_from"], w["model_to"]) for w in want["recs"]] == [(6, 20), (11, 20), (21, 26), (6, 20), (6, 12), (31, 40)]   # the longest piece between two stars
    assert check_against_align(ctx, model, got, want, "stars") == len(reads)
    # every match emission a star: every stretch is scored and none has a score: status 1, the whole first scored stretch, not recruited at -inf
    dead = with_tables(ctx, hm, np.vstack([hm.msc[:1], np.full_like(hm.msc[1:], NEG)]))
    reads = [np.concatenate([codons("TAA"), sense(rng, 9), codons("TAG"), sense(rng, 12)]), sense(rng, 30), codons("TAATAATAA")]
    got, want = run_local(ctx, dead, reads, min_aa=8, min_score=NEG, what="dead")
    assert [w["status"] for w in want["recs"]] == [1, 1, 2] and (want["recs"][0]["frame"], want["recs"][0]["aa_from"], want["recs"][0]["aa_len"]) == (0, 1, 9)
    assert not got["bits"].any() and got["stats"]["n_unaligned"] == 2 and got["stats"]["n_unscored"] == 1 and not any(np.isnan(got["recs"]["score"]))


# ---- 6. other paths and guards ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [65, 129])
def test_position_specific_models(ctx, models, M):
    cons, text, seed = R.rich_protein_model(M)
    model = models.from_text(f"lrich{M}", text)
    seqs = [s for _, s in R.rich_sequences(model[0], cons, seed)]
    reads = R.rich_reads(seqs, seed)
    got, want = run_local(ctx, model, reads, min_aa=1, min_score=NEG, what=f"rich {M}")
    run_local(ctx, model, reads, min_aa=1, min_score=NEG, what=f"rich {M}, stored as sequenced", reversed_storage=False, want=want)   # both storage orders
    assert {w["frame"] for w in want["recs"] if w["status"] == 0} == set(range(6))
    assert any(w["model_from"] > 1 for w in want["recs"]) and any(0 < w["model_to"] < M for w in want["recs"])


def test_golden_model_that_does_not_fit_lds(ctx, models, tmp_path):
    mg, gdir = helpers.bigm_inputs("m1200", str(tmp_path))
    model = models.from_text("lm1200", open(os.path.join(gdir, "for_enone.hmm")).read())
    reads = [r[:75] for r in mg.reads[:60]]                                 # (25 residues a frame: the plain-Python yardstick takes seconds on 1200 columns)
    got, want = run_local(ctx, model, reads, min_aa=12, what="M=1200")
    assert got["stats"]["msc_in_lds"] == 0 and model[0].M == 1200          # the match scores are read from device memory
    assert 2 <= want["stats"]["n_recruited"] < 60


def test_prefix_chunks_repeats_and_modes(ctx, models):
    from megagta_amd import api
    rng = np.random.default_rng(87)
    prot = protein(rng, 100)
    model = models.of_protein(prot, "lchunk100")
    hm, dev, _ = model
    reads = [gene_read(rng, prot, int(rng.integers(60, 153))) for _ in range(70)] + [rng.integers(0, 4, int(n), dtype=np.uint8) for n in (0, 1, 2, 5, 59, 60, 61, 150, 1000)]
    want = lref.recruit(hm, reads)
    rd, _, _ = upload(ctx, reads)
    outs = {}
    L = ctx._L
    try:
        outs["default"] = ctx.recruit(dev, rd, params=dict(local=True))
        outs["again"] = ctx.recruit(dev, rd, params=dict(mode=1))
        for chunk in (1, 3, 64):
            ctx.set_recruit_chunk(chunk)
            outs[chunk] = ctx.recruit(dev, rd, params=dict(local=True))
        ctx.set_recruit_chunk(0)
        for name, res in outs.items():
            assert_is(res, want, f"chunk {name}")
            for f in ("hit_bits", "recs", "col_depth"):
                assert res[f].tobytes() == outs["default"][f].tobytes(), (name, f)
            assert {k: v for k, v in res["stats"].items() if k not in VOLATILE} == {k: v for k, v in outs["default"]["stats"].items() if k not in VOLATILE}
        # the reads behind n_short_reads have no bit and no record
        cut = ctx.recruit(dev, rd, n_short_reads=40, params=dict(local=True))
        assert_is(cut, lref.recruit(hm, reads[:40]), "n_short")
        assert cut["recs"].tobytes() == outs["default"]["recs"][:40].tobytes()
        # mode 0 given explicitly gives the bytes of params = NULL, and is not the local answer
        n, words = len(reads), (len(reads) + 63) // 64
        by = {}
        for name in ("null", "zero"):
            bits, recs, depth, st = np.zeros(words, dtype=np.uint64), np.zeros(n, dtype=rc.REC), np.zeros(hm.M, dtype=np.uint64), api._lib.RecruitStats()
            par = api._lib.RecruitParams()
            par.min_aa, par.mode, par.min_score = 20, 0, BITS20
            assert L.mgta_reads_recruit(ctx.h, dev.h, rd.h, 1, n, None if name == "null" else C.byref(par), bits.ctypes.data, recs.ctypes.data, depth.ctypes.data, C.byref(st)) == 0
            by[name] = (bits.tobytes(), recs.tobytes(), depth.tobytes(), {k: v for k, v in st.as_dict().items() if k not in VOLATILE})
        assert by["null"] == by["zero"]
        glob = ctx.recruit(dev, rd, params=dict(local=False))
        assert glob["recs"].tobytes() == by["null"][1] and glob["recs"].tobytes() != outs["default"]["recs"].tobytes()
        assert_is(glob, ref.recruit(hm, reads), "mode 0")
        # any other mode is refused before anything is written
        for mode in (2, -1):
            bits, recs, depth = np.full(words, 77, dtype=np.uint64), np.zeros(n, dtype=rc.REC), np.full(hm.M, 77, dtype=np.uint64)
            recs.view(np.uint8)[:] = 77
            st = api._lib.RecruitStats()
            st.n_reads = 77
            par.mode = mode
            assert L.mgta_reads_recruit(ctx.h, dev.h, rd.h, 1, n, C.byref(par), bits.ctypes.data, recs.ctypes.data, depth.ctypes.data, C.byref(st)) == -1
            assert b"mode = %d" % mode in L.mgta_last_error()
            assert (bits == 77).all() and (recs.view(np.uint8) == 77).all() and (depth == 77).all() and st.n_reads == 77
        with pytest.raises(api.MegaGtaError):
            ctx.recruit(dev, rd, params=dict(mode=2))
        with pytest.raises(ValueError):
            ctx.recruit(dev, rd, params=dict(mode=1, local=True))
    finally:
        ctx.set_recruit_chunk(0)
        rd.free()


# ---- 7. a metagenome -------------------------------------------------------------------------------------------------------------------
def test_metagenome_local_set_contains_the_global_set(ctx, models):
    mg = synth.make_metagenome(4000, 150, (("g", 120),), seed=3, genome_len=4000)
    model = models.of_protein(mg.genes[0].consensus, "lmeta120")
    reads = [r for r in mg.reads]
    got, want = run_local(ctx, model, reads, what="metagenome")
    glob = run_global(ctx, model, reads)
    n_glob, n_loc = int(glob["bits"].sum()), int(got["bits"].sum())
    print("metagenome: recruited globally", n_glob, "locally", n_loc, "of", len(reads), "stretches", got["stats"]["n_frames_scored"], "global", glob["stats"]["n_frames_scored"])
    assert not (glob["bits"] & ~got["bits"]).any() and n_loc > n_glob >= 0.05 * len(reads)   # at 20 bits the local set contains the global set
    scored = glob["recs"]["status"] == 0
    assert (got["recs"]["score"][scored] >= glob["recs"]["score"][scored]).all() and (got["recs"]["status"][scored] == 0).all()
    assert got["stats"]["n_frames_scored"] >= glob["stats"]["n_frames_scored"] and got["stats"]["n_cells"] >= glob["stats"]["n_cells"]


# ---- 8. process boundary and driver ----------------------------------------------------------------------------------------------------
def test_driver_recruit_local_end_to_end(ctx, golden_dir, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    mg = synth.make_metagenome(6000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)    # the sample of the other driver tests
    synth.write_fasta(mg.reads, str(tmp_path / "reads.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "45", "-t", "4", "--min-contig-len", "150"]
    files = {}
    for name, extra in {"local": ["--match-reads", "--recruit", "--recruit-local"], "plain": ["--recruit"]}.items():
        out = tmp_path / name
        r = subprocess.run(base + ["-o", str(out)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
        files[name] = rc.read_files(str(out / "contigs" / "rplB"))          # the four files parse
    assert files["local"]["summary"]["recruit_mode"] == "local" and "recruit_mode" not in files["plain"]["summary"]
    assert "assembled_fraction" in files["local"]["summary"] and list(files["local"]["summary"])[-3] == "recruit_mode"
    assert set(files["plain"]["reads"].tolist()) < set(files["local"]["reads"].tolist())          # the reads contain those of a plain --recruit run
    assert (tmp_path / "local" / "tmp" / "cp.txt").read_text().splitlines() == [f"{i}\tdone" for i in range(6 + 2)]
    # the files say what Context.recruit says in local mode about the same reads and model
    from megagta_amd import api
    hm = H.parse_hmm(os.path.join(toy, "for_enone.hmm"))
    dev = api.DeviceHmm(ctx, hm)
    reads = [r for r in mg.reads]
    rd, packed, start = upload(ctx, reads)
    try:
        res = ctx.recruit(dev, rd, params=dict(local=True))
    finally:
        rd.free()
        dev.free()
    idx = rc.hit_indices(res["hit_bits"], len(reads))
    d = tmp_path / "local" / "contigs" / "rplB"
    assert files["local"]["reads"].tolist() == idx.tolist() and (d / "recruit.txt").read_text() == rc.recruit_text(res["recs"], idx)
    assert (d / "recruit_cols.txt").read_text() == rc.cols_text(res["col_depth"])
    assert any(r["aa_len"] < 20 for r in files["local"]["recs"]) or any(r["aa_from"] > 0 for r in files["local"]["recs"])   # aligned spans, not stretches
    # the one-shot process and the worker take the flag and write the same four files
    synth.write_lib_bin(mg.reads, str(tmp_path / "reads.lib"))
    subprocess.run([BIN, "recruit", f"{toy}/for_enone.hmm", str(tmp_path / "reads.lib"), str(tmp_path / "one"), "--local"], check=True, capture_output=True, timeout=120)
    r = subprocess.run([BIN, "serve"], input=f"recruit\t{toy}/for_enone.hmm\t{tmp_path}/reads.lib\t{tmp_path}/w\t--min-bits\t20\t--local\nquit\n",
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0"], r.stderr[-2000:]
    for tail, name in (("_reads.fa", "recruit_reads.fa"), (".txt", "recruit.txt"), ("_cols.txt", "recruit_cols.txt")):
        assert open(f"{tmp_path}/one{tail}").read() == open(f"{tmp_path}/w{tail}").read() == (d / name).read_text(), tail
    assert open(f"{tmp_path}/one_summary.txt").read() == open(f"{tmp_path}/w_summary.txt").read() == rc.summary_text(res["stats"], [len(idx)], local=True)
