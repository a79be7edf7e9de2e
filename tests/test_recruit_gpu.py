"""Read recruitment by the gene's model (Context.recruit / `megagta recruit` / `megagta.py --recruit`).

Two yardsticks, neither of them the code under test (tests/recruit_ref.py): (a) the rule in plain Python with the entry column carried
through the recurrence, (b) the same translation, stretch and frame choice around the device's own Context.align, which finds
model_from by its traceback.  Every read of every case is compared with (b): the hit bit, every field of the record (the score in its
8 bytes), the column depth and the stats that are functions of the input; (a) is run on every read of the small cases and on a sample
of the large ones."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from megagta_amd import hmm as H
from megagta_amd import matchreads, readlib, synth
from megagta_amd import recruit as rc
from tests import helpers
from tests import recruit_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
NEG = float("-inf")
INF = float("inf")
BITS20 = 20 * ref.LN2
SENSE = [c for c in range(64) if ref.CODON[c] != "*"]
VOLATILE = ("blocks_per_cu", "waves_per_block", "grid_blocks", "lds_bytes", "msc_in_lds", "rows_per_wave", "chunk", "ms_scan", "ms_fill")


# ---- models, reads -------------------------------------------------------------------------------------------------------------------
class Models:
    def __init__(self, ctx, tmp):
        self.ctx, self.tmp, self.made = ctx, tmp, {}

    def from_text(self, name, text):
        from megagta_amd import api
        if name not in self.made:
            path = os.path.join(self.tmp, name + ".hmm")
            open(path, "w").write(text)
            hm = H.parse_hmm(path)
            self.made[name] = (hm, api.DeviceHmm(self.ctx, hm), path)
        return self.made[name]

    def of_protein(self, prot, name):
        return self.from_text(name, synth.hmm_text("syn", prot))


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def models(ctx, tmp_path_factory):
    return Models(ctx, str(tmp_path_factory.mktemp("recruit_models")))


def protein(rng, n):
    return "".join(synth.AA_ORDER[c] for c in rng.integers(0, 20, n))


def coding(rng, prot):
    """base codes of one codon per residue, drawn among the residue's codons"""
    out = []
    for a in prot:
        c = int(rng.choice(synth.codons_for(a)))
        out += [c >> 4, (c >> 2) & 3, c & 3]
    return np.array(out, dtype=np.uint8)


def codons(*cs):
    """base codes of the codons given as text"""
    return ref.codes_of("".join(cs))


def revcomp(codes):
    return (3 - np.asarray(codes, dtype=np.uint8)[::-1]).astype(np.uint8)


def gene_read(rng, prot, n_bases):
    """n_bases of the gene's coding sequence from a position at random (any frame), on a strand at random; random bases where the gene
    is shorter"""
    cds = coding(rng, prot)
    if len(cds) >= n_bases:
        a = int(rng.integers(0, len(cds) - n_bases + 1))
        r = cds[a:a + n_bases]
    else:
        a = int(rng.integers(0, n_bases - len(cds) + 1))
        r = np.concatenate([rng.integers(0, 4, a, dtype=np.uint8), cds, rng.integers(0, 4, n_bases - len(cds) - a, dtype=np.uint8)])
    return revcomp(r) if rng.integers(0, 2) else r.copy()


def upload(ctx, reads, reversed_storage=True):
    if reversed_storage:
        packed, start = readlib.pack_for_build(reads)
    else:
        start = np.zeros(len(reads) + 1, dtype=np.uint64)
        np.cumsum([len(r) for r in reads], out=start[1:])
        packed = readlib.pack_codes(np.concatenate(reads) if reads else np.zeros(0, dtype=np.uint8))
        if packed.size == 0:
            packed = np.zeros(1, dtype=np.uint32)
    return ctx.upload_reads(packed, start), packed, start


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
def align_scorer(ctx, dev):
    """yardstick (b): the stretches as protein sequences through the device's mgta_seqs_align"""
    def score(seqs):
        recs = ctx.align(dev, seqs, cols=False, paths=False)["recs"]
        return [(float(r["score"]), int(r["model_from"]), int(r["model_to"])) if int(r["status"]) == 0 else (NEG, 0, 0) for r in recs]
    return score


def eight(x):
    return struct.pack("<d", float(x))


def assert_is(got, want, what=""):
    """every read, every output"""
    recs = got["recs"]
    assert len(recs) == len(want["recs"]) == len(got["bits"]), what
    for i, w in enumerate(want["recs"]):
        r = recs[i]
        tag = (what, i, w, float(r["score"]))
        assert eight(r["score"]) == eight(w["score"]), tag
        for f in ("status", "frame", "aa_from", "aa_len", "model_from", "model_to"):
            assert int(r[f]) == w[f], (f,) + tag
        assert bytes(r["pad"]) == b"\0\0", tag
    assert got["bits"].tolist() == want["bits"].tolist(), what
    assert rc.hit_indices(got["hit_bits"], len(recs)).tolist() == np.flatnonzero(want["bits"]).tolist(), what
    assert got["col_depth"].tolist() == want["col_depth"].tolist(), what
    assert {k: got["stats"][k] for k in ref.STABLE} == want["stats"], what


def run_and_compare(ctx, model, reads, min_aa=20, min_score=BITS20, what="", reversed_storage=True, n_short=None, plain=True):
    """the device against yardstick (b) on every read, and against yardstick (a) where plain (the small cases)"""
    hm, dev, _ = model
    rd, _, _ = upload(ctx, reads, reversed_storage)
    try:
        got = ctx.recruit(dev, rd, n_short_reads=n_short, params=dict(min_aa=min_aa, min_score=min_score), reads_reversed=reversed_storage)
    finally:
        rd.free()
    scanned = reads if n_short is None else reads[:n_short]
    want_b = ref.recruit(hm, scanned, min_aa, min_score, scorer=align_scorer(ctx, dev))
    assert_is(got, want_b, what + " (b)")
    if plain:
        assert_is(got, ref.recruit(hm, scanned, min_aa, min_score), what + " (a)")
    return got, want_b


# ---- 1. read lengths, word edges, storage order ---------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 3, 4, 5, 59, 60, 61, 62, 63, 64, 65, 149, 150, 151, 152, 15, 16, 17, 31, 32, 33, 47, 48, 49]


def length_reads(rng, prot):
    reads = []
    for n in LENGTHS + LENGTHS[::-1]:                                       # every length twice: a piece of the gene, then bases at random
        reads.append(gene_read(rng, prot, n) if len(reads) < len(LENGTHS) else rng.integers(0, 4, n, dtype=np.uint8))
    reads += [gene_read(rng, prot, 1000), gene_read(rng, prot, 61), gene_read(rng, prot, 7), gene_read(rng, prot, 62), gene_read(rng, prot, 150)]
    return reads + [gene_read(rng, prot, 65) for _ in range(16)]            # 65 = 4 * 16 + 1: these start at every position of a packed word


@pytest.mark.parametrize("reversed_storage", [True, False])
def test_read_lengths_word_edges_and_storage_order(ctx, models, reversed_storage):
    rng = np.random.default_rng(21)
    prot = protein(rng, 65)
    model = models.of_protein(prot, "len65")
    reads = length_reads(rng, prot)
    start = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    assert set(int(s) % 16 for s in start[:-1]) == set(range(16))            # a read starts at every position of a packed word
    got, want = run_and_compare(ctx, model, reads, what=f"lengths reversed={reversed_storage}", reversed_storage=reversed_storage)
    by_len = {len(r): w for r, w in zip(reads[:len(LENGTHS)], want["recs"][:len(LENGTHS)])}
    assert all(by_len[n]["status"] == 2 for n in LENGTHS if n <= 59)         # fewer than 20 codons in every frame
    assert all(by_len[n]["status"] == 0 for n in (62, 63, 64, 65, 149, 150, 151, 152))   # 20 codons of the gene in at least one frame
    assert want["stats"]["n_recruited"] > 5 and want["stats"]["n_unscored"] > 20
    assert want["recs"][2 * len(LENGTHS)]["aa_len"] > 60                     # the read of 1000 bases: the whole gene in one frame
    assert got["stats"]["rows_per_wave"] == 336 and got["stats"]["msc_in_lds"] == 1    # 1000 / 3 = 333 residues, in eights
    # the reads behind n_short_reads have no bit and no record
    cut, _ = run_and_compare(ctx, model, reads, what="n_short", reversed_storage=reversed_storage, n_short=len(LENGTHS) + 3)
    assert len(cut["recs"]) == len(cut["bits"]) == len(LENGTHS) + 3 and cut["stats"]["n_reads"] == len(LENGTHS) + 3
    assert cut["recs"].tobytes() == got["recs"][:len(LENGTHS) + 3].tobytes()


def test_longest_read_and_one_base_more(ctx, models):
    from megagta_amd import api
    rng = np.random.default_rng(22)
    prot = protein(rng, 65)
    model = models.of_protein(prot, "len65")
    hm, dev, _ = model
    # 3 * 4096 + 2 bases without a stop in frame 2: a stretch of 4096 residues with the gene in its middle
    body = np.array([[c >> 4, (c >> 2) & 3, c & 3] for c in rng.choice(SENSE, 4096)], dtype=np.uint8).reshape(-1)
    body[3 * 2000:3 * 2065] = coding(rng, prot)
    longest = np.concatenate([codons("TA"), body])
    assert len(longest) == ref.MAX_BASES
    reads = [gene_read(rng, prot, 150), longest, gene_read(rng, prot, 90)]
    got, want = run_and_compare(ctx, model, reads, what="longest", plain=False)
    assert want["stretches"][[s[:2] for s in want["stretches"]].index((1, 2))][2:4] == (0, 4096)
    assert want["recs"][1]["status"] == 0 and got["stats"]["rows_per_wave"] == 4096 and got["stats"]["waves_per_block"] == 1
    # one base more: refused with the read's number, nothing written
    L = ctx._L
    rd, _, _ = upload(ctx, [reads[0], reads[2], np.concatenate([longest, codons("A")]), np.concatenate([longest, codons("AC")])])
    try:
        bits, recs, depth = np.full(1, 77, dtype=np.uint64), np.zeros(4, dtype=rc.REC), np.full(hm.M, 77, dtype=np.uint64)
        recs.view(np.uint8)[:] = 77
        st = api._lib.RecruitStats()
        st.n_reads = 77
        import ctypes as C
        assert L.mgta_reads_recruit(ctx.h, dev.h, rd.h, 1, 4, None, bits.ctypes.data, recs.ctypes.data, depth.ctypes.data, C.byref(st)) == -1
        assert b"read 2 " in L.mgta_last_error() and str(ref.MAX_BASES).encode() in L.mgta_last_error()
        assert (bits == 77).all() and (recs.view(np.uint8) == 77).all() and (depth == 77).all() and st.n_reads == 77
        ok = ctx.recruit(dev, rd, n_short_reads=2)                            # the long reads behind n_short_reads are not looked at
        assert ok["recs"].tobytes() == got["recs"][[0, 2]].tobytes()
    finally:
        rd.free()


# ---- 2. stops and stretches ----------------------------------------------------------------------------------------------------------
def test_stops_and_stretches(ctx, models):
    rng = np.random.default_rng(23)
    prot = protein(rng, 64)
    model = models.of_protein(prot, "stop64")
    gene = lambda a, n: coding(rng, prot[a:a + n])
    reads = [np.concatenate([codons("TAA"), gene(3, 30)]),                   # 0: a stop as first codon
             np.concatenate([gene(3, 30), codons("TGA")]),                   # 1: as last codon
             codons(*["TAA"] * 25),                                          # 2: in every codon of frame 0
             np.concatenate([gene(0, 22), codons("TAG"), gene(30, 22)]),     # 3: two equally long stretches: the first
             np.concatenate([gene(0, 22), codons("TAG"), gene(30, 23)]),     # 4: the second is longer
             np.concatenate([codons("TAA"), gene(5, 20), codons("TAA")]),    # 5: a stretch of exactly min_aa
             np.concatenate([codons("TAA"), gene(5, 19), codons("TAA")]),    # 6: of min_aa - 1
             np.concatenate([codons("TAA"), gene(5, 19), codons("TAA"), gene(40, 19), codons("TAG"), gene(20, 20)])]   # 7: the last one alone is scored
    got, want = run_and_compare(ctx, model, reads, what="stops")
    f0 = {s[0]: s[2:4] for s in want["stretches"] if s[1] == 0}              # frame 0 of every read: (aa_from, aa_len)
    assert f0[0] == (1, 30) and f0[1] == (0, 30) and 2 not in f0 and f0[3] == (0, 22) and f0[4] == (23, 23) and f0[5] == (1, 20) and 6 not in f0 and f0[7] == (41, 20)
    assert ref.frames(reads[2])[0] == "*" * 25 and [want["recs"][i]["frame"] for i in (0, 1, 3, 4, 5, 7)] == [0] * 6
    assert all(want["recs"][i]["status"] == 0 for i in (0, 1, 3, 4, 5, 7))
    # min_aa = 1: stretches of one residue are scored, an empty frame is not
    ones = [codons("TAA", "AAA", "TAA"), codons("AAA"), codons("AA"), codons("TAATAA"), codons("TGA", "TGG"), np.zeros(0, dtype=np.uint8)]
    got1, want1 = run_and_compare(ctx, model, ones, min_aa=1, min_score=NEG, what="min_aa 1")
    assert (0, 0, 1, 1, "K") in want1["stretches"] and want1["recs"][2]["status"] == 2 and want1["recs"][5]["status"] == 2
    assert want1["recs"][1]["status"] == 0 and want1["recs"][1]["aa_len"] == 1 and want1["bits"].tolist()[:2] == [True, True]
    assert got1["stats"]["n_unscored"] == 2


# ---- 3. models ---------------------------------------------------------------------------------------------------------------------
def model_reads(rng, prot, n=40):
    reads = [gene_read(rng, prot, int(rng.integers(60, 153))) for _ in range(n)]
    reads += [rng.integers(0, 4, int(rng.integers(60, 153)), dtype=np.uint8) for _ in range(n // 4)]
    return reads


@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 128, 129])
def test_model_widths(ctx, models, M):
    rng = np.random.default_rng(300 + M)
    prot = protein(rng, M)
    model = models.of_protein(prot, f"width{M}")
    assert model[0].M == M
    if M <= 2:
        # one or two columns take one or two residues and no more: short reads at min_aa = 1, and longer ones that are unaligned
        reads = [coding(rng, prot), np.concatenate([codons("TAA"), coding(rng, prot), codons("TGA")]), revcomp(coding(rng, prot)), codons("AAAAAC"),
                 codons("A" * 27), rng.integers(0, 4, 40, dtype=np.uint8)]
        got, want = run_and_compare(ctx, model, reads, min_aa=1, min_score=NEG, what=f"M={M}")
        assert want["recs"][0]["status"] == 0 and (want["recs"][0]["model_from"], want["recs"][0]["model_to"]) == (1, M)
        if M == 1:                                                           # eight or nine residues in every frame, one column, no insert state
            assert want["recs"][4]["status"] == 1 and not want["bits"][4] and want["stats"]["n_unaligned"] >= 1
    else:
        got, want = run_and_compare(ctx, model, model_reads(rng, prot), what=f"M={M}", plain=M <= 65)
        assert want["stats"]["n_recruited"] >= 10 and want["stats"]["n_recruited"] < len(want["recs"])
        assert any(w["model_from"] > 1 for w in want["recs"]) and any(0 < w["model_to"] < M for w in want["recs"])
        assert sum(c > 0 for c in want["stats"]["n_recruited_frame"]) >= 3   # several frames
    assert got["stats"]["msc_in_lds"] == 1 and got["stats"]["waves_per_block"] == 4
    print("M", M, "blocks per CU", got["stats"]["blocks_per_cu"], "LDS", got["stats"]["lds_bytes"], "chunk", got["stats"]["chunk"])


def test_golden_model_that_does_not_fit_lds(ctx, models, tmp_path):
    mg, gdir = helpers.bigm_inputs("m1200", str(tmp_path))
    model = models.from_text("m1200", open(os.path.join(gdir, "for_enone.hmm")).read())
    assert model[0].M == 1200
    reads = [r for r in mg.reads[:240]]
    got, want = run_and_compare(ctx, model, reads, what="M=1200", plain=False)
    assert got["stats"]["msc_in_lds"] == 0                                   # the match scores are read from device memory
    assert 10 <= want["stats"]["n_recruited"] < 200 and int(want["col_depth"].max()) >= 2
    sample = [int(i) for i in np.flatnonzero(want["bits"])[:2]] + [0]
    plain = ref.recruit(model[0], [reads[i] for i in sample])
    for k, i in enumerate(sample):
        assert plain["recs"][k] == want["recs"][i], i


def with_stars(text, match_stars=(), trans_stars=()):
    """the model text with `*` for the match emission (node, letter) and the transition (node, 0 .. 6)"""
    lines = text.split("\n")
    node_line = {}
    for n, line in enumerate(lines):
        t = line.split()
        if len(t) >= 23 and t[0].isdigit():
            node_line[int(t[0])] = n
    for node, letter in match_stars:
        t = lines[node_line[node]].split()
        t[1 + synth.AA_ORDER.index(letter.upper())] = "*"
        lines[node_line[node]] = "  " + "  ".join(t)
    for node, x in trans_stars:
        t = lines[node_line[node] + 2].split()
        t[x] = "*"
        lines[node_line[node] + 2] = "          " + "  ".join(t)
    return "\n".join(lines)


def test_minus_infinity_in_the_tables(ctx, models):
    rng = np.random.default_rng(31)
    prot = protein(rng, 40)
    # no insert and no delete anywhere, and no way from column 20 to 21: a stretch is placed only without a gap and on one side of the cut
    stars = [(j, x) for j in range(1, 41) for x in (ref.MI, ref.MD)] + [(20, ref.MM)]
    model = models.from_text("star40", with_stars(synth.hmm_text("s", prot), trans_stars=stars))
    assert model[0].tsc[ref.MM, 20] == NEG and model[0].tsc[ref.MI, 7] == NEG
    reads = [coding(rng, prot[0:20]), coding(rng, prot[20:40]), coding(rng, prot[5:30]), coding(rng, prot), revcomp(coding(rng, prot[8:33])),
             coding(rng, prot[0:21]), np.concatenate([codons("TAA"), coding(rng, prot[18:40])])]
    got, want = run_and_compare(ctx, model, reads, min_score=NEG, what="stars")
    assert [w["status"] for w in want["recs"][:2]] == [0, 0] and (want["recs"][1]["model_from"], want["recs"][1]["model_to"]) == (21, 40)
    una = [i for i, w in enumerate(want["recs"]) if w["status"] == 1]
    assert len(una) >= 2 and not want["bits"][una].any() and want["stats"]["n_unaligned"] == len(una)   # not recruited even at -inf
    assert not any(np.isnan(got["recs"]["score"]))


# ---- 4. frame ties -------------------------------------------------------------------------------------------------------------------
def test_frame_ties_go_to_the_lower_frame(ctx, models):
    rng = np.random.default_rng(41)
    prot = "K" * 30 + protein(rng, 34)
    model = models.of_protein(prot, "ties64")
    half = np.concatenate([coding(rng, prot[30:52]), rng.integers(0, 4, 2, dtype=np.uint8)])
    own_rc = np.concatenate([half, revcomp(half)])                           # equal to its own reverse complement: frames 3 .. 5 repeat 0 .. 2
    assert own_rc.tolist() == revcomp(own_rc).tolist()
    poly = codons("A" * 62)                                                  # frames 0, 1 and 2 are twenty K each
    assert ref.frames(poly)[:3] == ["K" * 20] * 3
    reads = [own_rc, poly, revcomp(poly), codons("A" * 64)]
    got, want = run_and_compare(ctx, model, reads, min_score=NEG, what="ties")
    fr = ref.frames(own_rc)
    assert fr[:3] == fr[3:] and want["recs"][0]["status"] == 0 and want["recs"][0]["frame"] < 3
    assert want["recs"][1]["frame"] == 0 and want["recs"][2]["frame"] == 3   # three equal frames on a strand: the lowest
    assert [s[1] for s in want["stretches"] if s[0] == 1][:3] == [0, 1, 2]
    assert want["recs"][3]["frame"] == 0 and want["recs"][3]["aa_len"] == 21  # 64 bases: frame 0 has a residue more than frame 2


# ---- 5. threshold --------------------------------------------------------------------------------------------------------------------
def test_threshold_is_inclusive_and_takes_infinities(ctx, models):
    rng = np.random.default_rng(51)
    prot = protein(rng, 65)
    model = models.of_protein(prot, "len65")
    reads = model_reads(rng, prot, 24)
    low, want = run_and_compare(ctx, model, reads, min_score=NEG, what="-inf", plain=False)
    scored = [i for i, w in enumerate(want["recs"]) if w["status"] == 0]
    assert low["bits"].tolist() == [w["status"] == 0 for w in want["recs"]] and len(scored) > 12
    none, _ = run_and_compare(ctx, model, reads, min_score=INF, what="+inf", plain=False)
    assert not none["bits"].any() and none["col_depth"].sum() == 0 and none["recs"].tobytes() == low["recs"].tobytes()
    scores = sorted(want["recs"][i]["score"] for i in scored)
    at = scores[len(scores) // 2]
    exact, w_exact = run_and_compare(ctx, model, reads, min_score=at, what="exact", plain=False)
    above, _ = run_and_compare(ctx, model, reads, min_score=float(np.nextafter(at, INF)), what="above", plain=False)
    n_at = sum(s == at for s in scores)
    assert exact["stats"]["n_recruited"] == sum(s >= at for s in scores) == above["stats"]["n_recruited"] + n_at and n_at >= 1
    # the defaults: 20 residues and 20 bits, as a NULL params pointer and as the wrapper's own
    hm, dev, _ = model
    rd, _, _ = upload(ctx, reads)
    try:
        dflt = ctx.recruit(dev, rd)
        by_bits = ctx.recruit(dev, rd, params=dict(min_bits=20.0))
        words = np.zeros(1, dtype=np.uint64)
        assert ctx._L.mgta_reads_recruit(ctx.h, dev.h, rd.h, 1, len(reads), None, words.ctypes.data, None, None, None) == 0
    finally:
        rd.free()
    assert dflt["bits"].tolist() == by_bits["bits"].tolist() == [w["status"] == 0 and w["score"] >= BITS20 for w in want["recs"]]
    assert words.tolist() == dflt["hit_bits"].tolist()


# ---- 6. chunking, repeatability ------------------------------------------------------------------------------------------------------
def test_chunks_and_calls_give_the_same_bytes(ctx, models):
    rng = np.random.default_rng(61)
    prot = protein(rng, 100)
    model = models.of_protein(prot, "chunk100")
    hm, dev, _ = model
    reads = model_reads(rng, prot, 160) + length_reads(rng, prot)
    rd, _, _ = upload(ctx, reads)
    outs = {}
    try:
        outs["default"] = ctx.recruit(dev, rd)
        outs["again"] = ctx.recruit(dev, rd)
        for chunk in (1, 7, 64, 1000):
            ctx.set_recruit_chunk(chunk)
            outs[chunk] = ctx.recruit(dev, rd)
    finally:
        ctx.set_recruit_chunk(0)
        rd.free()
    assert [outs[c]["stats"]["chunk"] for c in (1, 7, 64, 1000)] == [1, 7, 64, 64]
    want = ref.recruit(hm, reads, scorer=align_scorer(ctx, dev))
    for name, res in outs.items():
        assert_is(res, want, f"chunk {name}")
        for f in ("hit_bits", "recs", "col_depth"):
            assert res[f].tobytes() == outs["default"][f].tobytes(), (name, f)
        assert {k: v for k, v in res["stats"].items() if k not in VOLATILE} == {k: v for k, v in outs["default"]["stats"].items() if k not in VOLATILE}
    rd, _, _ = upload(ctx, reads)
    try:
        bare = ctx.recruit(dev, rd, recs=False, cols=False)
    finally:
        rd.free()
    assert bare["recs"] is None and bare["col_depth"] is None and bare["hit_bits"].tobytes() == outs["default"]["hit_bits"].tobytes()


# ---- 7. a metagenome -----------------------------------------------------------------------------------------------------------------
def test_metagenome(ctx, models):
    mg = synth.make_metagenome(4000, 150, (("g", 120),), seed=3, genome_len=4000)
    model = models.of_protein(mg.genes[0].consensus, "meta120")
    hm, dev, _ = model
    reads = [r for r in mg.reads]
    want = ref.recruit(hm, reads, scorer=align_scorer(ctx, dev))
    n_hit = int(want["bits"].sum())
    print("metagenome: recruited", n_hit, "of", len(reads), "scored frames", want["stats"]["n_frames_scored"], "unscored", want["stats"]["n_unscored"])
    assert n_hit >= 0.05 * len(reads) and len(reads) - n_hit >= 0.5 * len(reads)   # on yardstick (b): the gene is there, most reads are not its
    rd, _, _ = upload(ctx, reads)
    try:
        got = ctx.recruit(dev, rd)
    finally:
        rd.free()
    assert_is(got, want, "metagenome (b)")
    # yardstick (a) on about 50 reads: recruited ones, ones with a score below the threshold, the first few as they come
    scored_low = [i for i, w in enumerate(want["recs"]) if w["status"] == 0 and not want["bits"][i]]
    sample = sorted(set(np.flatnonzero(want["bits"])[:20].tolist() + scored_low[:20] + list(range(10))))
    plain = ref.recruit(hm, [reads[i] for i in sample])
    for k, i in enumerate(sample):
        assert eight(plain["recs"][k]["score"]) == eight(want["recs"][i]["score"]) and plain["recs"][k] == want["recs"][i], i
        assert bool(plain["bits"][k]) == bool(want["bits"][i])
    assert int(got["col_depth"].max()) <= n_hit and int(got["col_depth"].sum()) == sum(w["model_to"] - w["model_from"] + 1 for w, b in zip(want["recs"], want["bits"]) if b)


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------
def test_guards(ctx, models):
    from megagta_amd import api
    import ctypes as C
    L = ctx._L
    rng = np.random.default_rng(71)
    prot = protein(rng, 65)
    hm, dev, _ = models.of_protein(prot, "len65")
    reads = [gene_read(rng, prot, 150) for _ in range(5)]
    rd, _, _ = upload(ctx, reads)
    other = api.Context(0)
    try:
        bits, recs, depth = np.full(2, 77, dtype=np.uint64), np.zeros(6, dtype=rc.REC), np.full(hm.M + 1, 77, dtype=np.uint64)
        recs.view(np.uint8)[:] = 77
        outs = (bits.ctypes.data, recs.ctypes.data, depth.ctypes.data, None)
        par = api._lib.RecruitParams()
        par.min_aa, par.min_score = 20, BITS20
        assert L.mgta_reads_recruit(None, dev.h, rd.h, 1, 5, None, *outs) == -1 and b"ctx" in L.mgta_last_error()
        assert L.mgta_reads_recruit(ctx.h, None, rd.h, 1, 5, None, *outs) == -1 and b"model" in L.mgta_last_error()
        assert L.mgta_reads_recruit(ctx.h, dev.h, None, 1, 5, None, *outs) == -1 and b"reads" in L.mgta_last_error()
        assert L.mgta_reads_recruit(ctx.h, dev.h, rd.h, 1, 5, None, None, *outs[1:]) == -1 and b"hit_bits" in L.mgta_last_error()
        assert L.mgta_reads_recruit(ctx.h, dev.h, rd.h, 1, 6, None, *outs) == -1 and b"n_short_reads = 6" in L.mgta_last_error()
        assert L.mgta_reads_recruit(other.h, dev.h, rd.h, 1, 5, None, *outs) == -1 and b"another context" in L.mgta_last_error()
        rd2, _, _ = upload(other, reads)
        try:
            assert L.mgta_reads_recruit(ctx.h, dev.h, rd2.h, 1, 5, None, *outs) == -1 and b"another context" in L.mgta_last_error()
        finally:
            rd2.free()
        par.min_aa = 0
        assert L.mgta_reads_recruit(ctx.h, dev.h, rd.h, 1, 5, C.byref(par), *outs) == -1 and b"min_aa = 0" in L.mgta_last_error()
        par.min_aa, par.min_score = 20, float("nan")
        assert L.mgta_reads_recruit(ctx.h, dev.h, rd.h, 1, 5, C.byref(par), *outs) == -1 and b"NaN" in L.mgta_last_error()
        assert L.mgta_ctx_set_recruit_chunk(None, 3) == -1 and b"ctx" in L.mgta_last_error()
        assert (bits == 77).all() and (recs.view(np.uint8) == 77).all() and (depth == 77).all()     # nothing was written by the refused calls
        # a valid call writes the bits of 5 reads, 5 records and M depths, and nothing behind them
        par.min_score = BITS20
        assert L.mgta_reads_recruit(ctx.h, dev.h, rd.h, 1, 5, C.byref(par), *outs) == 0
        want = ref.recruit(hm, reads)
        assert int(bits[0]) == sum(1 << i for i in np.flatnonzero(want["bits"])) and int(bits[1]) == 77
        assert (recs[5:].view(np.uint8) == 77).all() and int(depth[hm.M]) == 77 and depth[:hm.M].tolist() == want["col_depth"].tolist()
        assert [int(s) for s in recs["status"][:5]] == [w["status"] for w in want["recs"]]
        # no reads: zero depths, zero stats, no bit asked for
        st = api._lib.RecruitStats()
        st.n_reads = 77
        assert L.mgta_reads_recruit(ctx.h, dev.h, rd.h, 1, 0, None, None, None, depth.ctypes.data, C.byref(st)) == 0
        assert (depth[:hm.M] == 0).all() and int(depth[hm.M]) == 77 and st.n_reads == 0 and st.n_cells == 0
        empty = ctx.recruit(dev, rd, n_short_reads=0)
        assert len(empty["bits"]) == 0 and len(empty["recs"]) == 0 and len(empty["hit_bits"]) == 0 and empty["stats"]["n_recruited"] == 0
        with pytest.raises(ValueError):
            ctx.recruit(dev, rd, params=dict(min_len=3))
    finally:
        rd.free()
        other.close()


# ---- 9. process boundary and driver --------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_driver_recruit_end_to_end(ctx, golden_dir, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    mg = synth.make_metagenome(6000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)    # the sample of the other driver tests
    synth.write_fasta(mg.reads, str(tmp_path / "reads.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "45", "-t", "4", "--min-contig-len", "150",
            "--match-reads"]
    trees = {}
    for name, extra in {"rc": ["--recruit"], "plain": []}.items():
        out = tmp_path / name
        r = subprocess.run(base + ["-o", str(out)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
        trees[name] = _tree(str(out))
    d = "contigs/rplB/"
    new = {d + "recruit_reads.fa", d + "recruit.txt", d + "recruit_cols.txt", d + "recruit_summary.txt"}
    assert set(trees["rc"]) - set(trees["plain"]) == new                  # four files per gene ...
    assert not [f for f in trees["plain"] if "recruit" in f]              # ... and none without the flag
    for f in set(trees["plain"]) - {"log", "opts.txt", "tmp/cp.txt"}:
        assert trees["rc"][f] == trees["plain"][f], f
    # one checkpoint for the flag's step (one gene) behind the seven of a run without it, whose cp.txt is what it was
    assert trees["plain"]["tmp/cp.txt"].decode().splitlines() == [f"{i}\tdone" for i in range(6 + 1)]
    assert trees["rc"]["tmp/cp.txt"].decode().splitlines() == [f"{i}\tdone" for i in range(6 + 2)]
    # the four files parse and say what Context.recruit says about the same reads and model
    from megagta_amd import api
    files = rc.read_files(str(tmp_path / "rc" / "contigs" / "rplB"))
    hm = H.parse_hmm(os.path.join(toy, "for_enone.hmm"))
    dev = api.DeviceHmm(ctx, hm)
    reads = [r for r in mg.reads]
    rd, packed, start = upload(ctx, reads)
    try:
        res = ctx.recruit(dev, rd)
    finally:
        rd.free()
        dev.free()
    idx = rc.hit_indices(res["hit_bits"], len(reads))
    assert len(idx) > 0 and files["reads"].tolist() == idx.tolist()
    assert trees["rc"][d + "recruit_reads.fa"].decode() == matchreads.match_reads_text(idx, packed, start)
    assert trees["rc"][d + "recruit.txt"].decode() == rc.recruit_text(res["recs"], idx)
    assert trees["rc"][d + "recruit_cols.txt"].decode() == rc.cols_text(res["col_depth"]) and len(files["col_depth"]) == hm.M
    matched = matchreads.parse_match_reads(trees["rc"][d + "nucl_merged_match_reads.fa"].decode())[0]
    assert trees["rc"][d + "recruit_summary.txt"].decode() == rc.summary_text(res["stats"], [len(idx)], idx, matched)
    both = len(set(files["reads"].tolist()) & set(matched.tolist()))       # from the two .fa files
    assert files["summary"]["recruited_and_matched"] == both and files["summary"]["assembled_fraction"] == float("%.4f" % (both / len(idx)))
    assert files["summary"]["reads_scanned"] == 6000 and files["summary"]["recruited_lib0"] == len(idx)
    # the one-shot process and the worker write the same four files
    synth.write_lib_bin(mg.reads, str(tmp_path / "reads.lib"))
    subprocess.run([BIN, "recruit", f"{toy}/for_enone.hmm", str(tmp_path / "reads.lib"), str(tmp_path / "one")], check=True, capture_output=True, timeout=120)
    r = subprocess.run([BIN, "serve"], input=f"recruit\t{toy}/for_enone.hmm\t{tmp_path}/reads.lib\t{tmp_path}/w\t--min-bits\t20\t--min-aa\t20\nquit\n",
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0"], r.stderr[-2000:]
    for tail, name in (("_reads.fa", "recruit_reads.fa"), (".txt", "recruit.txt"), ("_cols.txt", "recruit_cols.txt")):
        assert open(f"{tmp_path}/one{tail}").read() == open(f"{tmp_path}/w{tail}").read() == trees["rc"][d + name].decode(), tail
    assert open(f"{tmp_path}/one_summary.txt").read() == open(f"{tmp_path}/w_summary.txt").read() == rc.summary_text(res["stats"], [len(idx)])
