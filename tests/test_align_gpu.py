"""Alignment to the model (Context.align / `megagta align` / `megagta.py --align`): protein sequences placed on the columns of a profile HMM.

The yardstick is `restate`: the recurrence and the tie rules of include/megagta_hip.h as three nested Python loops over Python floats
(IEEE doubles, one add per +).  Every sequence of every case is compared: the score bit for bit, the record's integers, cols and path
byte for byte."""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from megagta_amd import align as al
from megagta_amd import hmm as H
from megagta_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
AA = "acdefghiklmnpqrstvwy"
NEG = float("-inf")
MM, MI, MD, IM, II, DM, DD = range(7)
MAX_LEN = 4096


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------
def restate(hm, seq):
    """-> dict(status, score, model_from, model_to, n_match, n_insert, n_delete, cols (bytes, M), path (str), ties (equal finite
    candidates met at a maximum))"""
    if isinstance(seq, str):
        seq = seq.encode("latin-1")
    M, L = hm.M, len(seq)
    msc, tsc, alpha = hm.msc.tolist(), hm.tsc.tolist(), hm.alpha.tolist()
    out = dict(status=1, score=NEG, model_from=0, model_to=0, n_match=0, n_insert=0, n_delete=0, cols=b"-" * M, path="", ties=0)
    if L == 0:
        return out
    ties = 0
    VM = [[NEG] * (M + 1) for _ in range(L + 1)]
    VI = [[NEG] * (M + 1) for _ in range(L + 1)]
    VD = [[NEG] * (M + 1) for _ in range(L + 1)]
    FM = [[None] * (M + 1) for _ in range(L + 1)]      # the candidate that won: "B", "M", "I", "D"
    FI = [[None] * (M + 1) for _ in range(L + 1)]
    FD = [[None] * (M + 1) for _ in range(L + 1)]
    for i in range(1, L + 1):
        x = seq[i - 1]
        a = alpha[x] if x < 127 else -1
        for j in range(1, M + 1):
            e = msc[j][a] if a >= 0 else 0.0
            for state in "MID":
                if state == "M":
                    cands = [("B", 0.0)] if i == 1 else []
                    if i > 1 and j > 1:
                        cands += [("M", VM[i - 1][j - 1] + tsc[MM][j - 1]), ("I", VI[i - 1][j - 1] + tsc[IM][j - 1]), ("D", VD[i - 1][j - 1] + tsc[DM][j - 1])]
                elif state == "I":
                    cands = [("M", VM[i - 1][j] + tsc[MI][j]), ("I", VI[i - 1][j] + tsc[II][j])] if i > 1 and j < M else []
                else:
                    cands = [("M", VM[i][j - 1] + tsc[MD][j - 1]), ("D", VD[i][j - 1] + tsc[DD][j - 1])] if i > 1 and j > 1 else []
                best, who = NEG, None
                for name, v in cands:                                     # the candidate written first wins on equality
                    if who is None or v > best:
                        best, who = v, name
                    elif v == best and v > NEG:
                        ties += 1
                if state == "M":
                    VM[i][j], FM[i][j] = best + e, who                    # the maximum first, then + e
                elif state == "I":
                    VI[i][j], FI[i][j] = best, who
                else:
                    VD[i][j], FD[i][j] = best, who
    score = max(VM[L][1:])
    out["ties"] = ties + sum(1 for v in VM[L][1:] if v == score and score > NEG) - (1 if score > NEG else 0)
    if score == NEG:
        return out
    j = VM[L].index(score, 1)                                             # the lowest column that reaches the score
    i, state = L, "M"
    cols, path = [ord("-")] * M, []
    out.update(status=0, score=score, model_to=j)
    while True:
        path.append(state)
        if state == "M":
            cols[j - 1] = ord(chr(seq[i - 1]).upper()) if seq[i - 1] < 128 else seq[i - 1]
            out["n_match"] += 1
            out["model_from"] = j
            if FM[i][j] == "B":
                break
            state, i, j = FM[i][j], i - 1, j - 1
        elif state == "I":
            out["n_insert"] += 1
            state, i = FI[i][j], i - 1
        else:
            out["n_delete"] += 1
            state, j = FD[i][j], j - 1
    assert i == 1
    out.update(cols=bytes(cols), path="".join(reversed(path)))
    return out


def bits(x):
    return struct.pack("<d", float(x))


def assert_is(res, wants, seqs, M, what=""):
    """every sequence, every output"""
    recs, cols, paths = res["recs"], res["cols"], res["paths"]
    assert len(recs) == len(wants) == len(paths) and cols.shape == (len(wants), M)
    for i, w in enumerate(wants):
        r = recs[i]
        tag = (what, i, seqs[i][:40], w["score"], float(r["score"]))
        assert bits(r["score"]) == bits(w["score"]), tag                  # the 8 bytes
        for f in ("status", "model_from", "model_to", "n_match", "n_insert", "n_delete"):
            assert int(r[f]) == w[f], (f,) + tag
        assert cols[i].tobytes() == w["cols"], tag
        assert paths[i] == w["path"], tag
        L = len(seqs[i])
        assert len(paths[i]) == (L + w["n_delete"] if w["status"] == 0 else 0) and len(paths[i]) <= L + max(0, M - 2)
    st = res["stats"]
    assert st["n_seqs"] == len(wants) and st["n_unaligned"] == sum(w["status"] for w in wants) and st["n_aligned"] == st["n_seqs"] - st["n_unaligned"]
    assert st["n_cells"] == sum(len(s) for s in seqs) * M


def stable(st):
    return {n: v for n, v in st.items() if not n.startswith("ms_") and n != "n_batches"}


# ---- models and sequences ----------------------------------------------------------------------------------------------------------
def protein(rng, n):
    return "".join(AA[c] for c in rng.integers(0, 20, n)).upper()


class Models:
    def __init__(self, ctx, tmp, golden_dir):
        self.ctx, self.tmp, self.golden_dir, self.made = ctx, tmp, golden_dir, {}

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

    def toy(self):
        path = os.path.join(self.golden_dir, "toy", "for_enone.hmm")
        return self.from_text("toy", open(path).read())


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def models(ctx, tmp_path_factory, golden_dir):
    return Models(ctx, str(tmp_path_factory.mktemp("align_models")), golden_dir)


def consensus(hm):
    """the residue with the highest match score of every column"""
    letters = {int(hm.alpha[ord(c)]): c for c in AA}
    return "".join(letters[int(np.argmax(hm.msc[j]))] for j in range(1, hm.M + 1))


def run_and_compare(ctx, model, seqs, what=""):
    hm, dev, _ = model
    wants = [restate(hm, s) for s in seqs]
    res = ctx.align(dev, seqs, cols=True, paths=True)
    assert_is(res, wants, seqs, hm.M, what)
    return res, wants


# ---- 1. strip and lane edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 100, 129])
def test_strip_and_lane_edges(ctx, models, M):
    rng = np.random.default_rng(100 + M)
    model = models.toy() if M == 100 else models.of_protein(protein(rng, M), f"edge{M}")
    hm = model[0]
    assert hm.M == M
    cons = consensus(hm)
    seqs = []
    for L in (1, 2, 63, 64, 65, 130):
        # a piece of the model's protein where it is long enough (a real placement), the protein repeated otherwise (L > M: inserts)
        reps = (cons * (L // M + 2))
        a = int(rng.integers(0, max(1, M - L + 1))) if L <= M else int(rng.integers(0, M))
        seqs.append(reps[a:a + L])
        seqs.append("".join(AA[c] for c in rng.integers(0, 20, L)))       # and letters at random
    res, wants = run_and_compare(ctx, model, seqs, f"M={M}")
    lens = {len(s) for s in seqs}
    assert any(l < M for l in lens) or M == 1
    assert any(l > M for l in lens)
    if M > 2:
        assert any(w["n_insert"] > 0 for w, s in zip(wants, seqs) if len(s) > M)    # L > M forces inserts
    assert res["stats"]["msc_in_lds"] == 1 and res["stats"]["waves_per_block"] == 4
    print("M", M, "blocks per CU", res["stats"]["blocks_per_cu"], "LDS", res["stats"]["lds_bytes"])


# ---- 2. fragments ------------------------------------------------------------------------------------------------------------------
def fragments(rng, prot, n_each=6):
    out = []
    M = len(prot)
    for kind in ("sub", "del", "ins", "unknown"):
        for r in range(n_each):
            n = int(rng.integers(20, min(M, 90) + 1))
            a = int(rng.integers(0, M - n + 1))
            s = list(prot[a:a + n].lower())
            at = int(rng.integers(3, n - 8))
            k = 1 + r % 5
            if kind == "sub":
                for p in rng.integers(0, n, 1 + r):
                    s[p] = AA[(AA.index(s[p]) + 1 + int(rng.integers(0, 19))) % 20]
            elif kind == "del":
                del s[at:at + k]
            elif kind == "ins":
                s[at:at] = [AA[c] for c in rng.integers(0, 20, k)]
            else:
                for p in rng.integers(0, n, 1 + r):
                    s[p] = "x*"[int(rng.integers(0, 2))]
            out.append("".join(s))
    return out


def test_fragments_substituted_deleted_inserted_unknown(ctx, models):
    rng = np.random.default_rng(5)
    for model in (models.of_protein(protein(rng, 150), "frag150"), models.toy()):
        hm = model[0]
        seqs = fragments(rng, consensus(hm).upper())
        res, wants = run_and_compare(ctx, model, seqs, f"fragments M={hm.M}")
        assert all(w["status"] == 0 for w in wants)
        assert any(w["n_delete"] > 0 for w in wants) and any(w["n_insert"] > 0 for w in wants)
        assert any(b"X" in w["cols"] for w in wants) and any(b"*" in w["cols"] for w in wants)
        assert any(w["model_from"] > 1 for w in wants) and any(w["model_to"] < hm.M for w in wants)


# ---- 3. case -----------------------------------------------------------------------------------------------------------------------
def test_upper_and_lower_case_input(ctx, models):
    rng = np.random.default_rng(6)
    model = models.of_protein(protein(rng, 150), "frag150")
    seqs = fragments(rng, consensus(model[0]).upper(), n_each=2)
    low, _ = run_and_compare(ctx, model, seqs, "lower")
    up, _ = run_and_compare(ctx, model, [s.upper() for s in seqs], "upper")
    mixed, _ = run_and_compare(ctx, model, ["".join(c.upper() if i % 3 else c for i, c in enumerate(s)) for s in seqs], "mixed")
    for other in (up, mixed):
        assert other["recs"].tobytes() == low["recs"].tobytes() and other["cols"].tobytes() == low["cols"].tobytes() and other["paths"] == low["paths"]
    assert run_and_compare(ctx, model, [s.encode() for s in seqs], "bytes")[0]["recs"].tobytes() == low["recs"].tobytes()
    # bytes without a column, 127 and above included, emit 0 in a match state
    run_and_compare(ctx, model, [b"acd\x7fef\x80\xffgh", b"\x00\x01", b"-.-"], "unknown bytes")


# ---- 4. ties -----------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_first_candidate_and_the_lowest_column(ctx, models):
    model = models.of_protein("A" * 70, "ties70")
    seqs = ["a" * n for n in (1, 2, 5, 64, 69, 70, 71, 90)] + ["a" * 10 + "x" * 3 + "a" * 10]
    res, wants = run_and_compare(ctx, model, seqs, "ties")
    assert all(w["ties"] > 0 for w in wants)                              # the yardstick really meets equal candidates on this input
    # every placement of a short run scores the same: the lowest end column wins, so the run sits at the model's start
    for w, s in zip(wants[:5], seqs[:5]):
        assert (w["model_from"], w["model_to"]) == (1, len(s)) and w["path"] == "M" * len(s)


# ---- 5. -inf -----------------------------------------------------------------------------------------------------------------------
def with_stars(text, match_stars=(), trans_stars=()):
    """the model text with `*` for the match emission (node, letter) and the transition (node, 0 .. 6)"""
    letters = synth.AA_ORDER
    lines = text.split("\n")
    node_line = {}
    for n, line in enumerate(lines):
        t = line.split()
        if len(t) >= 23 and t[0].isdigit():
            node_line[int(t[0])] = n
    for node, letter in match_stars:
        t = lines[node_line[node]].split()
        t[1 + letters.index(letter.upper())] = "*"
        lines[node_line[node]] = "  " + "  ".join(t)
    for node, x in trans_stars:
        t = lines[node_line[node] + 2].split()
        t[x] = "*"
        lines[node_line[node] + 2] = "          " + "  ".join(t)
    return "\n".join(lines)


def test_minus_infinity_in_the_tables(ctx, models):
    # two columns, two residues: the only path is M1 M2
    cut_t = models.from_text("star_t", with_stars(synth.hmm_text("s", "AC"), trans_stars=[(1, MM)]))
    cut_e = models.from_text("star_e", with_stars(synth.hmm_text("s", "AC"), match_stars=[(2, "C")]))
    assert cut_t[0].tsc[MM, 1] == NEG and cut_e[0].msc[2, cut_e[0].alpha[ord("c")]] == NEG
    for model, seqs in ((cut_t, ["ac", "a", "c", "aca"]), (cut_e, ["ac", "aa", "c", "a"])):
        res, wants = run_and_compare(ctx, model, seqs, "stars M=2")
        assert wants[0]["status"] == 1 and wants[0]["score"] == NEG and wants[0]["cols"] == b"--" and wants[0]["path"] == ""
        assert any(w["status"] == 0 for w in wants[1:])
        assert int(res["recs"]["status"][0]) == 1 and res["stats"]["n_unaligned"] == sum(w["status"] for w in wants)
    # a longer model with both: paths go round the cut where they can
    rng = np.random.default_rng(9)
    prot = protein(rng, 40)
    model = models.from_text("star40", with_stars(synth.hmm_text("s", prot), match_stars=[(10, prot[9]), (30, "W")], trans_stars=[(20, MM), (21, MD), (5, II)]))
    seqs = [prot[a:b].lower() for a, b in ((0, 40), (5, 25), (15, 30), (19, 21), (8, 12), (0, 10), (25, 35))] + [prot.lower()[:20] + "ww" + prot.lower()[20:], "w" * 45]
    res, wants = run_and_compare(ctx, model, seqs, "stars M=40")
    assert any(w["status"] == 0 for w in wants)
    assert not any(math.isnan(float(s)) for s in res["recs"]["score"])


# ---- 6. empty and batch edges ------------------------------------------------------------------------------------------------------
def test_empty_and_batch_edges(ctx, models):
    rng = np.random.default_rng(12)
    model = models.of_protein(protein(rng, 20), "short20")
    hm, dev, _ = model
    res = ctx.align(dev, [], cols=True, paths=True)
    assert len(res["recs"]) == 0 and res["cols"].shape == (0, 20) and res["paths"] == [] and all(v == 0 for v in res["stats"].values())
    cons = consensus(hm)
    some = ["", cons[3:12], "", cons, cons[:5] + "kk" + cons[5:], ""]
    res, wants = run_and_compare(ctx, model, some, "empty among others")
    assert [w["status"] for w in wants] == [1, 0, 1, 0, 0, 1]
    # 3 000 short sequences, more than the groups in flight; with the batch switch and without it the outputs do not move
    seqs = []
    for _ in range(3000):
        n = int(rng.integers(2, 13))
        a = int(rng.integers(0, 20 - n + 1))
        s = list(cons[a:a + n])
        if rng.integers(0, 3) == 0:
            s[int(rng.integers(0, n))] = AA[int(rng.integers(0, 20))]
        seqs.append("".join(s))
    seqs[17] = ""
    whole, wants = run_and_compare(ctx, model, seqs, "3000")
    assert whole["stats"]["n_batches"] == 1
    outs = {}
    try:
        for cells in (1, 20 * 100):
            ctx.set_align_batch(cells)
            outs[cells] = ctx.align(dev, seqs, cols=True, paths=True)
    finally:
        ctx.set_align_batch(0)
    assert outs[1]["stats"]["n_batches"] == 3000                         # every sequence a batch of its own
    assert 1 < outs[2000]["stats"]["n_batches"] < 3000
    for cells, res in outs.items():
        assert_is(res, wants, seqs, 20, f"batch {cells}")
        assert res["recs"].tobytes() == whole["recs"].tobytes() and res["cols"].tobytes() == whole["cols"].tobytes() and res["paths"] == whole["paths"], cells
    # records alone: no cols, no paths
    bare = ctx.align(dev, seqs, cols=False, paths=False)
    assert set(bare) == {"recs", "stats"} and bare["recs"].tobytes() == whole["recs"].tobytes()
    # 12 000 drawn from those: more sequences than waves in flight, so a wave takes one sequence after another
    pick = rng.integers(0, 3000, 12000)
    many = ctx.align(dev, [seqs[i] for i in pick], cols=True, paths=True)
    assert_is(many, [wants[i] for i in pick], [seqs[i] for i in pick], 20, "12000")
    assert many["stats"]["grid_blocks"] * many["stats"]["waves_per_block"] < 12000


# ---- 7. wide model, long sequences -------------------------------------------------------------------------------------------------
def test_wide_model_from_device_memory(ctx, models):
    rng = np.random.default_rng(13)
    prot = protein(rng, 1200)
    model = models.of_protein(prot, "wide1200")
    seqs = [prot[100:200].lower(), prot[1000:1200].lower(), prot[300:450].lower() + prot[460:700].lower(), prot[630:800].lower() + "kkk" + prot[800:900].lower()]
    assert [len(s) for s in seqs] == [100, 200, 390, 273]
    res, _ = run_and_compare(ctx, model, seqs, "M=1200")
    assert res["stats"]["msc_in_lds"] == 0                                # the match scores do not fit LDS: read from device memory


def test_longest_sequences(ctx, models):
    """the sequence lengths at which a workgroup holds 4, 2 and 1 sequences, the limit included"""
    rng = np.random.default_rng(14)
    prot = protein(rng, 65)
    model = models.of_protein(prot, "long65")
    for L, waves in ((1300, 2), (MAX_LEN, 1)):
        s = "".join(AA[c] for c in rng.integers(0, 20, L))
        s = s[:L // 2] + prot.lower() + s[L // 2 + 65:]
        assert len(s) == L
        res, _ = run_and_compare(ctx, model, [s, prot.lower()], f"L={L}")
        assert res["stats"]["waves_per_block"] == waves


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------
def test_guards(ctx, models):
    from megagta_amd import api
    L = ctx._L
    hm, dev, _ = models.of_protein("ACDEF", "guard5")
    off = np.array([0, 4, 8], dtype=np.uint64)
    recs = np.zeros(2, dtype=api.ALIGN_REC)
    recs_raw = recs.view(np.uint8)
    recs_raw[:] = 77
    cols, path, plen = np.full(10, 77, dtype=np.uint8), np.full(8 + 10, 77, dtype=np.uint8), np.full(2, 77, dtype=np.int32)
    outs = (recs.ctypes.data, cols.ctypes.data, path.ctypes.data, plen.ctypes.data)
    args = (b"acdeacde", off.ctypes.data, 2)
    assert L.mgta_seqs_align(None, dev.h, *args, *outs, None) == -1 and b"ctx" in L.mgta_last_error()
    assert L.mgta_seqs_align(ctx.h, None, *args, *outs, None) == -1 and b"model" in L.mgta_last_error()
    assert L.mgta_seqs_align(ctx.h, dev.h, b"acdeacde", None, 2, *outs, None) == -1 and b"offsets" in L.mgta_last_error()
    assert L.mgta_seqs_align(ctx.h, dev.h, b"acdeacde", off.ctypes.data, -1, *outs, None) == -1 and b"n = -1" in L.mgta_last_error()
    assert L.mgta_seqs_align(ctx.h, dev.h, *args, None, *outs[1:], None) == -1 and b"recs" in L.mgta_last_error()
    assert L.mgta_seqs_align(ctx.h, dev.h, *args, outs[0], outs[1], outs[2], None, None) == -1 and b"path_len" in L.mgta_last_error()
    down = np.array([0, 8, 4], dtype=np.uint64)
    assert L.mgta_seqs_align(ctx.h, dev.h, b"acdeacde", down.ctypes.data, 2, *outs, None) == -1 and b"offsets must ascend" in L.mgta_last_error()
    long_off = np.array([0, 4, 4 + MAX_LEN + 1], dtype=np.uint64)
    assert L.mgta_seqs_align(ctx.h, dev.h, b"a" * (MAX_LEN + 5), long_off.ctypes.data, 2, *outs, None) == -1
    assert str(MAX_LEN).encode() in L.mgta_last_error() and b"limit" in L.mgta_last_error()
    assert L.mgta_ctx_set_align_batch(ctx.h, -1) == -1 and b"cells" in L.mgta_last_error()
    assert L.mgta_ctx_set_align_batch(None, 8) == -1 and b"ctx" in L.mgta_last_error()
    assert (recs_raw == 77).all() and (cols == 77).all() and (path == 77).all() and (plen == 77).all()   # nothing was written by the refused calls
    assert L.mgta_seqs_align(ctx.h, dev.h, *args, *outs, None) == 0      # the same arguments with everything in place: a valid call
    w = restate(hm, "acde")
    assert recs["status"].tolist() == [0, 0] and bits(recs["score"][0]) == bits(recs["score"][1]) == bits(w["score"])
    assert cols.tobytes() == w["cols"] * 2 and plen.tolist() == [4, 4]
    assert path[0:4].tobytes() == path[4 + 5:4 + 5 + 4].tobytes() == b"MMMM" and (path[4:9] == 77).all()     # at offsets[i] + i * M
    assert L.mgta_seqs_align(ctx.h, dev.h, None, None, 0, None, None, None, None, None) == 0


# ---- 9. process boundary -----------------------------------------------------------------------------------------------------------
def test_one_shot_and_worker_write_the_same_files(ctx, models, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    rng = np.random.default_rng(15)
    hm, dev, hmm_path = models.toy()
    seqs = fragments(rng, consensus(hm).upper(), n_each=3) + ["", "MKV"]
    headers = [f"c{j} len={len(s)}" if j % 3 else f"c{j}" for j, s in enumerate(seqs)]
    prot = str(tmp_path / "p.fa")
    open(prot, "w").write("".join(f">{h}\n{s}\n" for h, s in zip(headers, seqs)))
    subprocess.run([BIN, "align", hmm_path, prot, str(tmp_path / "one")], check=True, capture_output=True, timeout=120)
    r = subprocess.run([BIN, "serve"], input=f"align\t{hmm_path}\t{prot}\t{tmp_path}/w\nquit\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0"], r.stderr[-2000:]
    res, wants = run_and_compare(ctx, models.toy(), seqs, "cli")
    want = {"_aligned.fasta": al.aligned_fasta_text(headers, seqs, res),
            "_aligned.txt": al.table_text([al.record_name(h) for h in headers], [len(s) for s in seqs], res["recs"])}
    for tail, text in want.items():
        assert open(f"{tmp_path}/one{tail}").read() == open(f"{tmp_path}/w{tail}").read() == text and len(text) > 0, tail
    rows = al.read_aligned_fasta(f"{tmp_path}/one_aligned.fasta")
    assert [h for h, _ in rows] == headers
    for (h, line), s, w in zip(rows, seqs, wants):
        assert al.a2m_columns(line).encode() == w["cols"] and len(line) == hm.M + w["n_insert"]
        if w["status"] == 0:
            assert "".join(c for c in line if c != "-").lower() == s.lower()
    back = al.read_table(f"{tmp_path}/one_aligned.txt")
    assert back["lens"].tolist() == [len(s) for s in seqs] and back["recs"]["status"].tolist() == [w["status"] for w in wants]


# ---- 10. driver end to end ---------------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_driver_align_end_to_end(golden_dir, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    mg = synth.make_metagenome(6000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)    # the sample of the other driver tests
    synth.write_fasta(mg.reads, str(tmp_path / "reads.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "45", "-t", "4", "--min-contig-len", "150"]
    trees = {}
    for name, extra in {"al": ["--align"], "plain": []}.items():
        out = tmp_path / name
        r = subprocess.run(base + ["-o", str(out)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
        trees[name] = _tree(str(out))
    d = "contigs/rplB/"
    new = {d + "prot_merged_aligned.fasta", d + "prot_merged_aligned.txt"}
    assert set(trees["al"]) - set(trees["plain"]) == new                  # files per gene ...
    assert not [f for f in trees["plain"] if "_aligned." in f]            # ... and none without the flag
    for f in set(trees["plain"]) - {"log", "opts.txt", "tmp/cp.txt"}:
        assert trees["al"][f] == trees["plain"][f], f
    # one record per input record, under its header, one A2M line each whose residues are the contig's
    lines = trees["al"][d + "prot_merged.fasta"].decode().splitlines()
    prot = [(h[1:], s) for h, s in zip(lines[0::2], lines[1::2])]
    assert len(prot) > 0
    rows = al.parse_aligned_fasta(trees["al"][d + "prot_merged_aligned.fasta"].decode())
    table = al.parse_table(trees["al"][d + "prot_merged_aligned.txt"].decode())
    assert len(rows) == len(prot) == len(table["names"])
    assert [h for h, _ in rows] == [h for h, _ in prot] and table["names"] == [al.record_name(h) for h, _ in prot]
    hm = H.parse_hmm(os.path.join(toy, "for_enone.hmm"))
    for (h, line), (_, s), r, n in zip(rows, prot, table["recs"], table["lens"]):
        w = restate(hm, s)
        assert n == len(s) and int(r["status"]) == w["status"] and al.a2m_columns(line).encode() == w["cols"]
        assert [int(r[f]) for f in ("model_from", "model_to", "n_match", "n_insert", "n_delete")] == [w[f] for f in ("model_from", "model_to", "n_match", "n_insert", "n_delete")]
        assert al.score_text(float(r["score"])) == al.score_text(w["score"])
    # one checkpoint for the flag's step (one gene) behind the six of a run without the flag, whose cp.txt is what it was
    assert trees["plain"]["tmp/cp.txt"].decode().splitlines() == [f"{i}\tdone" for i in range(6)]
    assert trees["al"]["tmp/cp.txt"].decode().splitlines() == [f"{i}\tdone" for i in range(6 + 1)]
    assert trees["al"]["log"].count(b"Aligning the contigs") == 1 and trees["plain"]["log"].count(b"Aligning the contigs") == 0
