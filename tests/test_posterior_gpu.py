"""Forward score and posteriors on the device (Context.posterior / `megagta posterior` / `megagta.py --posterior`).

The yardstick is `restate` of tests/test_posterior_host.py: the rule of include/megagta_hip.h in Python floats, never the code under
test.  The tolerance is derived, not tuned: a chain of dependent cells has at most L + M links; lse does not amplify an input error; a
link adds at most a few roundings of a value no larger than S (the largest finite |value| in the restatement's six matrices for that
sequence) and a few ulps from exp and log of arguments of order 1.  Hence tol = 16 (L + M) 2^-53 max(1, S) for F, Bt and every exponent,
and for a probability |p_dev - p_ref| <= (expm1(3 tol) + (L + 1) 2^-52) p_ref + 1e-300, the (L + 1) term being for the column sums.
Every test prints the largest error it saw as a share of its bound."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from megagta_amd import align as al
from megagta_amd import hmm as H
from megagta_amd import posterior as po
from megagta_amd import synth
from tests import helpers as TH
from tests.test_align_gpu import Models, consensus, fragments, protein
from tests.test_posterior_host import pp_of, restate, tolerance, with_stars

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
AA = "acdefghiklmnpqrstvwy"
NEG = float("-inf")
MM, MI, MD, IM, II, DM, DD = range(7)
MAX_LEN = 4096
WORST = {"exponent": 0.0, "probability": 0.0}                             # largest error / bound seen by this module


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()
    print("largest error as a share of the derived bound:", WORST)


@pytest.fixture(scope="module")
def models(ctx, tmp_path_factory, golden_dir):
    return Models(ctx, str(tmp_path_factory.mktemp("posterior_models")), golden_dir)


def viterbi_labels(ctx, dev, seqs):
    res = ctx.align(dev, seqs, cols=True, paths=True)
    return po.labels_of(res, seqs), res


def near(got, want, tol, what):
    if want == NEG:
        assert got == NEG, what
        return
    assert not math.isnan(got) and abs(got - want) <= tol, what + (got, want, tol)
    if tol > 0:
        WORST["exponent"] = max(WORST["exponent"], abs(got - want) / tol)


def prob_near(got, want, tol, L, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and not np.isnan(got).any(), what
    bound = (math.expm1(3 * tol) + (L + 1) * 2.0 ** -52) * want + 1e-300
    err = np.abs(got - want)
    assert (err <= bound).all(), what + (float((err / bound).max()), int(np.argmax(err / bound)))
    if got.size:
        WORST["probability"] = max(WORST["probability"], float((err / bound).max()))


def assert_is(res, wants, seqs, labels, M, what=""):
    """every sequence, every output, against the restatement"""
    recs = res["recs"]
    assert len(recs) == len(wants) and res["col_match"].shape == res["col_insert"].shape == (len(wants), M)
    for i, w in enumerate(wants):
        L, tol = len(seqs[i]), tolerance(w)
        tag = (what, i, seqs[i][:30], L)
        assert int(recs["status"][i]) == w["status"], tag
        near(float(recs["fwd"][i]), w["fwd"], tol, tag + ("fwd",))
        near(float(recs["bwd"][i]), w["bwd"], tol, tag + ("bwd",))
        prob_near(res["col_match"][i], w["col_match"], tol, L, tag + ("col_match",))
        prob_near(res["col_insert"][i], w["col_insert"], tol, L, tag + ("col_insert",))
        if labels is not None:
            assert len(res["pp"][i]) == L
            prob_near(res["pp"][i], pp_of(w, labels[i]), tol, L, tag + ("pp",))
        # on the device's numbers alone: the posteriors of L residues sum to L
        total = float(res["col_match"][i].sum() + res["col_insert"][i].sum())
        if w["status"] == 0:
            assert abs(total - L) <= (L * M) * 2.0 ** -52 + 3 * tol * L, tag + (total,)
        else:
            assert total == 0 and float(recs["fwd"][i]) == float(recs["bwd"][i]) == NEG, tag
    st = res["stats"]
    assert st["n_seqs"] == len(wants) and st["n_unaligned"] == sum(w["status"] for w in wants) and st["n_scored"] == st["n_seqs"] - st["n_unaligned"]
    assert st["n_cells"] == sum(len(s) for s in seqs) * M
    for name in ("pp", "col_match", "col_insert"):
        if name in res:
            assert not any(np.isnan(np.asarray(a)).any() for a in (res[name] if name == "pp" else [res[name]])), name


def run_and_compare(ctx, model, seqs, what="", labels=None):
    hm, dev, _ = model
    if labels is None:
        labels, _ = viterbi_labels(ctx, dev, seqs)
    wants = [restate(hm, s) for s in seqs]
    res = ctx.posterior(dev, seqs, labels=labels, cols=True)
    assert_is(res, wants, seqs, labels, hm.M, what)
    return res, wants, labels


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
        reps = (cons * (L // M + 2))
        a = int(rng.integers(0, max(1, M - L + 1))) if L <= M else int(rng.integers(0, M))
        seqs.append(reps[a:a + L])                                        # a piece of the consensus (repeated where L > M: inserts)
        seqs.append("".join(AA[c] for c in rng.integers(0, 20, L)))       # and letters at random
    res, wants, labels = run_and_compare(ctx, model, seqs, f"M={M}")
    assert res["stats"]["msc_in_lds"] == 1 and res["stats"]["waves_per_block"] == 4
    if M > 2:
        assert any(l < 0 for lab in labels for l in lab)                  # L > M forces inserts: insert labels are exercised
    print("M", M, "blocks per CU", res["stats"]["blocks_per_cu"], "LDS", res["stats"]["lds_bytes"], WORST)


# ---- 2. labels are taken as given --------------------------------------------------------------------------------------------------
def test_labels_are_taken_as_given(ctx, models):
    rng = np.random.default_rng(31)
    model = models.toy()
    hm, dev, _ = model
    cons = consensus(hm)
    seqs = [cons[10:80], cons[30:50] + "kkw" + cons[50:90], "".join(AA[c] for c in rng.integers(0, 20, 70))]
    vit, _ = viterbi_labels(ctx, dev, seqs)
    labels = []
    for lab in vit:
        lab = list(lab)
        for r in range(len(lab)):
            kind = r % 4
            if kind == 0:                                                 # a match state off the Viterbi path
                lab[r] = (abs(lab[r]) + 1 + int(rng.integers(0, 3))) % hm.M + 1
            elif kind == 1:                                               # an insert state
                lab[r] = -int(rng.integers(1, hm.M))
            elif kind == 2:
                lab[r] = 0
        labels.append(lab)
    assert any(a != b for x, y in zip(labels, vit) for a, b in zip(x, y))
    res, wants, _ = run_and_compare(ctx, model, seqs, "given labels", labels=labels)
    for pp, lab in zip(res["pp"], labels):
        assert all(p == 0.0 for p, l in zip(pp, lab) if l == 0)
    # the extreme labels: match state M, insert state M - 1, match state 1
    edge = [[hm.M] * len(seqs[0]), [-(hm.M - 1)] * len(seqs[1]), [1] * len(seqs[2])]
    run_and_compare(ctx, model, seqs, "edge labels", labels=edge)
    # no labels: no pp, the same records and column sums
    bare = ctx.posterior(dev, seqs, labels=None, cols=True)
    assert "pp" not in bare and bare["recs"].tobytes() == res["recs"].tobytes() and bare["col_match"].tobytes() == res["col_match"].tobytes()
    none = ctx.posterior(dev, seqs, labels=None, cols=False)
    assert set(none) == {"recs", "stats"} and none["recs"].tobytes() == res["recs"].tobytes()


# ---- 3. -inf in the tables ---------------------------------------------------------------------------------------------------------
def test_minus_infinity_in_the_tables(ctx, models):
    cut_t = models.from_text("pstar_t", with_stars(synth.hmm_text("s", "AC"), trans_stars=[(1, MM)]))
    cut_e = models.from_text("pstar_e", with_stars(synth.hmm_text("s", "AC"), match_stars=[(2, "C")]))
    assert cut_t[0].tsc[MM, 1] == NEG and cut_e[0].msc[2, cut_e[0].alpha[ord("c")]] == NEG
    rng = np.random.default_rng(9)
    prot = protein(rng, 40)
    star40 = models.from_text("pstar40", with_stars(synth.hmm_text("s", prot), match_stars=[(10, prot[9]), (30, "W")], trans_stars=[(20, MM), (21, MD), (5, II)]))
    long_seqs = [prot[a:b].lower() for a, b in ((0, 40), (5, 25), (15, 30), (19, 21), (8, 12), (0, 10), (25, 35))] + [prot.lower()[:20] + "ww" + prot.lower()[20:], "w" * 45]
    for model, seqs in ((cut_t, ["ac", "a", "c", "aca"]), (cut_e, ["ac", "aa", "c", "a"]), (star40, long_seqs)):
        res, wants, _ = run_and_compare(ctx, model, seqs, f"stars M={model[0].M}")
        vit = ctx.align(model[1], seqs, cols=False, paths=False)
        assert res["recs"]["status"].tolist() == vit["recs"]["status"].tolist()       # unaligned exactly where align says so
        for i, w in enumerate(wants):
            if w["status"]:
                assert float(res["recs"]["fwd"][i]) == float(res["recs"]["bwd"][i]) == NEG
                assert not res["pp"][i].any() and not res["col_match"][i].any() and not res["col_insert"][i].any()
        assert not np.isnan(res["recs"]["fwd"]).any() and not np.isnan(res["recs"]["bwd"]).any()
        if model is not star40:
            assert wants[0]["status"] == 1 and any(w["status"] == 0 for w in wants[1:])
    assert any(w["status"] == 0 for w in wants)


# ---- 4. unknown and lower-case letters ---------------------------------------------------------------------------------------------
def test_unknown_and_lower_case_letters(ctx, models):
    rng = np.random.default_rng(6)
    model = models.of_protein(protein(rng, 70), "pcase70")
    cons = consensus(model[0])
    seqs = [cons[5:60], cons[5:30] + "x*x" + cons[33:60], cons[0:20] + "xx" + cons[20:40]]
    low, _, labels = run_and_compare(ctx, model, seqs, "lower")
    up, _, _ = run_and_compare(ctx, model, [s.upper() for s in seqs], "upper")
    mixed, _, _ = run_and_compare(ctx, model, ["".join(c.upper() if i % 3 else c for i, c in enumerate(s)) for s in seqs], "mixed")
    for other in (up, mixed):
        assert other["recs"].tobytes() == low["recs"].tobytes() and other["col_match"].tobytes() == low["col_match"].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(other["pp"], low["pp"]))
    assert run_and_compare(ctx, model, [s.encode() for s in seqs], "bytes")[0]["recs"].tobytes() == low["recs"].tobytes()
    # bytes without a column, 127 and above included, emit 0 in a match state
    run_and_compare(ctx, model, [b"acd\x7fef\x80\xffgh", b"\x00\x01", b"-.-", b"*x*"], "unknown bytes")


# ---- 5. batches --------------------------------------------------------------------------------------------------------------------
def test_batches_move_no_output(ctx, models):
    rng = np.random.default_rng(12)
    model = models.of_protein(protein(rng, 20), "pshort20")
    hm, dev, _ = model
    empty = ctx.posterior(dev, [], labels=[], cols=True)
    assert len(empty["recs"]) == 0 and empty["col_match"].shape == (0, 20) and empty["pp"] == [] and all(v == 0 for v in empty["stats"].values())
    cons = consensus(hm)
    seqs = ["", cons[3:12], "", cons, cons[:5] + "kk" + cons[5:], ""]
    for _ in range(300):
        n = int(rng.integers(1, 31))
        seqs.append("".join(AA[c] for c in rng.integers(0, 20, n)) if rng.integers(0, 2) else (cons * 2)[int(rng.integers(0, 20)):][:n])
    seqs[50] = ""
    labels, _ = viterbi_labels(ctx, dev, seqs)
    whole, wants, _ = run_and_compare(ctx, model, seqs, "one batch", labels=labels)
    assert [w["status"] for w in wants[:6]] == [1, 0, 1, 0, 0, 1] and whole["stats"]["n_batches"] == 1
    outs = []
    try:
        for cells in (1, 20 * 100, 0, 1, 20 * 100, 0):                    # every setting twice: across settings and across runs
            ctx.set_posterior_batch(cells)
            outs.append((cells, ctx.posterior(dev, seqs, labels=labels, cols=True)))
    finally:
        ctx.set_posterior_batch(0)
    n_empty = sum(1 for s in seqs if not s)                               # (empty sequences hold no cell: they share the last batch)
    assert n_empty == 4 and outs[0][1]["stats"]["n_batches"] == len(seqs) - (n_empty - 1)      # every other sequence a batch of its own
    assert 1 < outs[1][1]["stats"]["n_batches"] < len(seqs) - n_empty and outs[2][1]["stats"]["n_batches"] == 1
    for cells, res in outs:
        assert res["recs"].tobytes() == whole["recs"].tobytes(), cells    # the 8 bytes of every double
        assert res["col_match"].tobytes() == whole["col_match"].tobytes() and res["col_insert"].tobytes() == whole["col_insert"].tobytes(), cells
        assert all(a.tobytes() == b.tobytes() for a, b in zip(res["pp"], whole["pp"])), cells
        stable = {n: v for n, v in res["stats"].items() if n in ("n_seqs", "n_scored", "n_unaligned", "n_cells")}
        assert stable == {n: whole["stats"][n] for n in stable}
    # more sequences than waves in flight: a wave takes one sequence after another
    pick = rng.integers(0, len(seqs), 12000)
    many = ctx.posterior(dev, [seqs[i] for i in pick], labels=[labels[i] for i in pick], cols=True)
    assert many["stats"]["workgroups"] * many["stats"]["waves_per_block"] < 12000
    assert many["recs"]["fwd"].tobytes() == whole["recs"]["fwd"][pick].tobytes() and many["col_match"].tobytes() == whole["col_match"][pick].tobytes()
    assert all(many["pp"][k].tobytes() == whole["pp"][i].tobytes() for k, i in enumerate(pick))


# ---- 6. wide model from device memory ----------------------------------------------------------------------------------------------
def test_wide_model_from_device_memory(ctx, models, golden_dir, tmp_path):
    """The models of tests/golden/bigm whose match scores do not fit LDS are m600 and m1200 (regenerated from their seeds, as every
    test of them does); star.hmm of that directory has 12 columns and `*` entries, so its scores do fit.  Both are run: the
    1200-column model for the path through device memory, star.hmm for its tables."""
    rng = np.random.default_rng(13)
    _, gdir = TH.bigm_inputs("m1200", str(tmp_path))
    wide = models.from_text("bigm1200", open(os.path.join(gdir, "for_enone.hmm")).read())
    assert wide[0].M == 1200
    cons = consensus(wide[0])
    seqs = [cons[100:130], cons[1150:1200], cons[300:330] + cons[340:374], cons[630:670] + "kkk" + cons[670:707]]
    assert [len(s) for s in seqs] == [30, 50, 64, 80]
    res, _, _ = run_and_compare(ctx, wide, seqs, "M=1200")
    assert res["stats"]["msc_in_lds"] == 0                                # the match scores do not fit LDS: read from device memory
    star = models.from_text("bigm_star", open(os.path.join(golden_dir, "bigm", "star.hmm")).read())
    cons = consensus(star[0])
    seqs = [cons, cons[2:9], (cons * 7)[:80], "".join(AA[c] for c in rng.integers(0, 20, 40))]
    run_and_compare(ctx, star, seqs, "star.hmm")


# ---- 7. the longest sequence -------------------------------------------------------------------------------------------------------
def test_longest_sequence(ctx, models):
    from megagta_amd import api
    rng = np.random.default_rng(14)
    prot = protein(rng, 16)
    model = models.of_protein(prot, "plong16")
    hm, dev, _ = model
    s = "".join(AA[c] for c in rng.integers(0, 20, MAX_LEN))
    s = s[:2000] + prot.lower() + s[2016:]
    assert len(s) == MAX_LEN
    res, _, _ = run_and_compare(ctx, model, [s, prot.lower()], f"L={MAX_LEN}")
    assert res["stats"]["waves_per_block"] == 1
    with pytest.raises(api.MegaGtaError) as e:
        ctx.posterior(dev, [s + "a"], labels=None, cols=False)
    assert str(MAX_LEN) in str(e.value) and "limit" in str(e.value)


# ---- 8. guards ---------------------------------------------------------------------------------------------------------------------
def test_guards(ctx, models):
    from megagta_amd import api
    L = ctx._L
    hm, dev, _ = models.of_protein("ACDEF", "pguard5")
    other = api.Context(0)
    try:
        off = np.array([0, 4, 8], dtype=np.uint64)
        recs = np.zeros(2, dtype=api.POST_REC)
        recs.view(np.uint8)[:] = 77
        lab = np.array([1, 2, 3, 4, 1, -1, 2, 3], dtype=np.int32)
        pp, cm, ci = np.full(8, 7.0), np.full(10, 7.0), np.full(10, 7.0)
        args = (b"acdeacde", off.ctypes.data, 2)
        outs = (pp.ctypes.data, cm.ctypes.data, ci.ctypes.data)
        call = L.mgta_seqs_posterior
        assert call(None, dev.h, *args, lab.ctypes.data, recs.ctypes.data, *outs, None) == -1 and b"ctx" in L.mgta_last_error()
        assert call(ctx.h, None, *args, lab.ctypes.data, recs.ctypes.data, *outs, None) == -1 and b"model" in L.mgta_last_error()
        assert call(other.h, dev.h, *args, lab.ctypes.data, recs.ctypes.data, *outs, None) == -1 and b"another context" in L.mgta_last_error()
        assert call(ctx.h, dev.h, b"acdeacde", None, 2, lab.ctypes.data, recs.ctypes.data, *outs, None) == -1 and b"offsets" in L.mgta_last_error()
        assert call(ctx.h, dev.h, None, off.ctypes.data, 2, lab.ctypes.data, recs.ctypes.data, *outs, None) == -1 and b"seqs" in L.mgta_last_error()
        assert call(ctx.h, dev.h, b"acdeacde", off.ctypes.data, -1, lab.ctypes.data, recs.ctypes.data, *outs, None) == -1 and b"n = -1" in L.mgta_last_error()
        assert call(ctx.h, dev.h, *args, lab.ctypes.data, None, *outs, None) == -1 and b"recs" in L.mgta_last_error()
        assert call(ctx.h, dev.h, *args, None, recs.ctypes.data, *outs, None) == -1 and b"labels" in L.mgta_last_error()      # pp without labels
        down = np.array([0, 8, 4], dtype=np.uint64)
        assert call(ctx.h, dev.h, b"acdeacde", down.ctypes.data, 2, lab.ctypes.data, recs.ctypes.data, *outs, None) == -1 and b"offsets must ascend" in L.mgta_last_error()
        for at, bad in ((5, 6), (2, -5), (7, -6), (0, 1 << 30)):          # above M, -M, below -M, far out
            wrong = lab.copy()
            wrong[at] = bad
            assert call(ctx.h, dev.h, *args, wrong.ctypes.data, recs.ctypes.data, *outs, None) == -1
            msg = L.mgta_last_error()
            assert b"label %d" % bad in msg and b"sequence %d, residue %d" % (at // 4, at % 4) in msg, msg
        assert L.mgta_ctx_set_posterior_batch(ctx.h, -1) == -1 and b"cells" in L.mgta_last_error()
        assert L.mgta_ctx_set_posterior_batch(None, 8) == -1 and b"ctx" in L.mgta_last_error()
        assert (recs.view(np.uint8) == 77).all() and (pp == 7).all() and (cm == 7).all() and (ci == 7).all()      # nothing was written by the refused calls
        st = __import__("megagta_amd._lib", fromlist=["PostStats"]).PostStats()
        st.n_seqs = 5
        import ctypes
        assert call(ctx.h, dev.h, None, None, 0, None, None, None, None, None, ctypes.byref(st)) == 0 and all(v == 0 for v in st.as_dict().values())
        assert (recs.view(np.uint8) == 77).all() and (pp == 7).all()
        assert call(ctx.h, dev.h, *args, lab.ctypes.data, recs.ctypes.data, *outs, None) == 0          # the same arguments with everything in place
        w = restate(hm, "acde")
        assert recs["status"].tolist() == [0, 0] and abs(recs["fwd"][0] - w["fwd"]) <= tolerance(w) and recs["fwd"][0] == recs["fwd"][1]
        prob_near([pp[5], pp[0]], [w["PI"][2][1], w["PM"][1][1]], tolerance(w), 4, ("guards", "pp"))      # at offsets[i] + the residue's place
    finally:
        other.close()


# ---- 9. files ----------------------------------------------------------------------------------------------------------------------
def test_one_shot_and_worker_write_the_same_files(ctx, models, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    rng = np.random.default_rng(15)
    hm, dev, hmm_path = models.toy()
    seqs = fragments(rng, consensus(hm).upper(), n_each=3) + ["", "MKV", "".join(AA[c] for c in rng.integers(0, 20, 50))]
    headers = [f"c{j} len={len(s)}" if j % 3 else f"c{j}" for j, s in enumerate(seqs)]
    prot = str(tmp_path / "p.fa")
    open(prot, "w").write("".join(f">{h}\n{s}\n" for h, s in zip(headers, seqs)))
    subprocess.run([BIN, "posterior", hmm_path, prot, str(tmp_path / "one")], check=True, capture_output=True, timeout=120)
    r = subprocess.run([BIN, "serve"], input=f"align\t{hmm_path}\t{prot}\t{tmp_path}/w\nposterior\t{hmm_path}\t{prot}\t{tmp_path}/w\nquit\n", capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0", "DONE", "0"], r.stderr[-2000:]
    labels, ares = viterbi_labels(ctx, dev, seqs)
    pres = ctx.posterior(dev, seqs, labels=labels, cols=False)
    want = {"_posterior.txt": po.table_text([al.record_name(h) for h in headers], [len(s) for s in seqs], ares["recs"], pres["recs"], pres["pp"]),
            "_aligned_pp.fasta": po.pp_fasta_text(headers, ares, pres)}
    for tail, text in want.items():
        assert open(f"{tmp_path}/one{tail}").read() == open(f"{tmp_path}/w{tail}").read() == text and len(text) > 0, tail
    rows, a2m = po.read_pp_fasta(f"{tmp_path}/one_aligned_pp.fasta"), al.read_aligned_fasta(f"{tmp_path}/w_aligned.fasta")
    assert [h for h, _ in rows] == headers and [len(l) for _, l in rows] == [len(l) for _, l in a2m]
    back = po.read_table(f"{tmp_path}/one_posterior.txt")
    assert back["lens"].tolist() == [len(s) for s in seqs] and back["rows"]["status"].tolist() == pres["recs"]["status"].tolist()
    assert back["rows"]["mean_pp"][0] > 0.9 and back["rows"]["status"][-3] == 1       # a fragment of the consensus is placed with confidence


# ---- 10. driver --------------------------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_driver_posterior_end_to_end(golden_dir, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    mg = synth.make_metagenome(6000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)    # the sample of the other driver tests
    synth.write_fasta(mg.reads, str(tmp_path / "reads.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "45", "-t", "4", "--min-contig-len", "150"]
    r = subprocess.run(base + ["-o", str(tmp_path / "bad"), "--posterior"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--posterior needs --align" in r.stderr and not os.path.exists(tmp_path / "bad")
    trees = {}
    for name, extra in {"pp": ["--align", "--posterior"], "al": ["--align"]}.items():
        out = tmp_path / name
        r = subprocess.run(base + ["-o", str(out)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
        trees[name] = _tree(str(out))
    d = "contigs/rplB/"
    assert set(trees["pp"]) - set(trees["al"]) == {d + "prot_merged_posterior.txt", d + "prot_merged_aligned_pp.fasta"}
    assert not [f for f in trees["al"] if "_posterior." in f or "_aligned_pp." in f]
    for f in set(trees["al"]) - {"log", "opts.txt", "tmp/cp.txt"}:
        assert trees["pp"][f] == trees["al"][f], f
    # one checkpoint more than the run without the flag, whose cp.txt and log are what they were
    assert trees["al"]["tmp/cp.txt"].decode().splitlines() == [f"{i}\tdone" for i in range(7)]
    assert trees["pp"]["tmp/cp.txt"].decode().splitlines() == [f"{i}\tdone" for i in range(8)]
    assert trees["pp"]["log"].count(b"Scoring the placement") == 1 and trees["al"]["log"].count(b"Scoring the placement") == 0
    rows = po.parse_pp_fasta(trees["pp"][d + "prot_merged_aligned_pp.fasta"].decode())
    a2m = al.parse_aligned_fasta(trees["pp"][d + "prot_merged_aligned.fasta"].decode())
    table = po.parse_table(trees["pp"][d + "prot_merged_posterior.txt"].decode())
    vit = al.parse_table(trees["pp"][d + "prot_merged_aligned.txt"].decode())
    assert len(rows) == len(a2m) == len(table["names"]) > 0 and table["names"] == vit["names"]
    assert [h for h, _ in rows] == [h for h, _ in a2m] and [len(l) for _, l in rows] == [len(l) for _, l in a2m]
    hm = H.parse_hmm(os.path.join(toy, "for_enone.hmm"))
    lines = trees["pp"][d + "prot_merged.fasta"].decode().splitlines()
    for s, r, v in zip(lines[1::2], table["rows"], vit["recs"]):
        w = restate(hm, s)
        assert int(r["status"]) == w["status"] == int(v["status"])
        if w["status"] == 0:
            assert abs(r["fwd_nats"] - w["fwd"]) <= 5.1e-5 + tolerance(w) and abs(r["viterbi"] - float(v["score"])) <= 1e-9 and r["fwd_nats"] >= r["viterbi"] - 1e-4
