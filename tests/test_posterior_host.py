"""Forward score and posteriors (megagta_amd/posterior.py and the rule of mgta_seqs_posterior), without a device.

`restate` is the yardstick of tests/test_posterior_gpu.py too: the rule of include/megagta_hip.h as nested Python loops over Python
floats, lse written as the text writes it (m + log of the sum of exp(. - m), every term evaluated).  Here it is checked against the
identities the rule promises: Forward and backward totals agree, the posteriors of every residue sum to 1, and F is never below the
score of the best single path (the Viterbi restatement of tests/test_align_gpu.py)."""
import math
import os

import numpy as np
import pytest

from megagta_amd import align as al
from megagta_amd import hmm as H
from megagta_amd import posterior as po
from megagta_amd import synth
from tests.test_align_gpu import consensus, restate as viterbi

NEG = float("-inf")
MM, MI, MD, IM, II, DM, DD = range(7)
AA = "acdefghiklmnpqrstvwy"


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------
def lse(*v):
    m = max(v)
    if m == NEG:
        return NEG                                                        # (-inf - -inf is never evaluated)
    return m + math.log(sum(math.exp(x - m) for x in v))


def restate(hm, seq):
    """-> dict(status, fwd, bwd, PM, PI ([L + 2][M + 2] lists, row i and column j 1-based), col_match, col_insert ([M]), S (the largest
    finite |value| of the six matrices), L, M)"""
    if isinstance(seq, str):
        seq = seq.encode("latin-1")
    M, L = hm.M, len(seq)
    msc, tsc, alpha = hm.msc.tolist(), hm.tsc.tolist(), hm.alpha.tolist()
    tMM, tMI, tMD, tIM, tII, tDM, tDD = tsc
    zeros = lambda: [[0.0] * (M + 2) for _ in range(L + 2)]               # noqa: E731
    out = dict(status=1, fwd=NEG, bwd=NEG, PM=zeros(), PI=zeros(), col_match=[0.0] * M, col_insert=[0.0] * M, S=0.0, L=L, M=M)
    if L == 0:
        return out
    e = [None] * (L + 2)
    for i in range(1, L + 1):
        x = seq[i - 1]
        a = alpha[x] if x < 127 else -1
        e[i] = [0.0] + [(msc[j][a] if a >= 0 else 0.0) for j in range(1, M + 1)] + [NEG]
    e[L + 1] = [NEG] * (M + 2)
    table = lambda: [[NEG] * (M + 2) for _ in range(L + 2)]               # noqa: E731  (whatever is not defined is -inf)
    FM, FI, FD, BM, BI, BD = table(), table(), table(), table(), table(), table()
    log, exp = math.log, math.exp
    for i in range(1, L + 1):
        fm, fi, fd, ei = FM[i], FI[i], FD[i], e[i]
        pm, pi, pd = FM[i - 1], FI[i - 1], FD[i - 1]
        for j in range(1, M + 1):
            if i == 1:
                fm[j] = ei[j]
                continue
            if j > 1:
                a, b, c = pm[j - 1] + tMM[j - 1], pi[j - 1] + tIM[j - 1], pd[j - 1] + tDM[j - 1]
                m = max(a, b, c)
                fm[j] = (NEG if m == NEG else m + log(exp(a - m) + exp(b - m) + exp(c - m))) + ei[j]
                a, b = fm[j - 1] + tMD[j - 1], fd[j - 1] + tDD[j - 1]
                m = max(a, b)
                fd[j] = NEG if m == NEG else m + log(exp(a - m) + exp(b - m))
            if j < M:
                a, b = pm[j] + tMI[j], pi[j] + tII[j]
                m = max(a, b)
                fi[j] = NEG if m == NEG else m + log(exp(a - m) + exp(b - m))
    F = lse(*FM[L][1:M + 1])
    for j in range(1, M + 1):
        BM[L][j] = 0.0
    for i in range(L - 1, 0, -1):
        bm, bi, bd, nm, ni, en = BM[i], BI[i], BD[i], BM[i + 1], BI[i + 1], e[i + 1]
        for j in range(M, 0, -1):
            N = en[j + 1] + nm[j + 1] if j < M else NEG
            terms = [tMM[j] + N]
            if j < M:
                terms.append(tMI[j] + ni[j])
                if i > 1:
                    terms.append(tMD[j] + bd[j + 1])
            bm[j] = lse(*terms)
            if i > 1 and j < M:
                bi[j] = lse(tIM[j] + N, tII[j] + ni[j])
                if j > 1:
                    bd[j] = lse(tDM[j] + N, tDD[j] + bd[j + 1])
    Bt = lse(*[e[1][j] + BM[1][j] for j in range(1, M + 1)])
    S = 0.0
    for T in (FM, FI, FD, BM, BI, BD):
        for row in T:
            for v in row:
                if v != NEG and abs(v) > S:
                    S = abs(v)
    out.update(S=S, FM=FM, FI=FI, BM=BM, BI=BI)
    if F == NEG:
        return out
    PM, PI = out["PM"], out["PI"]
    for i in range(1, L + 1):
        for j in range(1, M + 1):
            if FM[i][j] != NEG and BM[i][j] != NEG:
                PM[i][j] = exp(FM[i][j] + BM[i][j] - F)
            if FI[i][j] != NEG and BI[i][j] != NEG:
                PI[i][j] = exp(FI[i][j] + BI[i][j] - F)
    out.update(status=0, fwd=F, bwd=Bt,
               col_match=[sum(PM[i][j] for i in range(L, 0, -1)) for j in range(1, M + 1)],
               col_insert=[sum(PI[i][j] for i in range(L, 0, -1)) for j in range(1, M + 1)])
    return out


def tolerance(w):
    """16 (L + M) 2^-53 max(1, S): a chain of dependent cells has at most L + M links, lse does not amplify an input error, a link adds
    a few roundings of a value no larger than S and a few ulps from exp and log of arguments of order 1"""
    return 16.0 * (w["L"] + w["M"]) * 2.0 ** -53 * max(1.0, w["S"])


def pp_of(w, labels):
    """the posterior the restatement gives the state every label names"""
    return [w["PM"][i + 1][l] if l > 0 else w["PI"][i + 1][-l] if l < 0 else 0.0 for i, l in enumerate(labels)]


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


def model_of_text(tmp, name, text):
    path = os.path.join(str(tmp), name + ".hmm")
    with open(path, "w") as fh:
        fh.write(text)
    return H.parse_hmm(path)


@pytest.fixture(scope="module")
def toy(golden_dir):
    return H.parse_hmm(os.path.join(golden_dir, "toy", "for_enone.hmm"))


# ---- the PP code and the labels ----------------------------------------------------------------------------------------------------
def test_pp_char_at_the_edges():
    assert [po.pp_char(p) for p in (0, 0.0499, 0.05, 0.9499, 0.95, 1.0)] == ["0", "0", "1", "9", "*", "*"]
    assert [po.pp_char(p) for p in (0.149, 0.15, 0.5, 0.849, 0.85)] == ["1", "2", "5", "8", "9"]


def test_labels_from_path():
    assert po.labels_from_path("MMM", 1) == [1, 2, 3]
    assert po.labels_from_path("MMM", 5) == [5, 6, 7]
    assert po.labels_from_path("MIIM", 2) == [2, -2, -2, 3]
    assert po.labels_from_path("MDDM", 1) == [1, 4]
    assert po.labels_from_path("MIDMDIM", 3) == [3, -3, 5, -6, 7]          # (any path is walked, also one the rule never makes)
    assert po.labels_from_path("MDMIM", 3) == [3, 5, -5, 6]
    assert po.labels_from_path("", 0, 4) == [0, 0, 0, 0] and po.labels_from_path("", 0) == []
    with pytest.raises(ValueError):
        po.labels_from_path("MXM", 1)


# ---- the files ---------------------------------------------------------------------------------------------------------------------
def fake_results(hm, seqs):
    """what Context.align and Context.posterior would return, from the two restatements"""
    wants = [viterbi(hm, s) for s in seqs]
    recs = np.zeros(len(seqs), dtype=al.REC)
    for i, w in enumerate(wants):
        recs[i] = (w["score"], w["status"], w["model_from"], w["model_to"], w["n_match"], w["n_insert"], w["n_delete"])
    align = dict(recs=recs, cols=np.array([list(w["cols"]) for w in wants], dtype=np.uint8).reshape(len(seqs), hm.M), paths=[w["path"] for w in wants])
    labels = po.labels_of(align, seqs)
    posts = [restate(hm, s) for s in seqs]
    prec = np.zeros(len(seqs), dtype=[("fwd", np.float64), ("bwd", np.float64), ("status", np.int32), ("pad", np.int32)])
    for i, w in enumerate(posts):
        prec[i] = (w["fwd"], w["bwd"], w["status"], 0)
    return align, dict(recs=prec, pp=[np.array(pp_of(w, l), dtype=np.float64) for w, l in zip(posts, labels)]), wants, posts


def test_writers_round_trip_and_line_lengths(toy, tmp_path):
    rng = np.random.default_rng(21)
    cons = consensus(toy)
    seqs = [cons[10:60], cons[5:30] + "kwkw" + cons[30:50], cons[0:20] + cons[26:70], "".join(AA[c] for c in rng.integers(0, 20, 30)), "", "MKV"]
    headers = [f"c{j} len={len(s)}" if j % 2 else f"c{j}" for j, s in enumerate(seqs)]
    align, post, wants, posts = fake_results(toy, seqs)
    assert any(w["n_insert"] for w in wants) and any(w["n_delete"] for w in wants) and wants[4]["status"] == 1
    prefix = str(tmp_path / "x")
    po.write_posterior(prefix, headers, seqs, align, post)
    al.write_align(prefix, headers, seqs, align)
    rows = po.read_pp_fasta(prefix + "_aligned_pp.fasta")
    a2m = al.read_aligned_fasta(prefix + "_aligned.fasta")
    assert [h for h, _ in rows] == headers == [h for h, _ in a2m]
    for (_, line), (_, row), w, p, s in zip(rows, a2m, wants, post["pp"], seqs):
        assert len(line) == len(row) == toy.M + w["n_insert"]
        # a dot exactly where the row holds `-`; elsewhere the code of that residue's posterior, in residue order
        assert [c == "." for c in line] == [c == "-" for c in row]
        assert [c for c in line if c != "."] == ([po.pp_char(v) for v in p] if w["status"] == 0 else [])
    back = po.read_table(prefix + "_posterior.txt")
    assert back["names"] == [al.record_name(h) for h in headers] and back["lens"].tolist() == [len(s) for s in seqs]
    for i, (w, v) in enumerate(zip(posts, wants)):
        r = back["rows"][i]
        assert int(r["status"]) == w["status"]
        if w["status"]:
            assert r["fwd_nats"] == r["fwd_bits"] == r["viterbi"] == NEG and r["mean_pp"] == r["min_pp"] == 0 and r["n_below_half"] == 0
            continue
        p = post["pp"][i]
        assert abs(r["fwd_nats"] - w["fwd"]) <= 5.1e-5 and abs(r["fwd_bits"] - w["fwd"] / math.log(2)) <= 5.1e-5 and abs(r["viterbi"] - v["score"]) <= 5.1e-5
        assert abs(r["mean_pp"] - float(np.mean(p))) <= 5.1e-5 and abs(r["min_pp"] - float(p.min())) <= 5.1e-5 and r["n_below_half"] == int((p < 0.5).sum())
    assert open(prefix + "_posterior.txt").read() == po.table_text(back["names"], back["lens"], align["recs"], post["recs"], post["pp"])
    with pytest.raises(ValueError):
        po.parse_table("no header\n")
    with pytest.raises(ValueError):
        po.parse_pp_fasta(">a\nAB\n")


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def check_identities(hm, seq):
    w, v = restate(hm, seq), viterbi(hm, seq)
    tol = tolerance(w)
    assert (w["fwd"] == NEG) == (v["score"] == NEG) and w["status"] == v["status"]
    if w["status"]:
        assert w["bwd"] == NEG and not any(any(r) for r in w["PM"]) and not any(any(r) for r in w["PI"])
        return w
    assert abs(w["fwd"] - w["bwd"]) <= tol, (w["fwd"], w["bwd"], tol)
    assert w["fwd"] >= v["score"] - tol
    for i in range(1, w["L"] + 1):
        total = sum(w["PM"][i][1:hm.M + 1]) + sum(w["PI"][i][1:hm.M + 1])
        assert abs(total - 1.0) <= 3 * tol, (i, total, tol)
    assert not any(math.isnan(x) for r in w["PM"] + w["PI"] for x in r)
    return w


def test_rule_on_the_toy_model(toy):
    rng = np.random.default_rng(22)
    cons = consensus(toy)
    piece = check_identities(toy, cons[20:70])
    lab = po.labels_from_path(viterbi(toy, cons[20:70])["path"], 21)
    assert min(pp_of(piece, lab)) > 0.99                                  # a piece of the consensus sits where Viterbi puts it
    rand = check_identities(toy, "".join(AA[c] for c in rng.integers(0, 20, 50)))
    v = viterbi(toy, "".join(AA[c] for c in np.random.default_rng(22).integers(0, 20, 50)))
    assert rand["fwd"] > v["score"] + 1.0                                 # a random protein has many paths: F is well above the best one
    one = check_identities(toy, "w")
    assert one["L"] == 1 and one["fwd"] == one["bwd"]
    check_identities(toy, "")
    check_identities(toy, "ax*" + cons[3:20] + "\x7f\xff")


def test_rule_with_minus_infinity_in_the_tables(tmp_path):
    cut_t = model_of_text(tmp_path, "star_t", with_stars(synth.hmm_text("s", "AC"), trans_stars=[(1, MM)]))
    cut_e = model_of_text(tmp_path, "star_e", with_stars(synth.hmm_text("s", "AC"), match_stars=[(2, "C")]))
    assert cut_t.tsc[MM, 1] == NEG and cut_e.msc[2, cut_e.alpha[ord("c")]] == NEG
    for hm, seqs in ((cut_t, ["ac", "a", "c", "aca"]), (cut_e, ["ac", "aa", "c", "a"])):
        ws = [check_identities(hm, s) for s in seqs]
        assert ws[0]["status"] == 1 and any(w["status"] == 0 for w in ws[1:])
    rng = np.random.default_rng(9)
    prot = "".join(AA[c] for c in rng.integers(0, 20, 40)).upper()
    hm = model_of_text(tmp_path, "star40", with_stars(synth.hmm_text("s", prot), match_stars=[(10, prot[9]), (30, "W")], trans_stars=[(20, MM), (21, MD), (5, II)]))
    for s in [prot[a:b].lower() for a, b in ((0, 40), (5, 25), (19, 21), (8, 12))] + [prot.lower()[:20] + "ww" + prot.lower()[20:], "w" * 45]:
        check_identities(hm, s)
