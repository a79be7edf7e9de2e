"""Position-specific profile HMMs (tests/rich_models.py, tests/golden/richm), without a device.

Every other model of the suite has one transition row for all its nodes, m->i == m->d, i->m == i->i and two-valued match columns.  Here:
  1. the committed rich models have the properties that make a misread table visible;
  2. (tests/test_hmm_parsers.py holds r75 and r130) both product parsers reproduce the reference's tables of r600, bit for bit;
  3. the oracle's searcher reproduces every `probe astar` line of the reference on the three cases;
  4. the yardsticks alone, run on six deliberately wrong models, change their answers on the inputs the GPU tests use: so a kernel with
     that mistake fails tests/test_rich_models_gpu.py;
  5. no search side of r75 or r130 closes more than 100 000 nodes."""
import json
import os
import subprocess

import numpy as np
import pytest

from megagta_amd import hmm as hmmlib
from tests import helpers as H
from tests import recruit_ref
from tests import rich_models as R
from tests.test_align_gpu import restate as viterbi
from tests.test_oracle_golden import _side_matches
from tests.test_posterior_host import restate as forward, tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
NEG = float("-inf")
MM, MI, MD, IM, II, DM, DD = range(7)
COMMITTED = [f"{case}_{d}_enone.hmm" for case in ("r75", "r130") for d in ("for", "rev")]


# ---- 1. the properties ---------------------------------------------------------------------------------------------------------------
def heuristic_branches(hm, pre, state_no):
    """hmm._heuristic's loop, counting the nodes at which it continues through D"""
    h, n_d = 0.0, 0
    for i in range(state_no + 1, hm.M + 1):
        if pre == "m":
            mt, dt = hm.tsc[MM, i - 1], hm.tsc[MD, i - 1]
        elif pre == "d":
            mt, dt = hm.tsc[DM, i - 1], hm.tsc[DD, i - 1]
        else:
            mt, dt = hm.tsc[IM, i - 1], NEG
        mt = mt + (float(hm.msc[i].max()) - hm.max_match[i])
        dt = dt - hm.max_match[i]
        if dt > mt and dt > NEG:
            h, pre, n_d = h + dt, "d", n_d + 1
        else:
            h, pre = h + mt, "m"
    return h, n_d


@pytest.mark.parametrize("name", COMMITTED)
def test_committed_models_are_position_specific(name):
    hm = hmmlib.parse_hmm(os.path.join(R.GOLDEN, name))
    M = hm.M
    for j in range(1, M):
        row = hm.tsc[:, j]
        assert len(set(row.tolist())) == 7, (j, row)                      # no two of a node's seven transitions are equal
        assert not np.array_equal(row, hm.tsc[:, j + 1]) and (j == 1 or not np.array_equal(row, hm.tsc[:, j - 1])), j
    for j in range(1, M + 1):
        assert len(set(hm.msc[j].tolist())) == 20, j                      # no two letters of a match row are equal
    assert len(set(hm.compo.tolist())) == 20
    assert hm.max_match[1:].max() - hm.max_match[1:].min() >= 2.0         # nats
    second = np.diff(hm.h[0], 2)
    assert np.abs(second).max() > 0.5, "h[0] is affine in the column"
    h0, n_d = heuristic_branches(hm, "m", 0)
    assert h0 == hm.h[0, 0] and n_d >= 1                                  # the copy is the loop, and it went through D
    for k, rows in enumerate("mid"):                                      # the three rows differ by more than constants
        assert heuristic_branches(hm, rows, 3)[0] == hm.h[k, 3]
    assert np.ptp(hm.h[0, 1:M - 1] - hm.h[2, 1:M - 1]) > 0.5 and np.ptp(hm.h[0, 1:M - 1] - hm.h[1, 1:M - 1]) > 0.5
    if name.startswith("r130"):
        assert np.isinf(hm.msc[1:]).sum() >= 10 and np.isinf(hm.tsc[MD, 1:M]).sum() >= 3 and np.isinf(hm.tsc[MI, 1:M]).sum() >= 3
    else:
        assert not np.isinf(hm.msc[1:]).any()


def test_generator_is_deterministic_and_respects_its_shape():
    cons, text, seed = R.rich_protein_model(64)
    assert R.rich_hmm_text("rich64", cons, seed) == text != R.rich_hmm_text("rich64", cons, seed + 1)
    ins, dels = R.rich_layout(64, seed)
    assert len(ins) >= 2 and len(dels) >= 2
    none = R.rich_hmm_text("x", cons, seed, n_insert=0, n_delete=0)
    assert R.rich_layout(64, seed, n_insert=0, n_delete=0) == ([], []) and none != text


# ---- 2. the parsers on r600 ----------------------------------------------------------------------------------------------------------
def test_parsers_reproduce_the_reference_tables_of_r600(tmp_path):
    meta = json.load(open(os.path.join(R.GOLDEN, "cases.json")))["r600"]
    _, gdir = R.richm_inputs("r600", str(tmp_path))
    for tag, name in (("for", "for_enone.hmm"), ("rev", "rev_enone.hmm")):
        hm = hmmlib.parse_hmm(os.path.join(gdir, name))
        got = dict(M=hm.M, A=hm.A, alpha=hm.alpha, msc=hm.msc, tsc=hm.tsc.T, maxm=hm.max_match, h=hm.h.T)
        assert hm.M == 600 and R.tables_md5(got) == meta["tables_md5"][tag], name
        if os.path.exists(BIN):
            out = subprocess.run([BIN, "hmmdump", os.path.join(gdir, name)], check=True, capture_output=True, text=True).stdout
            assert R.tables_md5(H.parse_probe_hmm(out.splitlines())) == meta["tables_md5"][tag], name


def test_tables_md5_sees_one_bit():
    t = H.parse_probe_hmm(H.gz_lines(os.path.join(R.GOLDEN, "r75_for_tables.txt.gz")))
    meta = json.load(open(os.path.join(R.GOLDEN, "cases.json")))["r75"]
    assert R.tables_md5(t) == meta["tables_md5"]["for"]
    t["h"][40][1] = float(np.nextafter(t["h"][40][1], 0.0))
    assert R.tables_md5(t) != meta["tables_md5"]["for"]


# ---- 3. the oracle's searcher is the reference's, and 5. what a side costs -----------------------------------------------------------
_graphs = {}


def case_graph(oracle, case, tmp):
    if case not in _graphs:
        packed, start, gdir, gold = R.richm_case(case, tmp)
        _graphs[case] = (oracle.Graph(oracle.Stream.build(packed, start, 44, threads=4)), gdir, gold)
    return _graphs[case]


@pytest.mark.parametrize("case,mode", [("r75", "cold"), ("r75", "warm"), ("r130", "cold"), ("r600", "cold"), ("r700", "cold")])
def test_oracle_searcher_vs_reference(oracle, tmp_path_factory, case, mode):
    g, gdir, gold = case_graph(oracle, case, str(tmp_path_factory.mktemp(case)))
    c = R.RICHM_CASES[case]
    S = oracle.Searcher(g, oracle.Hmm(os.path.join(gdir, "for_enone.hmm")), oracle.Hmm(os.path.join(gdir, "rev_enone.hmm")), c["prune"], 0.5)
    assert len(gold[mode]) == c["n_seeds"]
    for rec in gold[mode]:
        contig, Rs, Ls = S.search(rec["kmer"], rec["start_state"], cold=(mode == "cold"))
        _side_matches(Rs, rec["R"])
        _side_matches(Ls, rec["L"])
        assert contig == rec["contig"]
    if case in ("r75", "r130") and mode == "cold":                                 # the cost cap of the two cases every lane mode runs
        assert max(max(r["R"]["closed"], r["L"]["closed"]) for r in gold[mode]) <= 100000
    meta = json.load(open(os.path.join(R.GOLDEN, "cases.json")))[case]
    total = sum(r["R"]["closed"] + r["L"]["closed"] for r in gold["cold"])
    assert total == meta["closed_total"] and (case != "r600" or total <= meta["closed_total_m600"])
    assert sum(r["R"]["ok"] + r["L"]["ok"] for r in gold[mode]) >= len(gold[mode])        # (the searches do find paths)


# ---- 4. the fixtures can see the mistakes --------------------------------------------------------------------------------------------
def _wrong_dir(gdir, kind, tmp):
    d = os.path.join(tmp, kind)
    os.makedirs(d, exist_ok=True)
    for name in ("for_enone.hmm", "rev_enone.hmm"):
        with open(os.path.join(d, name), "w") as f:
            f.write(R.wrong_model_text(open(os.path.join(gdir, name)).read(), kind))
    return d


@pytest.mark.parametrize("kind", R.WRONG)
@pytest.mark.parametrize("case", ["r75", "r130"])
def test_astar_goldens_see_a_wrong_model(oracle, tmp_path_factory, case, kind):
    """the oracle on the mistaken tables gives another score, closed-node count or contig for one seed at least"""
    tmp = str(tmp_path_factory.mktemp(case + kind))
    g, gdir, gold = case_graph(oracle, case, tmp)
    d = _wrong_dir(gdir, kind, tmp)
    S = oracle.Searcher(g, oracle.Hmm(os.path.join(d, "for_enone.hmm")), oracle.Hmm(os.path.join(d, "rev_enone.hmm")), R.RICHM_CASES[case]["prune"], 0.5)
    n_changed = 0
    for rec in gold["cold"]:
        contig, Rs, Ls = S.search(rec["kmer"], rec["start_state"], cold=True)
        same = contig == rec["contig"]
        for res, ref in ((Rs, rec["R"]), (Ls, rec["L"])):
            same = same and res.ok == ref["ok"] and res.n_closed == ref["closed"] and (not ref["ok"] or (res.real_score == ref["real"] and res.score == ref["score"]))
        n_changed += not same
    print(case, kind, "changes", n_changed, "of", len(gold["cold"]), "seeds")
    assert n_changed >= 1


_protein = {}


def protein_case(name, tmp):
    """-> (model text, parsed model, [sequences], [reads]) of a rich protein-stage model; "r130" is that case's forward model"""
    if name not in _protein:
        if name == "r130":
            text = open(os.path.join(R.GOLDEN, "r130_for_enone.hmm")).read()
            cons, seed = R.richm_inputs("r130", os.path.join(tmp, "in"))[0].genes[0].consensus, R.RICHM_CASES["r130"]["model_seed"]
        else:
            cons, text, seed = R.rich_protein_model(name)
        hm = _parse(text, tmp, "right")
        seqs = [s for _, s in R.rich_sequences(hm, cons, seed)]
        _protein[name] = (text, hm, seqs, R.rich_reads(seqs, seed))
    return _protein[name]


def _parse(text, tmp, name):
    path = os.path.join(tmp, name + ".hmm")
    with open(path, "w") as f:
        f.write(text)
    return hmmlib.parse_hmm(path)


_right = {}


def right_answers(name, hm, seqs, reads):
    if name not in _right:
        _right[name] = ([viterbi(hm, s) for s in seqs], [forward(hm, s) for s in seqs],
                        [recruit_ref.recruit(hm, [r], 1, NEG)["recs"][0] for r in reads])
    return _right[name]


@pytest.mark.parametrize("kind", R.WRONG)
@pytest.mark.parametrize("name", [63, 64, 65, 129, "r130"])
def test_protein_stage_inputs_see_a_wrong_model(tmp_path_factory, name, kind):
    """restate of align, restate of posterior and the recruit yardstick, each on the mistaken model, over the sequences and reads of the
    GPU tests: an align record (score or path), a Forward score by more than ten times its tolerance, and a recruit record change"""
    tmp = str(tmp_path_factory.mktemp(f"p{name}{kind}"))
    text, hm, seqs, reads = protein_case(name, tmp)
    vit, fwd, rec = right_answers(name, hm, seqs, reads)
    bad = _parse(R.wrong_model_text(text, kind), tmp, kind)
    assert bad.M == hm.M and not (np.array_equal(bad.tsc, hm.tsc) and np.array_equal(bad.msc[1:], hm.msc[1:]))
    order = sorted(range(len(seqs)), key=lambda i: -len(seqs[i]))         # the long ones first: they cross most nodes
    seen = dict(align=None, posterior=None, recruit=None)
    for i in order:
        if seen["align"] is None:
            w = viterbi(bad, seqs[i])
            if (w["score"], w["path"], w["model_from"]) != (vit[i]["score"], vit[i]["path"], vit[i]["model_from"]):
                seen["align"] = i
        if seen["posterior"] is None:
            w = forward(bad, seqs[i])
            if w["status"] != fwd[i]["status"] or abs(w["fwd"] - fwd[i]["fwd"]) > 10 * tolerance(fwd[i]):
                seen["posterior"] = i
        if seen["recruit"] is None:
            if recruit_ref.recruit(bad, [reads[i]], 1, NEG)["recs"][0] != rec[i]:
                seen["recruit"] = i
        if None not in seen.values():
            break
    print(name, kind, "first input that sees it:", seen)
    assert None not in seen.values(), seen


@pytest.mark.parametrize("name", [63, 64, 65, 129, "r130"])
def test_best_paths_go_through_inserts_and_deletes(tmp_path_factory, name):
    """the Viterbi restatement on the GPU tests' sequences: I at the insert-friendly nodes, D over the delete-friendly stretches, at three
    distinct nodes or more"""
    text, hm, seqs, reads = protein_case(name, str(tmp_path_factory.mktemp(f"paths{name}")))
    vit = right_answers(name, hm, seqs, reads)[0]
    nodes_i, nodes_d = set(), set()
    for w in vit:
        j = w["model_from"]
        for st in w["path"][1:]:
            if st == "I":
                nodes_i.add(j)
            else:
                j += 1
                if st == "D":
                    nodes_d.add(j)
    assert nodes_i and nodes_d and len(nodes_i | nodes_d) >= 3, (nodes_i, nodes_d)
