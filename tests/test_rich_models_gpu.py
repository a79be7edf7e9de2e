"""Every kernel that reads a profile HMM -- the A* search, align, posterior, recruit -- on POSITION-SPECIFIC models (tests/rich_models.py).

The other suites feed these kernels models with one transition row for all nodes, m->i == m->d, i->m == i->i and two-valued match
columns, on which a table read one node off, two swapped transitions or two swapped letters compute the same numbers.  On the models
here they do not: tests/test_rich_models_host.py shows that each of six such mistakes, written into the model, changes what the yardsticks
say on exactly these inputs.  The yardsticks and their assertions are the other suites' own, imported: the reference's `probe astar`
goldens (tests/golden/richm) and the oracle for A*, `restate` for align and posterior, tests/recruit_ref.py for recruit."""
import os

import numpy as np
import pytest

from megagta_amd import hmm as hmmlib
from megagta_amd import posterior as po
from megagta_amd import synth
from tests import rich_models as R
from tests import test_align_gpu as TA
from tests import test_posterior_gpu as TP
from tests import test_recruit_gpu as TR
from tests.test_astar_gpu import _check_side, ctx, request_id, search_mode   # noqa: F401  (the fixtures of the A* suite, as they are)

pytestmark = pytest.mark.gpu
NEG = float("-inf")


# ---- A* ------------------------------------------------------------------------------------------------------------------------------
class _Case:
    """one case of tests/golden/richm on the device: graph, the two models, the reference's goldens; the oracle's graph when asked for"""

    def __init__(self, ctx, case, tmp):
        from megagta_amd import api
        self.case, self.c = case, R.RICHM_CASES[case]
        self.packed, self.start, self.gdir, self.gold = R.richm_case(case, tmp)
        self.g = api.Graph(ctx, ctx.build_sdbg(ctx.upload_reads(self.packed, self.start), 44))
        self.fpath, self.rpath = os.path.join(self.gdir, "for_enone.hmm"), os.path.join(self.gdir, "rev_enone.hmm")
        self.fw, self.rv = api.DeviceHmm(ctx, hmmlib.parse_hmm(self.fpath)), api.DeviceHmm(ctx, hmmlib.parse_hmm(self.rpath))
        self.mg = R.richm_inputs(case, os.path.join(tmp, "again"))[0]
        self._og = None

    def oracle_graph(self, oracle):
        if self._og is None:
            self._og = oracle.Graph(oracle.Stream.build(self.packed, self.start, 44, threads=8))
        return self._og

    def absent_seeds(self, oracle, n=20):
        """n seeds cut in frame from the gene's variants with one base changed, none of them a k-mer of the graph"""
        og, out = self.oracle_graph(oracle), []
        for kmer, pos in synth.synthetic_seeds(self.mg.genes[0], 45, 4 * n, seed=self.c["seed"]):
            kmer = kmer[:22] + "ACGT"[("ACGT".index(kmer[22]) + 1) % 4] + kmer[23:]
            if og.index_edge(kmer) < 0 and len(out) < n:
                out.append((kmer, pos - 1))
        assert len(out) == n
        return out


_cases = {}


@pytest.fixture(scope="module")
def cases(ctx, tmp_path_factory):
    def get(case):
        if case not in _cases:
            _cases[case] = _Case(ctx, case, str(tmp_path_factory.mktemp(case)))
        return _cases[case]
    yield get
    _cases.clear()


def _cold_vs_golden(c, st_lds):
    from megagta_amd import api
    gold = c.gold["cold"]
    res, st = api.astar_search(c.g, c.fw, c.rv, [r["kmer"] for r in gold], [r["start_state"] for r in gold], c.c["prune"], 0.5)
    assert st["hmm_in_lds"] == st_lds
    for r, ref in zip(res, gold):
        _check_side(r.right_side, ref["R"])
        _check_side(r.left_side, ref["L"])
        assert r.contig(ref["kmer"]) == ref["contig"]
    return res, st


@pytest.mark.parametrize("case", ["r75", "r130"])
def test_cold_vs_reference_every_lane_mode(cases, case, search_mode):
    """per seed, both sides: fields equal, fp64 scores bit-equal, closed-node counts equal, contig equal"""
    c = cases(case)
    assert len(c.gold["cold"]) == 40
    res, st = _cold_vs_golden(c, 1)
    if search_mode[1] and case == "r130":
        assert st["n_grown"] > 0 and st["n_rehash"] > 0 and st["n_retries"] == 0     # (prune 0: the searches outgrow a 128-node arena)


@pytest.mark.parametrize("case,search_mode", [("r600", (16, 0)), ("r600", (64, 0)), ("r700", (64, 0))], indirect=["search_mode"], ids=["r600-g16", "r600-g64", "r700-g64"])
def test_tables_in_device_memory_vs_reference(cases, case, search_mode):
    """astar_kernel<G, false>: the tables are read from device memory.  600 columns do not fit the LDS beside the heap tops of four searches
    per wavefront (g16); beside those of ONE search (g64) they still do -- as tests/test_astar_gpu.py says of m600 -- so r600 under g64 is
    the LDS kernel on a 600-column rich model, and r700 is the case that puts the 64-lane kernel on device memory"""
    c = cases(case)
    res, st = _cold_vs_golden(c, 1 if (case, request_id(search_mode)) == ("r600", "g64") else 0)
    assert st["max_search_expansions"] > 10000


@pytest.mark.parametrize("case", ["r75", "r130"])
def test_cold_vs_oracle_with_seeds_absent_from_the_graph(cases, oracle, case):
    """the goldens' seeds and 20 seeds that are no k-mer of the graph against the oracle's searcher, every count of a side"""
    from megagta_amd import api
    c = cases(case)
    seeds = [(r["kmer"], r["start_state"]) for r in c.gold["cold"]] + c.absent_seeds(oracle)
    res, st = api.astar_search(c.g, c.fw, c.rv, [s[0] for s in seeds], [s[1] for s in seeds], c.c["prune"], 0.5)
    S = oracle.Searcher(c.oracle_graph(oracle), oracle.Hmm(c.fpath), oracle.Hmm(c.rpath), c.c["prune"], 0.5)
    n_absent = 0
    for n, ((kmer, state), r) in enumerate(zip(seeds, res)):
        contig, Rs, Ls = S.search(kmer, state, cold=True)
        assert r.contig(kmer) == contig
        for got, ref in ((r.right_side, Rs), (r.left_side, Ls)):
            assert (got["ok"], got["n_closed"], got["n_expanded"], got["partial"], got["n_opened"]) == \
                   (ref.ok, ref.n_closed, ref.n_expanded, ref.partial, ref.n_opened)
            if ref.ok:
                assert got["real_score"] == ref.real_score and got["score"] == ref.score and got["fval"] == ref.fval
        if n >= len(c.gold["cold"]):                                      # an absent seed: nothing is expanded, the contig is the seed
            assert contig == kmer.lower() and Rs.n_expanded == Ls.n_expanded == 0
            n_absent += 1
    assert n_absent == 20


@pytest.mark.parametrize("window", [1, 16])
def test_windowed_warm_vs_oracle(cases, oracle, window):
    """r75 through the ordered-commit window: == the oracle run sequentially with the same rule; window 1 == the reference's warm golden"""
    from megagta_amd import api
    c = cases("r75")
    gold = c.gold["warm"]
    kmers, states = [r["kmer"] for r in gold], [r["start_state"] for r in gold]
    runs = [api.astar_search(c.g, c.fw, c.rv, kmers, states, 20, 0.5, cache_mode=window, cost_rate=0) for _ in range(2)]
    S = oracle.Searcher(c.oracle_graph(oracle), oracle.Hmm(c.fpath), oracle.Hmm(c.rpath), 20, 0.5)
    S.clear_cache()
    S.set_window(window)
    S.set_cost_rate(0)
    for i, (kmer, state) in enumerate(zip(kmers, states)):
        contig, Rs, Ls = S.search(kmer, state, cold=False)
        for res, _ in runs:
            r = res[i]
            assert r.contig(kmer) == contig, (window, i)
            for got, ref in ((r.right_side, Rs), (r.left_side, Ls)):
                assert got["ok"] == ref.ok and got["n_closed"] == ref.n_closed and got["n_expanded"] == ref.n_expanded
                if ref.ok:
                    assert got["real_score"] == ref.real_score and got["fval"] == ref.fval
            if window == 1:
                _check_side(r.right_side, gold[i]["R"])
                _check_side(r.left_side, gold[i]["L"])
                assert contig == gold[i]["contig"]
    cold = sum(r["R"]["closed"] + r["L"]["closed"] for r in c.gold["cold"])
    assert runs[0][1]["n_expansions"] < cold                              # the cache does short-cut on this model too


# ---- align, posterior, recruit -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(ctx, tmp_path_factory, golden_dir):
    return TA.Models(ctx, str(tmp_path_factory.mktemp("rich_models")), golden_dir)


_inputs = {}


def protein_case(models, name, tmp):
    """-> (model, sequences, reads, (insert-friendly nodes, delete-friendly stretches)): the inputs of tests/test_rich_models_host.py"""
    if name not in _inputs:
        if name == "r130":
            text = open(os.path.join(R.GOLDEN, "r130_for_enone.hmm")).read()
            cons, seed = R.richm_inputs("r130", tmp)[0].genes[0].consensus, R.RICHM_CASES["r130"]["model_seed"]
        else:
            cons, text, seed = R.rich_protein_model(name)
        model = models.from_text(f"rich{name}", text)
        seqs = [s for _, s in R.rich_sequences(model[0], cons, seed)]
        _inputs[name] = (model, seqs, R.rich_reads(seqs, seed), R.rich_layout(len(cons), seed))
    return _inputs[name]


NAMES = list(R.PROTEIN_MS) + ["r130"]


@pytest.mark.parametrize("name", NAMES)
def test_align_vs_restatement(ctx, models, tmp_path, name):
    model, seqs, _, (ins, dels) = protein_case(models, name, str(tmp_path))
    res, wants = TA.run_and_compare(ctx, model, seqs, f"rich {name}")     # records (the score's 8 bytes), columns and paths
    assert res["stats"]["msc_in_lds"] == 1
    if model[0].M >= 63:
        nodes_i, nodes_d = set(), set()
        for path, rec in zip(res["paths"], res["recs"]):                  # the DEVICE's paths: insert labels and delete gaps
            j = int(rec["model_from"])
            for st in path[1:]:
                if st == "I":
                    nodes_i.add(j)
                else:
                    j += 1
                    if st == "D":
                        nodes_d.add(j)
        assert nodes_i and nodes_d and len(nodes_i | nodes_d) >= 3, (nodes_i, nodes_d)
        assert nodes_i & set(ins) and nodes_d & {j for a, b in dels for j in range(a, b + 1)}     # where the model invites them
        labels = po.labels_of(res, seqs)
        assert any(l < 0 for lab in labels for l in lab)


@pytest.mark.parametrize("name", NAMES)
def test_posterior_vs_restatement(ctx, models, tmp_path, name):
    model, seqs, _, _ = protein_case(models, name, str(tmp_path))
    res, wants, labels = TP.run_and_compare(ctx, model, seqs, f"rich {name}")      # fwd, bwd, pp, column sums: the derived tolerance
    assert res["stats"]["msc_in_lds"] == 1
    assert any(w["status"] == 0 for w in wants)
    print(name, TP.WORST)


@pytest.mark.parametrize("reversed_storage", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_recruit_vs_both_yardsticks(ctx, models, tmp_path, name, reversed_storage):
    """reads coding for the sequences in all six frames, both storage orders: yardstick (b) around the device's align and yardstick (a) in
    plain Python, on every read (min_aa 1, no threshold: the short ones are scored too)"""
    model, seqs, reads, _ = protein_case(models, name, str(tmp_path))
    # (yardstick (a) never sees how the reads are stored: above 65 columns, where it takes seconds, it runs beside one of the two orders)
    got, want = TR.run_and_compare(ctx, model, reads, min_aa=1, min_score=NEG, what=f"rich {name}", reversed_storage=reversed_storage,
                                   plain=reversed_storage or model[0].M <= 65)
    if model[0].M >= 63:
        assert {w["frame"] for w in want["recs"] if w["status"] == 0} == set(range(6))
        assert any(w["model_from"] > 1 for w in want["recs"]) and any(0 < w["model_to"] < model[0].M for w in want["recs"])
    assert got["stats"]["msc_in_lds"] == 1


def test_protein_stages_with_the_match_scores_in_device_memory(ctx, models, tmp_path):
    """MSC_LDS == false: r600's forward model, four sequences of at most 80 residues, through the three stages"""
    _, gdir = R.richm_inputs("r600", str(tmp_path))
    model = models.from_text("rich600", open(os.path.join(gdir, "for_enone.hmm")).read())
    hm = model[0]
    assert hm.M == 600
    cons = R.richm_inputs("r600", str(tmp_path))[0].genes[0].consensus.lower()
    seed = R.RICHM_CASES["r600"]["model_seed"]
    ins, dels = R.rich_layout(600, seed)
    rng = np.random.default_rng(600)
    j, (d0, d1) = ins[len(ins) // 2], dels[len(dels) // 2]
    seqs = [cons[100:130],                                                           # a piece
            cons[j - 30:j] + "".join(R.AA[c] for c in rng.integers(0, 20, 3)) + cons[j:j + 40],   # a run behind an insert-friendly node
            cons[d0 - 41:d0 - 1] + cons[d1:d1 + 37],                                 # without a delete-friendly stretch
            R.emission_sample(hm, rng)[520:600]]                                     # the model's own emissions, up to the last column
    assert [len(s) for s in seqs] == [30, 73, 77, 80]
    res, wants = TA.run_and_compare(ctx, model, seqs, "rich 600")
    assert res["stats"]["msc_in_lds"] == 0 and wants[1]["n_insert"] >= 3 and wants[2]["n_delete"] == d1 - d0 + 1
    pres, _, _ = TP.run_and_compare(ctx, model, seqs, "rich 600")
    assert pres["stats"]["msc_in_lds"] == 0
    for reversed_storage in (True, False):
        got, want = TR.run_and_compare(ctx, model, R.rich_reads(seqs, seed), min_aa=1, min_score=NEG, what="rich 600", reversed_storage=reversed_storage, plain=True)
        assert got["stats"]["msc_in_lds"] == 0 and all(w["status"] == 0 for w in want["recs"])
