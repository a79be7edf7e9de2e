"""The pieces that align, posterior and nearest share (megagta_amd/csrc/seq_jobs.hpp and seq_dp.hpp: the batch cut, the forward sweep
over the model's strips, the traceback walk), pinned where the stages must agree with each other: the same batch switch cuts the same
batches in align and posterior and moves no output of either, Forward is never below Viterbi, the posterior of a residue in the state
Viterbi gave it is a probability, and a path's letters count what its record counts, in align and in nearest alike.  Small shapes: the
model widths round a strip edge (63, 64, 65) and over two strips (129), the sequence lengths 0, 1, 2, round a strip edge and over
two strips.  Nothing here needs a yardstick of its own: every equality holds for any correct implementation of include/megagta_hip.h."""
import numpy as np
import pytest

from megagta_amd import nearest as nr
from megagta_amd import posterior as po
from tests.test_align_gpu import AA, Models, consensus, protein

pytestmark = pytest.mark.gpu
WIDTHS = (63, 64, 65, 129)
LENGTHS = (1, 2, 63, 64, 65, 130)
SWITCHES = (1, None, 0)                      # cells of a batch: one, the longest sequence's (130 * M), the default


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def models(ctx, tmp_path_factory, golden_dir):
    return Models(ctx, str(tmp_path_factory.mktemp("shared_models")), golden_dir)


def sequences(hm, M):
    """14 sequences: none, and per length a piece of the model's consensus (repeated where L > M: inserts) and letters at random; one
    in lower case with letters no alphabet knows"""
    rng = np.random.default_rng(700 + M)
    cons = consensus(hm)
    seqs = [""]
    for L in LENGTHS:
        reps = cons * (L // M + 2)
        a = int(rng.integers(0, max(1, M - L + 1))) if L <= M else int(rng.integers(0, M))
        seqs.append(reps[a:a + L])
        seqs.append("".join(AA[c] for c in rng.integers(0, 20, L)).upper())
    odd = list((cons * 2)[:64].lower())
    odd[3], odd[40], odd[63] = "x", "*", "\x7f"
    seqs.append("".join(odd))
    return seqs


@pytest.fixture(scope="module")
def runs(ctx, models):
    """per model width: (model, sequences, align and posterior results under every batch switch), computed once"""
    made = {}

    def of(M):
        if M not in made:
            model = models.of_protein(protein(np.random.default_rng(600 + M), M), f"shared{M}")
            hm, dev, _ = model
            assert hm.M == M
            seqs = sequences(hm, M)
            al, post = [], []
            try:
                for c in SWITCHES:
                    cells = max(map(len, seqs)) * M if c is None else c
                    ctx.set_align_batch(cells)
                    ctx.set_posterior_batch(cells)
                    al.append(ctx.align(dev, seqs, cols=True, paths=True))
                    post.append(ctx.posterior(dev, seqs, cols=True))
            finally:
                ctx.set_align_batch(0)
                ctx.set_posterior_batch(0)
            made[M] = (model, seqs, al, post)
        return made[M]
    return of


@pytest.mark.parametrize("M", WIDTHS)
def test_align_and_posterior_cut_the_same_batches(runs, M):
    _, seqs, al, post = runs(M)
    for c, a, p in zip(SWITCHES, al, post):
        print("M", M, "switch", c, "align batches", a["stats"]["n_batches"], "posterior batches", p["stats"]["n_batches"], "cells", a["stats"]["n_cells"])
        if c != 0:
            assert a["stats"]["n_batches"] == p["stats"]["n_batches"], (M, c)
        assert a["stats"]["n_cells"] == p["stats"]["n_cells"] == sum(map(len, seqs)) * M
        # no output depends on the switch
        assert a["recs"].tobytes() == al[0]["recs"].tobytes() and a["cols"].tobytes() == al[0]["cols"].tobytes() and a["paths"] == al[0]["paths"], (M, c)
        assert p["recs"].tobytes() == post[0]["recs"].tobytes(), (M, c)
        assert p["col_match"].tobytes() == post[0]["col_match"].tobytes() and p["col_insert"].tobytes() == post[0]["col_insert"].tobytes(), (M, c)
    # one sequence per batch at one cell, and the longest alone in its batch at its own cells
    assert al[0]["stats"]["n_batches"] == len(seqs) and 1 < al[1]["stats"]["n_batches"] < len(seqs)
    a, p = al[0], post[0]
    assert [int(s) for s in a["recs"]["status"]] == [int(s) for s in p["recs"]["status"]]
    assert int(a["recs"]["status"][0]) == 1 and all(int(s) == 0 for s in a["recs"]["status"][1:])
    for i, s in enumerate(seqs):
        if int(a["recs"]["status"][i]) == 0:
            assert float(p["recs"]["fwd"][i]) >= float(a["recs"]["score"][i]), (M, i, float(p["recs"]["fwd"][i]), float(a["recs"]["score"][i]))


@pytest.mark.parametrize("M", WIDTHS)
def test_posterior_of_the_viterbi_labels_is_a_probability(ctx, runs, M):
    (hm, dev, _), seqs, al, post = runs(M)
    labels = po.labels_of(al[0], seqs)
    res = ctx.posterior(dev, seqs, labels=labels, cols=False)
    assert res["recs"].tobytes() == post[0]["recs"].tobytes()
    n_labelled = 0
    for i, (lab, pp) in enumerate(zip(labels, res["pp"])):
        assert len(lab) == len(pp) == len(seqs[i])
        if len(lab):
            assert all(v != 0 for v in lab), (M, i)                      # global in the sequence: every residue has a state
            print("M", M, "sequence", i, "pp min", float(pp.min()), "max", float(pp.max()))
            assert float(pp.min()) > 0.0 and float(pp.max()) <= 1.0, (M, i, float(pp.min()), float(pp.max()))
            n_labelled += len(lab)
    assert n_labelled == sum(map(len, seqs))


def counts(path):
    return path.count("M"), path.count("I"), path.count("D")


@pytest.mark.parametrize("M", WIDTHS)
def test_paths_count_what_the_records_count(ctx, models, runs, M):
    _, seqs, al, _ = runs(M)
    for r, path in zip(al[0]["recs"], al[0]["paths"]):
        assert counts(path) == (int(r["n_match"]), int(r["n_insert"]), int(r["n_delete"])) and len(path) == sum(counts(path))
    # nearest: the same sequences as contigs, the consensus of every model and a reference without residues as references
    refs = [consensus(runs(W)[0][0]) for W in WIDTHS] + [""]
    sub = nr.match_mismatch(5, -4)
    got = []
    try:
        for c in (1, 0):
            ctx.set_nearest_batch(c)
            got.append(ctx.nearest(seqs, refs, sub, 10, 1, paths=True))
    finally:
        ctx.set_nearest_batch(0)
    one, free = got
    assert one["recs"].tobytes() == free["recs"].tobytes() and one["paths"] == free["paths"]
    n_aligned = sum(int(r["status"]) == 0 for r in one["recs"])
    assert one["stats"]["n_batches"] == n_aligned == len(seqs) - 1 and free["stats"]["n_batches"] == 1
    for r, path in zip(one["recs"], one["paths"]):
        assert counts(path) == (int(r["n_match"]), int(r["n_insert"]), int(r["n_delete"])) and len(path) == sum(counts(path))
        assert (int(r["status"]) == 0) == (len(path) > 0)
