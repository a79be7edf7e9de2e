"""`denovo` on designed graphs (tests/denovo_shapes.py) that sit on its limits, one input on either side of each:

  tip length      a tip of t nodes goes iff t <= max_tip_len - 1                       (Trim's `i < len`, the device's `s < len`)
  bubble length   linked SNPs spanning k + 1 bases pop, k + 2 do not                  (`j < max_len`, max_len = 2k + 4)
  branch count    16 haplotypes in one window are a candidate, 17 are not             (`> kMaxBranches`)
  reach walk      regions of 16384 / 16385 edges, levels of 2048 / 2049 edges         (`seen > limit`, `at >= kReachFrontier`), and the
                  fans of the narrow walk, the wide walk and the two ways of not fitting, with no knob set
  the tie         which allele survives a bubble of equal weights, on either strand   (the `>=` of Pop)
  closed shapes   a ring and a ring with a bubble: no edge ends a path

References, in order of authority: the reference binary's one-thread files (tests/golden/denovo_limits, made by
tests/golden/make_golden_denovo_limits.py), the oracle, and numbers derived from the rules (denovo_shapes: the generators state them, the
restated Search and the model of the ordered rounds over tests/graph_nav_ref.py confirm them without the device or the oracle's denovo).
CPU: the oracle and the restatements against the files and the derived numbers.  GPU: the device against all three."""
import functools
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

from megagta_amd import readlib
from tests import denovo_shapes as D
from tests.graph_nav_ref import NavRef

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denovo_limits")
CANDIDATE_SHAPES = D.SPAN_SHAPES + D.BRANCH_SHAPES + D.SITE_SHAPES          # small enough for a search from every branching edge


@functools.lru_cache(maxsize=None)
def _golden():
    with open(os.path.join(GOLDEN, "expected.json")) as f:
        return json.load(f)


_SHAPES = {}


def _shape(oracle, name):
    """-> (reads, info, the oracle's stream), made once per process"""
    if name not in _SHAPES:
        reads, info = D.make(name)
        packed, start = readlib.pack_for_build(D.as_arrays(reads))
        _SHAPES[name] = (reads, info, oracle.Stream.build(packed, start, info["k"], threads=4), (packed, start))
    return _SHAPES[name][:3]


def _same_text(text, run):
    if "contigs" in run:
        return text == run["contigs"]
    return hashlib.sha256(text.encode()).hexdigest() == run["contigs_sha256"]


def _expected(info, run):
    """what the rules say about one run of a shape: only the keys the shape states"""
    tip, no_bubble, _ = run
    want = {"n_tips": info["n_tips"][tip] if "n_tips" in info else 0}           # (only the tip shapes have tips, at any setting)
    if not no_bubble:
        for key in ("n_bubbles", "n_contigs"):
            if key in info:
                want[key] = info[key]
    return want


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.GOLDEN_SHAPES)
def test_fixture_is_the_generated_shape(name):
    """the committed reads are the generator's: what the reference binary saw is what the tests build"""
    with gzip.open(os.path.join(GOLDEN, name + ".fa.gz"), "rt") as f:
        stored = [l.strip() for l in f if not l.startswith(">")]
    reads, info = D.make(name)
    assert stored == reads
    assert [(r["max_tip_len"], r["no_bubble"], r["min_contig"]) for r in _golden()[name]["runs"]] == [tuple(r) for r in info["runs"]]


@pytest.mark.parametrize("name", D.GOLDEN_SHAPES)
def test_oracle_vs_reference_one_thread(oracle, name):
    """the oracle's denovo equals the reference binary's one-thread files on every designed shape, and both give the derived counts"""
    _, info, st = _shape(oracle, name)
    for run, gold in zip(info["runs"], _golden()[name]["runs"]):
        text, stats = oracle.Graph(st).denovo(*run)
        assert _same_text(text, gold), (name, run)
        assert f"{stats['n_contigs']} {stats['total_len']}\n" == gold["info"]
        want = _expected(info, run)
        assert {key: stats[key] for key in want} == want, (name, run)


@pytest.mark.parametrize("name", D.CHAIN_SHAPES)
def test_oracle_on_chains(oracle, name):
    _, info, st = _shape(oracle, name)
    _, stats = oracle.Graph(st).denovo(0, False, 0)
    assert (stats["n_tips"], stats["n_bubbles"]) == (0, info["n_bubbles"])


def test_tip_lengths_on_both_sides():
    """every max_tip_len the tip shapes run with has a tip of T - 1 nodes (goes) and one of T nodes (stays)"""
    for T in D.TIP_RUNS:
        if T:
            t_max = (42 if T == -1 else T) - 1
            assert t_max in D.TIP_T and t_max + 1 in D.TIP_T and t_max + 2 in D.TIP_T
            assert D.tips_removed(t_max, T, 21) and not D.tips_removed(t_max + 1, T, 21)


@pytest.mark.parametrize("name", D.SITE_SHAPES)
def test_tie_survivors_in_reference_contigs(name):
    """one contig; it runs through one of the two alleles the tie rule keeps (one per strand) and through no other"""
    _, info = D.make(name)
    for gold in _golden()[name]["runs"]:
        text = gold["contigs"]
        has = lambda w: w in text or D.revcomp(w) in text
        assert gold["info"].split()[0] == "1"
        assert sum(has(w) for w in info["survivors"]) == 1 and not any(has(w) for w in info["losers"]), name


@pytest.mark.parametrize("name", CANDIDATE_SHAPES)
def test_search_restatement_and_rounds(oracle, name):
    """BranchGroup::Search restated over the numpy graph: the candidates are the designed ones -- the window's begin edges up to k + 1
    bases of span and up to 16 branches, nothing beyond -- and one more step / one branch more or less moves exactly the shapes that sit
    on the limit.  Then the ordered rounds as the device's rules state them: the count the shape names, the oracle's graph afterwards"""
    _, info, st = _shape(oracle, name)
    og = oracle.Graph(st)
    ref = NavRef.from_oracle(og)
    cands = D.candidates(ref)
    assert len(cands) == info["n_candidates"]
    k = info["k"]
    if "begin" in info:
        begin = [D.edge_of(ref, og, b) for b in info["begin"]]
        assert all(len(D._out(ref, b)) >= 2 for b in begin)                          # branching on either side of the limit
        assert all((b in cands) == (info["n_candidates"] > 0) for b in begin)
    if name in D.SPAN_SHAPES:
        j_end = k + 2 + info["span"]                                                  # the level of the end edge
        assert (j_end < 2 * k + 4) == info["pops"] and j_end in (2 * k + 2, 2 * k + 3, 2 * k + 4)
        for b in begin:
            assert D.search(ref, b, max_len=j_end) is None and D.search(ref, b, max_len=j_end + 1) is not None
    if name in D.BRANCH_SHAPES:
        for b in begin:
            assert D.search(ref, b, max_branches=info["H"] - 1) is None and D.search(ref, b, max_branches=info["H"]) is not None
    rounds = D.model_rounds(ref, cands, lambda b: True)
    assert rounds == info["n_rounds"]
    og.denovo(0, False, 0)
    assert np.array_equal(np.packbits(ref.invalid, bitorder="little"), og.invalid_now().view(np.uint8)[:(og.size + 7) // 8])


@pytest.mark.parametrize("name", D.BRANCH_SHAPES)
def test_oracle_undo_leaves_nothing(oracle, name):
    _, info, st = _shape(oracle, name)
    og = oracle.Graph(st)
    before = og.invalid_now()
    og.denovo(0, False, 0)
    assert np.array_equal(before, og.invalid_now())


@pytest.mark.parametrize("name", D.FAN_SHAPES + D.CHAIN_SHAPES)
def test_reach_regions_and_rounds(oracle, name):
    """the breadth-first walk of 2k + 4 levels over the numpy graph: every begin edge's region is in the regime the shape is built for
    (the chains: exactly at the limit or one edge past it), the strand that runs away from the fan is small; and the rounds the device's
    rules give for these regions are the ones the shape names -- with the verdict of the region at the limit turned round, the chains
    would take the other side's count"""
    _, info, st = _shape(oracle, name)
    og = oracle.Graph(st)
    ref = NavRef.from_oracle(og)
    assert og.size < 3.1e5
    begin = [D.edge_of(ref, og, b) for b in info["begin"]]
    regions = {b: D.region(ref, b) for b in begin}
    kinds = [D.verdict(*regions[b]) for b in begin]
    if name in D.FAN_SHAPES:
        S = info["S"]
        assert kinds == ([info["regime"]] + ["narrow"]) * S                            # (begin edges come as this strand's, the other strand's, per stem)
        seen, per_level = regions[begin[0]]
        if info["regime"] == "narrow":
            assert seen <= D.NARROW_MAX
        elif info["regime"] == "wide":
            assert D.NARROW_MAX < seen <= D.REACH_MAX and max(per_level) <= 100
        elif info["regime"] == "seen":
            assert seen > D.REACH_MAX and max(per_level) <= 1500
        else:
            assert max(per_level) > D.REACH_FRONTIER and per_level[info["k"] + 2 + D.FAN_TAIL + 5] >= 1500
    else:
        assert begin[0] < begin[1] < begin[4] < begin[5]                               # A < B < A' < B'
        seen, per_level = regions[begin[1]]
        assert kinds == ["narrow", ("wide", info["kind"])[info["over"]]] + ["narrow"] * 6
        if info["kind"] == "seen":
            assert seen == D.REACH_MAX + info["over"] and max(per_level) <= 1500
        else:
            assert max(per_level) == D.REACH_FRONTIER + info["over"] and seen < 8000
        turned = D.model_rounds(NavRef.from_oracle(og), sorted(begin), lambda b: b != begin[1] or bool(info["over"]))
        assert turned == 2 + (info["over"] ^ 1)
    fits = lambda b: D.verdict(*D.region(ref, b)) in ("narrow", "wide")
    assert D.model_rounds(ref, sorted(begin), fits) == info["n_rounds"]
    og.denovo(0, False, 0)
    assert np.array_equal(np.packbits(ref.invalid, bitorder="little"), og.invalid_now().view(np.uint8)[:(og.size + 7) // 8])


# ---- device ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    return api.Context(0)


def _device_runs(ctx, oracle, name, load):
    """every run of a shape: the device against the golden files (if the shape has them), the oracle and the derived numbers"""
    _, info, st = _shape(oracle, name)
    gold = _golden()[name]["runs"] if name in _golden() else [None] * len(info["runs"])
    for run, gd in zip(info["runs"], gold):
        og = oracle.Graph(st)
        want, wst = og.denovo(*run)
        g = load()
        before = g.invalid_bits()
        got, gst = g.denovo(*run)
        print(name, run, {key: gst[key] for key in ("n_tips", "n_bubbles", "n_bubble_candidates", "n_bubble_rounds", "n_contigs")})
        if gd is not None:
            assert _same_text(got, gd), (name, run)
            assert f"{gst['n_contigs']} {gst['total_len']}\n" == gd["info"]
        assert got == want, (name, run)
        assert (gst["n_tips"], gst["n_bubbles"]) == (wst["n_tips"], wst["n_bubbles"])
        assert np.array_equal(g.invalid_bits(), og.invalid_now()), (name, run)
        derived = _expected(info, run)
        assert {key: gst[key] for key in derived} == derived, (name, run)
        if not run[1]:
            for key, stat in (("n_candidates", "n_bubble_candidates"), ("n_rounds", "n_bubble_rounds")):
                if key in info:
                    assert gst[stat] == info[key], (name, run, stat)
        if name in D.BRANCH_SHAPES:
            assert np.array_equal(before, g.invalid_bits())                             # the undo leaves nothing behind
        g.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(D.SHAPES))
def test_device_on_designed_shapes(ctx, oracle, name):
    from megagta_amd import api
    st = _shape(oracle, name)[2]
    _device_runs(ctx, oracle, name, lambda: api.Graph(ctx, st.edges()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["span_k63_p1_s3", "span_k63_p2_s3", "fan_2100"])
def test_device_build_route(ctx, oracle, name):
    """reads -> device build -> resident graph -> the same checks"""
    from megagta_amd import api
    _, info, _ = _shape(oracle, name)
    packed, start = _SHAPES[name][3]

    def load():
        ctx.build_sdbg(ctx.upload_reads(packed, start), info["k"], min_count=1, collect=False)
        return api.Graph(ctx, None, info["k"])
    _device_runs(ctx, oracle, name, load)


@pytest.mark.gpu
def test_device_fan_walks_agree(ctx, oracle):
    """a region of a few thousand edges under MGTA_DENOVO_NARROW_MAX=24: the wave-wide walk from the first level on gives the same
    contigs and the same rounds"""
    from megagta_amd import api
    _, info, st = _shape(oracle, "fan_100")
    want, _ = oracle.Graph(st).denovo(0, False, 0)
    os.environ["MGTA_DENOVO_NARROW_MAX"] = "24"
    try:
        got, gst = api.Graph(ctx, st.edges()).denovo(0, False, 0)
    finally:
        del os.environ["MGTA_DENOVO_NARROW_MAX"]
    assert got == want and (gst["n_bubbles"], gst["n_bubble_rounds"]) == (info["n_bubbles"], info["n_rounds"])
