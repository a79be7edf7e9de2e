"""CPU only: what tests/test_walk_edges_gpu.py holds the window walks to (tests/walk_edges_ref.py) is itself pinned here.

1. the (k+1)-mer -> edge dict, built from the oracle's Label alone, agrees with the oracle's IndexBinarySearchEdge on present and absent
   windows, is injective, and leaves out exactly the edges that search never answers (those of tip nodes);
2. the inputs take the rare branches of the forward step (cov_step, csrc/walk.hpp), as conditions: the hint line before the target's line,
   an edge found in another line than the target node's last edge, a step from the graph's final edge, a step from an edge whose validity
   bit is set, a start edge with W > 4 -- and the census's own `found` column is the dict's answer, step for step;
3. the expectation of the read walks agrees with a count over strings that knows no graph, at k = 20.
"""
import numpy as np
import pytest

from tests import walk_edges_ref as X


@pytest.mark.parametrize("k", X.KS)
def test_dict_equals_the_index_search(oracle, k):
    w = X.get(k, oracle)
    og, ref, kmer, edge_of = w["og"], w["ref"], w["kmer"], w["edge_of"]
    assert og.size < 65535 and og.k == k
    keyed = np.nonzero((ref.W != 0) & ~ref.tip)[0]
    assert len(edge_of) == keyed.size                                       # injective: no two edges with one (k+1)-mer
    assert all(len(s) == k + 1 and set(s) <= set(X.DNA) for s in edge_of)
    tips = np.nonzero((ref.W != 0) & ref.tip)[0]
    assert tips.size > 0 and all(og.index_edge(kmer[e]) == -1 and kmer[e] not in edge_of for e in tips.tolist())    # never answered
    rng = np.random.default_rng(100 + k)
    present = rng.choice(keyed, 2500, replace=False).tolist() + [int(keyed[0]), int(keyed[-1])]
    for e in present:
        assert edge_of[kmer[e]] == e == og.index_edge(kmer[e]), e
    absent = []
    for e in rng.choice(keyed, 4000, replace=False).tolist():               # one letter changed: mostly absent, sometimes another edge
        at = int(rng.integers(0, k + 1))
        s = kmer[e][:at] + X.DNA[(X.DNA.index(kmer[e][at]) + int(rng.integers(1, 4))) % 4] + kmer[e][at + 1:]
        assert edge_of.get(s, -1) == og.index_edge(s), s
        absent.append(s not in edge_of)
    for _ in range(500):                                                    # random letters
        s = X.to_str(rng.integers(0, 4, k + 1))
        assert edge_of.get(s, -1) == og.index_edge(s), s
        absent.append(s not in edge_of)
    assert sum(absent) >= 2000
    # the restated ranks the census stands on, against the oracle's C calls
    for e in rng.choice(w["starts"], 300, replace=False).tolist() + [og.size - 1]:
        if ref.W[e]:
            assert int(ref.forward([e])[0]) == og.forward(e), e
        assert int(ref.rank_last([e])[0]) == og.rank_last(e) and [int(ref.rank_w(c, [e])[0]) for c in range(1, 5)] == [og.rank_w(c, e) for c in range(1, 5)]


@pytest.fixture(scope="module")
def final_edge_steps():
    return {}


@pytest.mark.parametrize("k", X.KS)
def test_inputs_take_every_branch_of_the_step(oracle, k, final_edge_steps, capsys):
    w = X.get(k, oracle)
    cz = X.census(w)
    n = X.census_counts(cz)
    with capsys.disabled():
        print(f"\n  census k {k:3d} edges {w['og'].size:6d} " + " ".join(f"{a} {b}" for a, b in n.items()), end="")
    assert w["og"].size < 65535
    assert n["hint_miss"] >= 1 and n["straddle"] >= 1 and n["invalid_found"] >= 1 and n["minus_found"] >= 1
    assert n["found"] >= 1000 and n["none"] >= 1000
    assert n["r_beyond"] == 0                                               # that branch is no condition: no step takes it
    final_edge_steps[k] = n["final_found"]
    # the census's own answer is the dict's: the step from e by c lands on the edge of label(e)[1:] + W(e) + c
    kmer, edge_of = w["kmer"], w["edge_of"]
    want = np.array([[edge_of.get(kmer[e][1:] + c, -1) for c in X.DNA] for e in cz["e"].tolist()], np.int64)
    assert np.array_equal(cz["found"], want)
    # the contigs and reads of the device test are what their names say
    two = X.step_contigs(w)
    assert len(two) == 4 * cz["e"].size and all(len(s) == k + 2 for s in two[:: 997])
    assert len(X.straddle_contigs(w, cz)) == 4 * n["straddle"]
    reads = X.walk_reads(w, cz)
    lens = {len(s) for s in reads}
    assert len(reads) >= X.MIN_READS and {0, k - 1, k, k + 1, k + 2} == lens
    have = set(reads)
    special = (cz["hint_miss"] | cz["final"] | cz["invalid"])[:, None] | cz["straddle"]
    assert all(two[4 * i + c] in have and X.rc(two[4 * i + c]) in have for i, c in zip(*np.nonzero(special)))


def test_some_graph_steps_from_its_final_edge(oracle, final_edge_steps):
    for k in X.KS:
        if k not in final_edge_steps:
            final_edge_steps[k] = X.census_counts(X.census(X.get(k, oracle)))["final_found"]
    assert sum(final_edge_steps.values()) >= 1, final_edge_steps


@pytest.mark.parametrize("k", X.DENOVO_KS)
def test_denovo_sets_validity_bits_the_walk_starts_from(oracle, k, capsys):
    """after `denovo` the walk does start from edges whose validity bit is set: found steps from edges that are no tips"""
    w = X.get(k, oracle)
    bits, _ = X.invalid_after_denovo(w, oracle)
    ref = w["ref"]
    assert not (ref.invalid & ~bits).any() and int((bits & ~ref.invalid).sum()) > 100
    cz = X.census(w, invalid=bits & ~ref.tip)
    n = X.census_counts(cz)
    with capsys.disabled():
        print(f"\n  after denovo k {k}: bits set {int(ref.invalid.sum())} -> {int(bits.sum())}, found steps from such an edge that is no tip {n['invalid_found']}", end="")
    assert n["invalid_found"] > 100
    found_on = bits[np.clip(cz["found"], 0, None)] & (cz["found"] >= 0)      # and steps that land ON such an edge: the scan does not skip it
    assert int(found_on.sum()) > 100


def test_read_expectation_equals_a_count_over_strings(oracle):
    k = 20
    w = X.get(k, oracle)
    reads = X.walk_reads(w, X.census(w))
    every = X.canon_contigs(w)
    numbers = sorted(set(X.canonical(w).values()))
    assert len(set(numbers)) == len(every) and 1 <= numbers[0] and numbers[-1] < 65536     # 16 bits tell any two apart, each has one set
    for reverse in (False, True):
        want = X.read_expectation(w, reads, reverse)
        hits, walked, searched = X.brute_force(w["read_strs"], k, [X.canon_contigs(w, b) for b in range(16)] + [every], reads, reverse)
        assert (walked, searched) == (want["walked"], want["searched"])
        for b in range(16):
            assert np.array_equal(hits[b], want["hits"][b]), b
        assert int(sum(hits[:16]).sum()) == sum(bin(int(c)).count("1") for c in want["canon"][want["canon"] >= 0].tolist()) > 10000
        assert np.array_equal(hits[16], want["found"])
    # per contig: the read windows equal to it on either strand, against a plain loop
    some = every[::len(every) // 60]
    got = X.window_counts(w, some, reads, False)
    all_windows = [s[p:p + k + 1] for s in reads for p in range(len(s) - k)]
    for c, n in zip(some, got.tolist()):
        assert n == sum(x == c or x == X.rc(c) for x in all_windows), c
    assert got.sum() > 60
